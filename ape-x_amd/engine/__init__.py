"""GPU-resident Ape-X engine (one rank = actor shard + HBM replay + learner)."""
from .vector import (VECTOR_ENVS, MLPDQNLearner, VectorActorShard, VectorApexEngine,  # noqa: F401
                     VectorEngineConfig, VectorEvaluator)
