"""GPU-resident Ape-X engine (one rank = actor shard + HBM replay + learner)."""
from .aql import AQLEngine, AQLEngineConfig, AQLEvaluator, AQLRolloutBuffers  # noqa: F401
from .aql_frame import AQLFrameConfig, AQLFrameEngine  # noqa: F401
from .dqn import DQNEngineConfig, DQNFrameEngine  # noqa: F401
from .vector import (VECTOR_ENVS, MLPDQNLearner, VectorActorShard, VectorApexEngine,  # noqa: F401
                     VectorEngineConfig, VectorEvaluator)
