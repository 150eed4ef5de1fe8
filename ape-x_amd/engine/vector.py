"""GPU Ape-X engine for vector-observation envs: the MLP dueling DQN of the reference's
``ApeX.py`` (MountainCar-v0, batch 64) and ``DQN.py`` (CartPole) with everything on one MI355X.

A vector observation is stored as a "frame" of ``4 * obs_dim`` bytes in the
:class:`~apex_amd.engine.hbm_replay.HBMReplay` frame ring, so the n-step batcher
(``nstep_emit``, both modes), the PER tree (``per_sample`` / ``per_write_batch``), the priority
mix, ``rmsprop_step`` with the StepLR fields and ``copy_f32`` are the Atari engine's kernels,
unchanged.  New HIP (``ops/csrc/vector_kernels.hip``): the env step, the acting forward with
the epsilon-greedy draw, and the learner's fused forward x3 / loss / backward.

Launch budget (kernel launches per step, all on the caller's stream, no host sync):

* actor step, 4 launches: ``vec_act`` (Q + epsilon-greedy) -> ``vec_classic_step`` ->
  ``nstep_emit`` (bumps the step counter) -> ``per_write_leaves`` (the E ring-ordered leaves and
  every tree level in one workgroup).
* learner SGD step, 5 launches at batch <= 64: ``per_sample`` -> ``vec_learn`` (target and
  online nets on s and s', double-DQN n-step Huber loss, per-sample backward vectors, the next
  step's PER beta) -> ``vec_grad`` (batch contraction into the flat gradient, no atomics, + the
  fp64 sum-of-squares partials ``grad_sumsq`` would produce) -> ``rmsprop_step`` (clip 40,
  centered RMSprop, early StepLR) -> ``per_write_batch`` (priority mix 0.9 max + 0.1 d + 1e-6,
  loss mean, step counter + 1; it walks <= 64 dirty paths inside its leaves launch, a larger
  batch adds one launch per tree level of more than 64 nodes).  ``fused_norm=False`` takes the
  norm from a separate ``grad_sumsq`` launch instead (6 launches).
* greedy evaluation: ``evaluate()`` is the stepwise yardstick (``vec_act`` ->
  ``vec_classic_step`` -> ``frame_hist_step`` + three torch ops per env step, a host sync every 50
  steps).  ``rollout_evaluate()`` is 1 launch + 1 read-back: ``vec_rollout`` plays every
  episode from reset to its first done inside one kernel, heads staged once, and returns the
  same floats bit for bit.  :class:`VectorEvaluator` is the non-blocking form, 2 launches per
  evaluation (``copy_f32`` snapshot on the training stream, ``vec_rollout`` on a side stream) +
  three async copies to pinned memory; eager, between graph replays.

Serial actor-then-learner on one stream; overlap and multi-GPU topologies are the Atari
engine's and are not offered here.  Envs other than ``VECTOR_ENVS`` -- any gym-API env with a
flat observation and a discrete action space, stepped on the CPU -- train under the same
replay and learner in :mod:`apex_amd.engine.vector_host`, which also overlaps the host's env
step with the learner.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass

import torch

from .. import ops
from ..models.dqn import DuelingDQN
from .evaluation import GreedyRollouts, RolloutBuffers, RolloutEvaluation
from .graphs import capture_graph, warm_up
from .hbm_replay import HBMReplay
from .shard import NStepShard

# env id -> (kind, obs_dim, n_actions, max_episode_steps); kind indexes the HIP env kernel
VECTOR_ENVS = {
    "CartPole-v0": (0, 4, 2, 200),
    "CartPole-v1": (0, 4, 2, 500),
    "MountainCar-v0": (1, 2, 3, 200),
}
MAX_BATCH = 1024
PARAM_KEYS = ("features.0.weight", "features.0.bias", "advantage.0.weight", "advantage.0.bias",
              "advantage.2.weight", "advantage.2.bias", "value.0.weight", "value.0.bias",
              "value.2.weight", "value.2.bias")


def env_spec(env_id: str) -> tuple[int, int, int, int]:
    if env_id not in VECTOR_ENVS:
        raise ValueError(f"GPU vector env must be one of {sorted(VECTOR_ENVS)}, got {env_id!r}")
    return VECTOR_ENVS[env_id]


def make_model(env_id: str) -> DuelingDQN:
    """The MLP ``DuelingDQN`` of ``env_id`` (reference state_dict keys)."""
    _, obs, n_actions, _ = env_spec(env_id)
    return DuelingDQN.from_shapes((obs,), n_actions)


def save_state_dict(model: DuelingDQN, path: str) -> str:
    """Reference-format checkpoint: ``torch.save(model.state_dict())`` on the CPU."""
    from ..utils.checkpoint import save_model

    return save_model(model, path)


def load_state_dict(path: str, env_id: str | None = None, model: DuelingDQN | None = None) -> DuelingDQN:
    from ..utils.checkpoint import load_model

    return load_model(model if model is not None else make_model(env_id), path)


def vec_net(hip, model: DuelingDQN):
    """``VecNet`` handle over the parameters of ``model`` (their storage must stay put)."""
    sd = dict(model.named_parameters())
    if tuple(sd) != PARAM_KEYS or model.cnn:
        raise ValueError("the vector kernels take the MLP form of DuelingDQN")
    for k, p in sd.items():
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"{k}: contiguous fp32 expected")
    d = {k: p.data_ptr() for k, p in sd.items()}
    d.update(obs=model.input_shape[0], A=model.num_actions)
    return hip.make_vec_net(d)


class VectorActorShard(NStepShard):
    """E vectorised classic-control envs over an ``HBMReplay`` whose frames are observations
    (``frame_bytes = 4 * obs_dim``): same surface as :class:`ActorShard` (``reset``,
    ``act_and_step``, ``episode_stats``, the ``st`` dict of the n-step batcher)."""

    def __init__(self, replay: HBMReplay, n_envs: int, env_id: str, n_step: int = 3, gamma: float = 0.99,
                 eps_base: float = 0.4, eps_alpha: float = 7.0, actor_offset: int = 0,
                 total_actors: int | None = None, seed: int = 0, mode: str = "reference",
                 max_episode_steps: int | None = None):
        self.env_id = env_id
        self.kind, self.obs_dim, n_actions, limit = env_spec(env_id)
        self.max_episode_steps = int(limit if max_episode_steps is None else max_episode_steps)
        if replay.frame_bytes != 4 * self.obs_dim:
            raise ValueError(f"replay frame_bytes must be 4 * obs_dim = {4 * self.obs_dim}")
        super().__init__(replay, n_envs, n_actions, n_step, gamma, eps_base, eps_alpha, actor_offset, total_actors,
                         seed, mode)
        E = self.E
        self.layout = self.hip.vec_env_state_layout()
        self.env_state = torch.zeros(E, self.layout["STRIDE"], dtype=torch.float32, device=self.device)
        self.ring = replay.frames.view(torch.float32)  # [F, obs_dim]
        self.env = self.hip.make_vec_env(self.kind, E, self.obs_dim, replay.frame_capacity, self.max_episode_steps,
                                         self.env_state.data_ptr(), self.ring.data_ptr(), self.seed)
        self._act = None
        self.reset()

    def set_policy(self, model: DuelingDQN) -> None:
        """Act with ``model`` (its parameter storage is read in place by every later step)."""
        if model.input_shape != (self.obs_dim,) or model.num_actions != self.A:
            raise ValueError("policy shape does not match the env")
        self._policy = model
        self._act = self.hip.make_vec_act(vec_net(self.hip, model), self.ring.data_ptr(), self.st["hist"].data_ptr(),
                                          self.E, self.eps.data_ptr(), self.act_seed,
                                          self.step_counter.data_ptr(), self.q.data_ptr(), self.actions.data_ptr())

    def reset(self) -> None:
        self.hip.vec_classic_reset(self.env, self.step_counter.data_ptr(), self.new_frame.data_ptr(),
                                   self.st["hist"].data_ptr(), self.ep_log.data_ptr(), self._stream())

    def observe(self) -> torch.Tensor:
        """Current observations f32 [E, obs_dim] (a gather from the ring; allocates)."""
        return self.ring[self.st["hist"][:, 3].long()]

    def act(self) -> None:
        """Q of the current observations into ``self.q`` and the epsilon-greedy actions."""
        if self._act is None:
            raise RuntimeError("set_policy() first: acting needs the HIP forward's weights")
        self.hip.vec_act(self._act, self._stream())

    def env_step(self) -> None:
        self.hip.vec_classic_step(self.env, self.actions.data_ptr(), self.step_counter.data_ptr(),
                                  self.reward.data_ptr(), self.done.data_ptr(), self.new_frame.data_ptr(),
                                  self.ep_log.data_ptr(), self._stream())

    def act_and_step(self, selected: bool = False, tree: bool = True) -> None:
        """One actor step of all envs.  ``selected``: ``self.actions`` (and ``self.q``) already
        hold this step's actions and Q.  ``tree=False``: rows only, no priority-tree write."""
        if not selected:
            self.act()
        self.env_step()
        self._emit(self.nstep, self.slot, self.prio, True)  # (the kernel bumps the counter)
        if tree:  # unique ring-ordered slots: leaves and every level in one launch
            self.replay.write_priorities(self.slot, self.prio, dedup=False, bumps=((self.replay.filled, self.E),))


@dataclass
class VectorEngineConfig:
    """Defaults: the reference's ``ApeX.py`` configuration."""
    env_id: str = "MountainCar-v0"
    n_envs: int = 256
    batch_size: int = 64
    n_step: int = 3
    gamma: float = 0.99
    lr: float = 1e-5
    rms_alpha: float = 0.95
    rms_eps: float = 1.5e-7
    centered: bool = True
    lr_gamma: float = 0.99
    lr_step_size: int = 1000
    lr_step_offset: int = 1          # scheduler.step() before optimizer.step()
    max_norm: float = 40.0
    replay_capacity: int = 1_000_000
    alpha: float = 0.6
    beta: float = 0.4
    beta_horizon: float = 1000.0
    publish_param_interval: int = 32
    target_update_interval: int = 2500
    threshold_size: int | None = None   # learning starts once len(replay) > this (default: batch_size)
    actor_steps_per_learner_step: int = 1
    nstep_mode: str = "reference"
    eps_base: float = 0.4
    eps_alpha: float = 7.0
    fused_norm: bool = True          # grad-norm partials from the gradient launch (5 launches per SGD step)
    seed: int = 0

    def validate(self, device_env: bool = True) -> "VectorEngineConfig":
        """``device_env=False``: ``env_id`` is only a label (the host-env engine takes its shapes
        from the vector env)."""
        if device_env:
            env_spec(self.env_id)
        if not 1 <= self.batch_size <= MAX_BATCH:
            raise ValueError(f"batch_size must be in [1, {MAX_BATCH}]")
        if self.nstep_mode not in ("reference", "textbook"):
            raise ValueError("nstep_mode must be 'reference' or 'textbook'")
        if self.n_envs < 1 or not 1 <= self.n_step <= 16:
            raise ValueError("n_envs >= 1 and n_step in [1, 16]")
        if self.n_envs > 4096:
            raise ValueError("n_envs <= 4096 (the actor step's one-launch tree write)")
        if self.replay_capacity < 2 * self.n_envs:
            raise ValueError("replay_capacity must hold at least two actor steps")
        if self.actor_steps_per_learner_step < 1:
            raise ValueError("actor_steps_per_learner_step >= 1")
        return self


class MLPDQNLearner:
    """Device-resident learner of the MLP dueling DQN over an observation-ring ``HBMReplay``
    (see the module docstring for the launch sequence)."""

    def __init__(self, model: DuelingDQN, replay: HBMReplay, cfg: VectorEngineConfig):
        self.hip = h = ops.hip()
        self.cfg = cfg
        self.replay = replay
        self.device = dev = replay.device
        self.model = model.to(dev)
        self.flat = self.model.flatten_parameters()
        self.target = copy.deepcopy(self.model)
        self.target._flat = None
        self.tflat = self.target.flatten_parameters()
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.P = self.flat.numel()
        self.obs_dim, self.A = self.model.input_shape[0], self.model.num_actions
        if replay.frame_bytes != 4 * self.obs_dim:
            raise ValueError("replay frame_bytes must be 4 * obs_dim")
        if self.P != h.vec_param_count(self.obs_dim, self.A):
            raise ValueError("unexpected parameter count for the MLP dueling net")
        self.segments = self.model.param_segments()
        assert tuple(n for n, _, _ in self.segments) == PARAM_KEYS
        B, A = int(cfg.batch_size), self.A
        self.B = B
        f32 = dict(dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(self.P, **f32)
        off = 0
        for p in self.model.parameters():
            n = p.numel()
            p.grad = self.flat_grad[off:off + n].view_as(p)
            off += n
        self.opt_s1 = torch.zeros(self.P, **f32)
        self.opt_s2 = torch.zeros(self.P, **f32)
        self.hp = h.RMSpropParams(cfg.lr, cfg.rms_alpha, cfg.rms_eps, cfg.max_norm, cfg.lr_gamma, cfg.lr_step_size,
                                  cfg.lr_step_offset, cfg.centered)
        self.idx = torch.zeros(B, dtype=torch.int32, device=dev)
        self.w = torch.zeros(B, **f32)
        self.q_s = torch.zeros(B, A, **f32)
        self.q_s2 = torch.zeros(B, A, **f32)
        self.qt_s2 = torch.zeros(B, A, **f32)
        self.lay = h.vec_layout()
        self.vec = torch.zeros(B, self.lay["STRIDE"], **f32)
        self.delta = torch.zeros(B, **f32)
        self.lw = torch.zeros(B, **f32)
        self.prio = torch.zeros(B, **f32)
        self.loss = torch.zeros(1, **f32)
        self.norms = torch.zeros(4, **f32)   # l2, (unused), clip coef, lr
        self.step_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        # PER beta, annealed on the device: vec_learn writes beta_by_frame(step + 1) for the next draw
        self.beta = torch.full((1,), float(cfg.beta), **f32)
        self.nblk = h.vec_grad_blocks(self.P)
        self.part = torch.zeros(self.nblk, dtype=torch.float64, device=dev)
        self.partials = torch.zeros(h.grad_norm_partials(), dtype=torch.float64, device=dev)
        self.ring = replay.frames.view(torch.float32)
        self.net = vec_net(h, self.model)
        self.tnet = vec_net(h, self.target)
        self.L = h.make_vec_learn(self.net, self.tnet, dict(
            replay.trans_ptrs(), ring=self.ring.data_ptr(), idx=self.idx.data_ptr(), w=self.w.data_ptr(), B=B,
            gamma_n=float(cfg.gamma ** cfg.n_step), q_s=self.q_s.data_ptr(), q_s2=self.q_s2.data_ptr(),
            qt_s2=self.qt_s2.data_ptr(), vec=self.vec.data_ptr(), delta=self.delta.data_ptr(),
            lw=self.lw.data_ptr(), step=self.step_counter.data_ptr(), beta_out=self.beta.data_ptr(),
            beta0=float(cfg.beta), beta_horizon=float(cfg.beta_horizon)))
        self.G = h.make_vec_grad(self.vec.data_ptr(), B, self.obs_dim, A, self.P, self.flat_grad.data_ptr(),
                                 self.part.data_ptr())

    @staticmethod
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream

    def sample(self) -> None:
        self.replay.sample_indices(self.B, self.idx, self.w, self.step_counter, self.beta)

    def forward_backward(self) -> None:
        """Q(s), Q(s'), Q_target(s'), loss terms and the flat gradient of the rows in ``idx``."""
        s = self._stream()
        self.hip.vec_learn(self.L, s)
        self.hip.vec_grad(self.G, s)

    def optimize(self) -> None:
        h, s = self.hip, self._stream()
        if self.cfg.fused_norm:
            parts, nparts = self.part, self.nblk
        else:
            h.grad_sumsq(self.flat_grad.data_ptr(), self.P, self.partials.data_ptr(), s)
            parts, nparts = self.partials, self.partials.numel()
        h.rmsprop_step(self.flat.data_ptr(), self.flat_grad.data_ptr(), self.opt_s1.data_ptr(),
                       self.opt_s2.data_ptr(), self.P, parts.data_ptr(), nparts, self.hp,
                       self.step_counter.data_ptr(), self.norms.data_ptr(), s)

    def write_priorities(self) -> None:
        """0.9 max + 0.1 delta + 1e-6 into the tree, the loss mean, step counter + 1."""
        self.replay.write_batch(idx=self.idx, mix=(self.delta, self.lw, self.prio, self.loss),
                                bump=self.step_counter)

    def step(self) -> None:
        self.sample()
        self.forward_backward()
        self.optimize()
        self.write_priorities()

    def sync_target(self) -> None:
        self.hip.copy_f32(self.tflat.data_ptr(), self.flat.data_ptr(), self.P, self._stream())

    def copy_params_to(self, dst_flat: torch.Tensor) -> None:
        self.hip.copy_f32(dst_flat.data_ptr(), self.flat.data_ptr(), self.P, self._stream())

    def state_dict(self):
        return self.model.state_dict()

    def stats(self) -> dict:
        """Host-side view of the last step's scalars (forces a sync; call rarely): the keys of
        ``DQNLearner.stats()``; ``grad_norm`` is the reference's logged value."""
        n = self.norms.tolist()
        ref = sum(self.flat_grad[o:o + k].norm().item() ** 0.5 for _, o, k in self.segments) ** 0.5
        return {"loss": float(self.loss.item()), "grad_norm_l2": n[0], "grad_norm": ref, "clip": n[2], "lr": n[3]}


class VectorApexEngine(GreedyRollouts):
    """Actor shard + observation-ring replay + MLP learner on one GPU."""

    def __init__(self, cfg: VectorEngineConfig, device: str | torch.device = "cuda"):
        self.cfg = cfg.validate()
        self.device = dev = torch.device(device)
        self.hip = ops.hip()
        self.kind, self.obs_dim, self.A, self.limit = env_spec(cfg.env_id)
        torch.manual_seed(cfg.seed)
        model = make_model(cfg.env_id)
        self.replay = HBMReplay(cfg.replay_capacity, cfg.n_envs, cfg.n_step, cfg.alpha, dev,
                                frame_bytes=4 * self.obs_dim, seed=cfg.seed + 17)
        self.learner = MLPDQNLearner(model, self.replay, cfg)
        self.actor_model = make_model(cfg.env_id).to(dev)
        self.actor_flat = self.actor_model.flatten_parameters()
        self.shard = VectorActorShard(self.replay, cfg.n_envs, cfg.env_id, cfg.n_step, cfg.gamma, cfg.eps_base,
                                      cfg.eps_alpha, seed=cfg.seed * 0x2545F491 + 0xAC7, mode=cfg.nstep_mode)
        self.shard.set_policy(self.actor_model)
        self.publish_params()
        self.learn_steps = 0
        self.actor_steps = 0
        self._g_actor = self._g_learn = None
        self._eval = None

    # ------------------------------------------------------------------ phases
    def publish_params(self) -> None:
        self.learner.copy_params_to(self.actor_flat)

    def _actor_body(self) -> None:
        self.shard.act_and_step()

    def actor_step(self) -> None:
        if self._g_actor is not None:
            self._g_actor.replay()
        else:
            self._actor_body()
        self.actor_steps += 1

    def learner_step(self) -> None:
        if self._g_learn is not None:
            self._g_learn.replay()
        else:
            self.learner.step()
        self.learn_steps += 1
        if self.learn_steps % self.cfg.publish_param_interval == 0:
            self.publish_params()
        if self.learn_steps % self.cfg.target_update_interval == 0:
            self.learner.sync_target()

    def fill(self, min_transitions: int | None = None) -> None:
        """Act until the replay holds more than ``threshold_size`` slots (ApeX.py: learning
        starts once ``len(buffer) > batch_size``)."""
        thr = self.cfg.threshold_size if self.cfg.threshold_size is not None else self.cfg.batch_size
        need = (thr if min_transitions is None else int(min_transitions)) + 1
        # n-step rows trail the env steps: the first n steps of an env emit nothing
        steps = -(-need // self.cfg.n_envs) + self.cfg.n_step
        for _ in range(steps):
            self.actor_step()

    def train_step(self) -> None:
        """One learner SGD step + its actor steps."""
        self.learner_step()
        for _ in range(self.cfg.actor_steps_per_learner_step):
            self.actor_step()

    def capture(self, warmup_iters: int = 3) -> None:
        """Warm up on a side stream (real, counted train steps), then capture the actor step
        and the learner step as hipGraphs."""
        warm_up(self.device, self.train_step, warmup_iters)
        torch.cuda.synchronize(self.device)
        self._pool = torch.cuda.graph_pool_handle()
        self._g_actor = capture_graph(self._actor_body, self._pool)
        self._g_learn = capture_graph(self.learner.step, self._pool)
        torch.cuda.synchronize(self.device)

    def run(self, n_steps: int) -> float:
        import time

        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        for _ in range(n_steps):
            self.train_step()
        torch.cuda.synchronize(self.device)
        return time.perf_counter() - t0

    def save(self, path: str) -> str:
        """Reference-format ``state_dict`` of the online network."""
        return save_state_dict(self.learner.model, path)

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, episodes: int = 10, seed: int | None = None) -> list[float]:
        """Greedy (epsilon = 0) returns of ``episodes`` episodes with the online weights, one
        env each, on a separate small shard with its own observation ring: nothing is written
        to the replay."""
        h, dev = self.hip, self.device
        n = int(episodes)
        if self._eval is None or self._eval["n"] != n:
            ring = torch.zeros(4 * n, self.obs_dim, dtype=torch.float32, device=dev)
            lay = h.vec_env_state_layout()
            ev = {"n": n, "ring": ring, "state": torch.zeros(n, lay["STRIDE"], dtype=torch.float32, device=dev),
                  "hist": torch.zeros(n, 4, dtype=torch.int32, device=dev),
                  "new_frame": torch.zeros(n, dtype=torch.int32, device=dev),
                  "ep_log": torch.zeros(n, 4, dtype=torch.float32, device=dev),
                  "q": torch.zeros(n, self.A, dtype=torch.float32, device=dev),
                  "actions": torch.zeros(n, dtype=torch.int32, device=dev),
                  "reward": torch.zeros(n, dtype=torch.float32, device=dev),
                  "done": torch.zeros(n, dtype=torch.float32, device=dev),
                  "eps": torch.zeros(n, dtype=torch.float32, device=dev),
                  "counter": torch.zeros(1, dtype=torch.int64, device=dev)}
            ev["act"] = h.make_vec_act(self.learner.net, ring.data_ptr(), ev["hist"].data_ptr(), n,
                                       ev["eps"].data_ptr(), 0, ev["counter"].data_ptr(), ev["q"].data_ptr(),
                                       ev["actions"].data_ptr())
            self._eval = ev
        ev = self._eval
        env = h.make_vec_env(self.kind, n, self.obs_dim, ev["ring"].shape[0], self.limit, ev["state"].data_ptr(),
                             ev["ring"].data_ptr(), self._eval_seed(seed))
        s = torch.cuda.current_stream().cuda_stream
        ev["counter"].zero_()
        h.vec_classic_reset(env, ev["counter"].data_ptr(), ev["new_frame"].data_ptr(), ev["hist"].data_ptr(),
                            ev["ep_log"].data_ptr(), s)
        first = torch.zeros(n, dtype=torch.float32, device=dev)
        got = torch.zeros(n, dtype=torch.bool, device=dev)
        for t in range(self.limit):
            h.vec_act(ev["act"], s)
            h.vec_classic_step(env, ev["actions"].data_ptr(), ev["counter"].data_ptr(), ev["reward"].data_ptr(),
                               ev["done"].data_ptr(), ev["new_frame"].data_ptr(), ev["ep_log"].data_ptr(), s)
            h.frame_hist_step(ev["hist"].data_ptr(), ev["new_frame"].data_ptr(), ev["done"].data_ptr(), n,
                              ev["counter"].data_ptr(), s)
            fin = (ev["done"] > 0) & ~got
            first = torch.where(fin, ev["ep_log"][:, 0], first)
            got |= fin
            if (t + 1) % 50 == 0 and bool(got.all()):
                break
        return first.tolist()

    # ---- GreedyRollouts: ``rollout_evaluate()`` is ``evaluate()`` in one ``vec_rollout`` launch
    _eval_steps = property(lambda self: self.learn_steps)
    _eval_limit = property(lambda self: self.limit)

    def _make_rollout(self, n: int) -> VecRolloutBuffers:
        return VecRolloutBuffers(self.hip, self.learner.net, self.kind, self.obs_dim, n, self.device)


class VecRolloutBuffers(RolloutBuffers):
    """Device outputs of ``vec_rollout`` for ``n`` episodes of one net + the launch."""

    def __init__(self, hip, net, kind: int, obs_dim: int, n: int, device):
        super().__init__(n, device)
        self.hip, self.net, self.kind, self.obs_dim = hip, net, int(kind), int(obs_dim)

    def launch(self, seed: int, max_steps: int, trace: dict | None = None) -> None:
        """One ``vec_rollout`` launch on the current stream.  ``trace``: the tensors
        ``obs`` f32 [n, T, obs_dim], ``q`` f32 [n, T, A] and ``act`` i32 [n, T]."""
        d = dict(kind=self.kind, N=self.n, obs=self.obs_dim, max_steps=int(max_steps), seed=int(seed),
                 returns=self.returns.data_ptr(), lengths=self.lengths.data_ptr(), ended=self.ended.data_ptr())
        if trace is not None:
            d.update(trace_obs=trace["obs"].data_ptr(), trace_q=trace["q"].data_ptr(),
                     trace_act=trace["act"].data_ptr(), trace_T=int(trace["obs"].shape[1]))
        self.hip.vec_rollout(self.hip.make_vec_rollout(self.net, d), torch.cuda.current_stream().cuda_stream)


class VectorEvaluator(RolloutEvaluation):
    """Greedy evaluation beside training (:class:`~apex_amd.engine.evaluation.SideStreamEvaluation`):
    ``launch()`` snapshots the online weights on the training stream (``copy_f32``) and plays the
    episodes with ``vec_rollout`` on a side stream; a result holds their ``returns``, ``lengths``
    and ``ended`` flags."""

    def __init__(self, engine: VectorApexEngine, episodes: int = 10, max_episode_steps: int | None = None,
                 **side):
        if not isinstance(engine, VectorApexEngine):
            raise TypeError("VectorEvaluator plays vec_rollout's device envs: it needs a VectorApexEngine; a "
                            "host-env engine evaluates on the host (VectorHostEngine.evaluate)")
        self.hip, self.n = engine.hip, int(episodes)
        self.model = copy.deepcopy(engine.learner.model)   # the snapshot
        self.model._flat = None
        self.flat = self.model.flatten_parameters()
        for p in self.model.parameters():
            p.requires_grad_(False)
        ro = VecRolloutBuffers(self.hip, vec_net(self.hip, self.model), engine.kind, engine.obs_dim, self.n,
                               engine.device)
        super().__init__(engine, ro, engine.limit if max_episode_steps is None else max_episode_steps, **side)

    def _snapshot(self) -> None:
        self.engine.learner.copy_params_to(self.flat)
