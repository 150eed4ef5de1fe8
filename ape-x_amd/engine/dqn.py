"""GPU engine of the single-process prioritized double-DQN trainer (reference ``DQN.py``,
BASELINE config 1; the host loop is ``trainers/dqn.py``): env, acting, PER and the SGD step of
one frame on one MI355X, six launches on the caller's stream, no host sync.

Every cadence is ``DQN.py``'s, not Ape-X's: epsilon(t) and beta(t) by frame index, inserts at
the running max priority, n = 1, Adam without clipping, one SGD step per frame acting with the
online weights, target sync on frames divisible by the interval (frame 0 included).

One frame (frame counter ``t`` on the device):

1. ``dqn_frame`` (``ops/csrc/vector_kernels.hip``, one workgroup): epsilon(t) / beta(t), Q of
   the E <= 8 envs' observations on the online net, the epsilon-greedy draw, the env step, the
   transition of env e into slot ``(filled + e) mod C`` with its leaf at ``max_prio^alpha`` and
   every level of its path, ``filled += E``, ``t += 1``.
2. ``per_sample`` (beta from 1.; exclusive-end mass unless ``exact_mass``)
3. ``vec_learn`` (``gamma_n = gamma``)
4. ``vec_grad`` (flat gradient + the norm partials)
5. ``adam_step`` (early StepLR)
6. ``per_write_batch`` (0.9 max + 0.1 delta + 1e-6; raises ``max_prio``; SGD counter + 1)

Launches 2-6 start on the first frame where ``(t + 1) E > batch_size`` (``DQN.py``:
``len(buffer) > batch_size`` after the frame's insert); the host knows that index.  The target
sync is an eager ``copy_f32`` between graph replays.  ``t`` counts loop iterations: with E > 1
one iteration steps all E envs and takes one SGD step.
"""
from __future__ import annotations

import copy
import time
from dataclasses import dataclass

import torch

from .. import ops
from .evaluation import GreedyRollouts
from .graphs import capture_graph, warm_up
from .hbm_replay import HBMReplay
from .shard import ACT_SEED_XOR
from .vector import MAX_BATCH, PARAM_KEYS, VecRolloutBuffers, env_spec, make_model, save_state_dict, vec_net

MAX_ENVS = 8   # rows of one forward pass of a workgroup (vector_kernels.hip kRows)


@dataclass
class DQNEngineConfig:
    """Defaults: the reference's ``DQN.py`` constructor."""
    env_id: str = "CartPole-v0"
    n_envs: int = 1
    batch_size: int = 32
    gamma: float = 0.99
    replay_capacity: int = 100_000
    alpha: float = 0.6
    beta: float = 0.4
    beta_horizon: float = 1000.0
    eps_start: float = 1.0
    eps_final: float = 0.01
    eps_decay: float = 500.0
    lr: float = 1e-3
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_eps: float = 1e-8
    weight_decay: float = 0.0
    max_norm: float = 0.0            # no clipping
    lr_gamma: float = 0.99
    lr_step_size: int = 1000
    lr_step_offset: int = 1          # scheduler.step() before optimizer.step()
    target_update_interval: int = 1000
    exact_mass: bool = False         # False: the reference's exclusive-end mass
    max_episode_steps: int | None = None   # None: the env's registered TimeLimit
    seed: int = 0

    def validate(self) -> "DQNEngineConfig":
        env_spec(self.env_id)
        if not 1 <= self.n_envs <= MAX_ENVS:
            raise ValueError(f"n_envs must be in [1, {MAX_ENVS}] (one workgroup's forward pass)")
        if not 1 <= self.batch_size <= MAX_BATCH:
            raise ValueError(f"batch_size must be in [1, {MAX_BATCH}]")
        if self.replay_capacity <= self.batch_size or self.replay_capacity < 2 * self.n_envs:
            raise ValueError("replay_capacity must exceed batch_size and hold two frames")
        if not (self.eps_decay > 0 and self.beta_horizon > 0):
            raise ValueError("eps_decay and beta_horizon must be > 0")
        if self.target_update_interval < 1:
            raise ValueError("target_update_interval >= 1")
        if self.max_episode_steps is not None and self.max_episode_steps < 1:
            raise ValueError("max_episode_steps >= 1")
        return self

    def first_learning_frame(self) -> int:
        """The first frame index t whose insert leaves ``len(buffer) = (t + 1) E > batch_size``."""
        return self.batch_size // self.n_envs


class DQNFrameEngine(GreedyRollouts):
    """``DQN.py`` on one GPU: ``frame()`` is one loop iteration of the reference trainer."""

    def __init__(self, cfg: DQNEngineConfig, device: str | torch.device = "cuda"):
        self.cfg = cfg.validate()
        self.device = dev = torch.device(device)
        self.hip = h = ops.hip()
        self.kind, self.obs_dim, self.A, limit = env_spec(cfg.env_id)
        self.limit = int(limit if cfg.max_episode_steps is None else cfg.max_episode_steps)
        E, A, B = int(cfg.n_envs), self.A, int(cfg.batch_size)
        self.E, self.B = E, B
        torch.manual_seed(cfg.seed)
        self.replay = rp = HBMReplay(cfg.replay_capacity, E, 1, cfg.alpha, dev, frame_bytes=4 * self.obs_dim,
                                     exact_mass=cfg.exact_mass, seed=cfg.seed + 17)
        self.model = make_model(cfg.env_id).to(dev)
        self.flat = self.model.flatten_parameters()
        self.target = copy.deepcopy(self.model)
        self.target._flat = None
        self.tflat = self.target.flatten_parameters()
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.P = self.flat.numel()
        if self.P != h.vec_param_count(self.obs_dim, A):
            raise ValueError("unexpected parameter count for the MLP dueling net")
        self.segments = self.model.param_segments()
        assert tuple(n for n, _, _ in self.segments) == PARAM_KEYS
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        # ---- actor side
        self.env_seed = (cfg.seed * 0x2545F491 + 0xAC7) & 0xFFFFFFFFFFFF
        self.act_seed = self.env_seed ^ ACT_SEED_XOR   # VectorActorShard's key of the action draw
        self.layout = h.vec_env_state_layout()
        self.env_state = torch.zeros(E, self.layout["STRIDE"], **f32)
        self.hist = torch.zeros(E, 4, **i32)
        self.new_frame = torch.zeros(E, **i32)
        self.ep_log = torch.zeros(E, 4, **f32)   # last return, last length, episodes, sum of returns
        self.q = torch.zeros(E, A, **f32)
        self.actions = torch.zeros(E, **i32)
        self.reward = torch.zeros(E, **f32)
        self.done = torch.zeros(E, **f32)
        self.slot = torch.zeros(E, **i32)
        self.t = torch.zeros(1, **i64)           # frame counter
        self.eps = torch.zeros(1, **f32)
        self.beta = torch.full((1,), float(cfg.beta), **f32)
        self.ring = rp.frames.view(torch.float32)   # [F, obs_dim]
        self.env = h.make_vec_env(self.kind, E, self.obs_dim, rp.frame_capacity, self.limit,
                                  self.env_state.data_ptr(), self.ring.data_ptr(), self.env_seed)
        self.net = vec_net(h, self.model)
        self.tnet = vec_net(h, self.target)
        self.F = h.make_dqn_frame(self.net, self.env, rp.tree, rp.trans_ptrs(), dict(
            act_seed=self.act_seed, hist=self.hist.data_ptr(), t=self.t.data_ptr(),
            eps_start=float(cfg.eps_start), eps_final=float(cfg.eps_final), eps_decay=float(cfg.eps_decay),
            beta0=float(cfg.beta), beta_horizon=float(cfg.beta_horizon), eps_out=self.eps.data_ptr(),
            beta_out=self.beta.data_ptr(), q=self.q.data_ptr(), actions=self.actions.data_ptr(),
            reward=self.reward.data_ptr(), done=self.done.data_ptr(), new_frame=self.new_frame.data_ptr(),
            ep_log=self.ep_log.data_ptr(), C=rp.capacity, filled=rp.filled.data_ptr(), slot=self.slot.data_ptr(),
            max_prio=rp.max_prio.data_ptr(), alpha=float(cfg.alpha)))
        # ---- learner side
        self.flat_grad = torch.zeros(self.P, **f32)
        off = 0
        for p in self.model.parameters():
            n = p.numel()
            p.grad = self.flat_grad[off:off + n].view_as(p)
            off += n
        self.opt_m = torch.zeros(self.P, **f32)
        self.opt_v = torch.zeros(self.P, **f32)
        self.hp = h.AdamParams(cfg.lr, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, cfg.weight_decay, cfg.max_norm,
                               cfg.lr_gamma, cfg.lr_step_size, cfg.lr_step_offset)
        self.idx = torch.zeros(B, **i32)
        self.w = torch.zeros(B, **f32)
        self.q_s = torch.zeros(B, A, **f32)
        self.q_s2 = torch.zeros(B, A, **f32)
        self.qt_s2 = torch.zeros(B, A, **f32)
        self.vec = torch.zeros(B, h.vec_layout()["STRIDE"], **f32)
        self.delta = torch.zeros(B, **f32)
        self.lw = torch.zeros(B, **f32)
        self.prio = torch.zeros(B, **f32)
        self.loss = torch.zeros(1, **f32)
        self.norms = torch.zeros(4, **f32)       # l2, (unused), clip coef, lr
        self.step_counter = torch.zeros(1, **i64)   # SGD steps (Adam's t, the StepLR, the PER draw's counter)
        self.nblk = h.vec_grad_blocks(self.P)
        self.part = torch.zeros(self.nblk, dtype=torch.float64, device=dev)
        # VecLearn::beta_out stays null: beta(t) is the frame kernel's
        self.L = h.make_vec_learn(self.net, self.tnet, dict(
            rp.trans_ptrs(), ring=self.ring.data_ptr(), idx=self.idx.data_ptr(), w=self.w.data_ptr(), B=B,
            gamma_n=float(cfg.gamma), q_s=self.q_s.data_ptr(), q_s2=self.q_s2.data_ptr(),
            qt_s2=self.qt_s2.data_ptr(), vec=self.vec.data_ptr(), delta=self.delta.data_ptr(),
            lw=self.lw.data_ptr(), step=self.step_counter.data_ptr()))
        self.G = h.make_vec_grad(self.vec.data_ptr(), B, self.obs_dim, A, self.P, self.flat_grad.data_ptr(),
                                 self.part.data_ptr())
        self.first_learning_frame = cfg.first_learning_frame()
        self.learning = True    # False: frames run launch 1 only (the insert path on its own)
        self.frames = 0         # host mirror of ``t``
        self.learn_steps = 0
        self._graph = None
        h.vec_classic_reset(self.env, self.t.data_ptr(), self.new_frame.data_ptr(), self.hist.data_ptr(),
                            self.ep_log.data_ptr(), self._stream())

    @staticmethod
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream

    # ------------------------------------------------------------------ the frame
    def act_insert(self) -> None:
        """Launch 1: the actor side of the frame (epsilon / beta, act, env step, insert)."""
        self.hip.dqn_frame(self.F, self._stream())

    def sample(self) -> None:
        self.replay.sample_indices(self.B, self.idx, self.w, self.step_counter, self.beta)

    def forward_backward(self) -> None:
        s = self._stream()
        self.hip.vec_learn(self.L, s)
        self.hip.vec_grad(self.G, s)

    def optimize(self) -> None:
        self.hip.adam_step(self.flat.data_ptr(), self.flat_grad.data_ptr(), self.opt_m.data_ptr(),
                           self.opt_v.data_ptr(), self.P, self.part.data_ptr(), self.nblk, self.hp,
                           self.step_counter.data_ptr(), self.norms.data_ptr(), self._stream())

    def write_priorities(self) -> None:
        self.replay.write_batch(idx=self.idx, mix=(self.delta, self.lw, self.prio, self.loss),
                                bump=self.step_counter)

    def sgd_step(self) -> None:
        """Launches 2-6."""
        self.sample()
        self.forward_backward()
        self.optimize()
        self.write_priorities()

    def _full_frame(self) -> None:
        self.act_insert()
        self.sgd_step()

    def sync_target(self) -> None:
        self.hip.copy_f32(self.tflat.data_ptr(), self.flat.data_ptr(), self.P, self._stream())

    def frame(self) -> None:
        """One iteration of ``DQN.py``'s loop at frame index ``self.frames``."""
        t = self.frames
        if self.learning and t >= self.first_learning_frame:
            if self._graph is not None:
                self._graph.replay()
            else:
                self._full_frame()
            self.learn_steps += 1
        else:
            self.act_insert()
        if t % self.cfg.target_update_interval == 0:
            self.sync_target()
        self.frames = t + 1

    def capture(self, warmup_iters: int = 3) -> None:
        """Run (real, counted) frames up to the first learning frame plus ``warmup_iters`` on a
        side stream, then capture the six launches of a learning frame as one hipGraph."""
        if not self.learning:
            raise RuntimeError("capture() records a learning frame")
        warm_up(self.device, self.frame, max(self.first_learning_frame - self.frames, 0) + warmup_iters)
        torch.cuda.synchronize(self.device)
        self._pool = torch.cuda.graph_pool_handle()
        self._graph = capture_graph(self._full_frame, self._pool)
        torch.cuda.synchronize(self.device)

    def run(self, n: int) -> float:
        """``n`` frames; the wall time they took."""
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        for _ in range(int(n)):
            self.frame()
        torch.cuda.synchronize(self.device)
        return time.perf_counter() - t0

    # ------------------------------------------------------------------ host views
    def stats(self) -> dict:
        """Host-side view of the last frame's scalars (forces a sync; call rarely)."""
        n = self.norms.tolist()
        log = self.ep_log.sum(0).tolist()
        return {"frames": self.frames, "learn_steps": self.learn_steps, "loss": float(self.loss.item()),
                "grad_norm_l2": n[0], "lr": n[3], "eps": float(self.eps.item()), "beta": float(self.beta.item()),
                "episodes": int(log[2]), "return_sum": float(log[3]), "max_prio": float(self.replay.max_prio.item())}

    def episode_stats(self) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(last episode return, last episode length, finished episode count) per env."""
        return self.ep_log[:, 0], self.ep_log[:, 1], self.ep_log[:, 2]

    def state_dict(self):
        return self.model.state_dict()

    def save(self, path: str) -> str:
        """Reference-format ``state_dict`` of the online network."""
        return save_state_dict(self.model, path)

    # ---- GreedyRollouts: ``rollout_evaluate()`` is one ``vec_rollout`` launch + one read-back
    _eval_steps = property(lambda self: self.frames)
    _eval_limit = property(lambda self: self.limit)

    def _make_rollout(self, n: int) -> VecRolloutBuffers:
        return VecRolloutBuffers(self.hip, self.net, self.kind, self.obs_dim, n, self.device)

    evaluate = GreedyRollouts.rollout_evaluate
