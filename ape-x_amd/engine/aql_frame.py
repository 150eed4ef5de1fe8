"""GPU engine of the single-process AQL trainer (reference ``AQL.py:17-150``; the host loop is
``trainers/aql.py:train_AQL``): one env, acting with the online net in train mode, one SGD step
per frame, everything on one MI355X with no host sync inside a frame.

Every cadence is ``AQL.py``'s, not ``AQL_dis.py``'s (:mod:`apex_amd.engine.aql`):

* behaviour epsilon drawn per frame: 0.5 when u > 0.1, else 0.05 (``AQL.py:116``);
* acting weights = the online net itself, NoisyNet noise applied;
* one SGD step per frame once ``len(buffer) > batch_size`` after that frame's insert: the first
  learning frame is ``t = batch_size``;
* NoisyNet noise is never reset (the constructor's noise stays; a target sync copies it), and
  the proposal is not copied to the target per step;
* ``CosineAnnealingLR(T_max=max_step, eta_min=lr/1000)`` on both Adams: SGD step k (0-based)
  runs at ``cosine_lr(k)`` (:func:`apex_amd.algo.schedules.cosine_lr`);
* PER beta(t) = min(1, beta0 + t (1 - beta0) / max_step) by frame index;
* full target sync after the frame's SGD step when ``t % target_update_interval == 0``, frame 0
  included; ``model{t}.pth`` when ``t % save_interval == 0`` or on the last frame (the caller's
  loop, ``trainers/aql.py``).

One learning frame is five launches (``fused=True``), frame counter ``t`` on the device:

1. ``aql_frame`` (``ops/csrc/aql_frame_kernels.hip``, one workgroup): proposal, candidate set,
   critic, this frame's epsilon, epsilon-greedy selection, env step, the transition into slot
   ``filled mod C`` at ``max_prio^alpha`` with every level of its path, ``filled += 1``,
   beta(t), ``t += 1``.
2. ``aql_learn_fwd`` (draws its own PER rows)
3. ``aql_learn_bwd`` (+ the priority write's leaves and level 1)
4. ``aql_grad`` (+ the tree's upper levels)
5. ``aql_update`` in ``AQL.py`` mode (``keep_noise``, ``no_proposal_copy``, cosine schedule)

``run(n)`` replays two captured hipGraphs -- launch 1 alone below the first learning frame, all
five from it on -- and issues the target sync eagerly between replays.  ``fused=False`` is the
launch-by-launch yardstick with the same seeds and counters: ``aql_propose`` -> noisy-effective
weights + ``aql_candidate_q`` -> ``aql_frame_eps`` + ``aql_select`` -> ``aql_env_step`` ->
``per_write_leaves`` -> ``per_sample`` -> forward, backward, ``per_write_batch``, ``aql_grad``,
``adam_step2`` (the host's ``cosine_lr(k)`` rounded to fp32) -> ``aql_post(regen=0)`` -> the
counter bump.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass

import numpy as np
import torch

from .. import envs, ops
from ..algo.schedules import cosine_lr
from ..models.aql import AQL
from ..utils.checkpoint import save_model, save_train_state
from .aql import ENV_KINDS, AQLEngine, AQLEngineConfig, AQLLearner, AQLReplay
from .evaluation import GreedyRollouts

MAX_T = 1024           # candidates per state (aql_frame / aql_rollout: one LDS row)
MAX_CAND_FLOATS = 4608  # T * (adim + 1): the candidate set and its Q row in LDS
MAX_BATCH = 64         # the fused step's tree workgroups stage <= 64 dirty paths
# (action dim, number of discrete actions or None) per env kind
_ACTION_SPEC = {0: (4, None), 1: (1, 2), 2: (1, None)}


def frame_seeds(seed: int) -> dict:
    """The 48-bit Philox keys of an engine built with ``cfg.seed = seed``: env dynamics / resets,
    proposal sampling, selection, and the per-frame epsilon draw (``aql_frame_kernels.hip``)."""
    base = (int(seed) * 0x2545F491 + 0xAC7) & 0xFFFFFFFFFFFF
    return {"env": base, "prop": base ^ 0x9909, "sel": base ^ 0xA9C1, "eps": base ^ 0xE951}


@dataclass
class AQLFrameConfig:
    """Defaults: the reference's ``AQL.py`` constructor."""
    env_id: str = "Pendulum-v0"
    n_envs: int = 1
    capacity: int = 100_000
    batch_size: int = 32
    gamma: float = 0.99
    lr: float = 1e-4
    lr_eta_min: float | None = None     # None: lr / 1000 (AQL.py:44-45)
    max_step: int = 1_000_000           # T_max of the cosine schedule and the beta horizon, in frames
    ent_lam: float = 0.8
    propose_sample: int = 100
    uniform_sample: int = 100
    action_var: float = 0.25
    alpha: float = 0.6
    beta_start: float = 0.4
    max_norm: float = 40.0              # clip on each optimizer
    target_update_interval: int = 1000
    save_interval: int = 10_000
    eps_hi: float = 0.5                 # behaviour epsilon: eps_hi when u > eps_p, else eps_lo
    eps_lo: float = 0.05
    eps_p: float = 0.1
    exact_mass: bool = False            # False = the reference's exclusive-end sampling mass
    max_episode_steps: int | None = None   # None: the env's registered TimeLimit
    fused: bool = True                  # False: the launch-by-launch yardstick (module docstring)
    use_graphs: bool = True             # run(): replay captured hipGraphs (fused only)
    track_losses: bool = False          # device-side loss sums per step (three small launches more)
    trace_q: bool = False               # aql_frame also writes the frame's Q row (tests)
    seed: int = 0

    def candidates(self) -> tuple[int, int]:
        """(T, action dim) of the env's candidate sets."""
        adim, n_act = _ACTION_SPEC[ENV_KINDS[self.env_id]]
        uni = self.uniform_sample if n_act is None else min(self.uniform_sample, n_act)
        return int(self.propose_sample + uni), adim

    def eta_min(self) -> float:
        return self.lr / 1000 if self.lr_eta_min is None else float(self.lr_eta_min)

    def validate(self) -> "AQLFrameConfig":
        if self.env_id not in ENV_KINDS:
            raise ValueError(f"GPU AQL env must be one of {sorted(ENV_KINDS)}")
        if self.n_envs != 1:
            raise ValueError("n_envs must be 1 (AQL.py is a single-env trainer)")
        if self.propose_sample < 0 or self.uniform_sample < 0:
            raise ValueError("propose_sample and uniform_sample must be >= 0")
        T, adim = self.candidates()
        if not (1 <= T <= MAX_T and T * (adim + 1) <= MAX_CAND_FLOATS):
            raise ValueError(f"the candidate set must fit LDS: 1 <= T <= {MAX_T} and T * (adim + 1) <= "
                             f"{MAX_CAND_FLOATS} (T = {T}, adim = {adim})")
        if not 1 <= self.batch_size <= MAX_BATCH:
            raise ValueError(f"batch_size must be in [1, {MAX_BATCH}]")
        if self.capacity <= self.batch_size:
            raise ValueError("capacity must exceed batch_size")
        if self.target_update_interval < 1:
            raise ValueError("target_update_interval >= 1")
        if self.max_step < 1:
            raise ValueError("max_step >= 1")
        if self.max_episode_steps is not None and self.max_episode_steps < 1:
            raise ValueError("max_episode_steps >= 1")
        return self

    def first_learning_frame(self) -> int:
        """The first frame index t whose insert leaves ``len(buffer) = t + 1 > batch_size``."""
        return self.batch_size // self.n_envs

    def learner_config(self) -> AQLEngineConfig:
        """The :class:`AQLLearner` view of this config."""
        return AQLEngineConfig(env_id=self.env_id, n_envs=1, capacity=self.capacity, batch_size=self.batch_size,
                               gamma=self.gamma, n_steps=1, lr=self.lr, ent_lam=self.ent_lam,
                               propose_sample=self.propose_sample, uniform_sample=self.uniform_sample,
                               action_var=self.action_var, alpha=self.alpha, beta_start=self.beta_start,
                               max_step=self.max_step, max_norm=self.max_norm, track_losses=self.track_losses,
                               exact_mass=self.exact_mass, fused=self.fused, seed=self.seed)


class AQLFrameEngine(GreedyRollouts):
    """``AQL.py`` on one GPU: ``frame()`` is one loop iteration of the reference trainer."""

    def __init__(self, cfg: AQLFrameConfig, device: str | torch.device = "cuda"):
        self.cfg = cfg.validate()
        self.device = dev = torch.device(device)
        self.hip = h = ops.hip()
        self.kind = ENV_KINDS[cfg.env_id]
        self.host_env = envs.make(cfg.env_id)
        torch.manual_seed(cfg.seed)
        kw = dict(propose_sample=cfg.propose_sample, uniform_sample=cfg.uniform_sample, action_var=cfg.action_var,
                  device=dev)
        self.model = AQL(env=self.host_env, **kw).to(dev)
        self.target = AQL(env=self.host_env, **kw).to(dev)
        self.target.load_state_dict(self.model.state_dict())
        for m in (self.model, self.target):
            m.q.train()
        self.cont = bool(self.model.env_iscontinuous)
        self.T = int(self.model.total_sample)
        self.obs = int(self.host_env.observation_space.shape[0])
        self.adim = int(self.model.num_actions) if self.cont else 1
        assert (self.T, self.adim) == cfg.candidates()
        self.B = int(cfg.batch_size)
        self.replay = r = AQLReplay(cfg.capacity, self.obs, self.T, self.adim, cfg.alpha, dev, seed=cfg.seed + 17)
        self.lr_eta_min = cfg.eta_min()
        self.learner = L = AQLLearner(self.model, self.target, r, cfg.learner_config(), step_opts=dict(
            keep_noise=1, no_proposal_copy=1, cos_T_max=float(cfg.max_step), cos_eta_min=float(self.lr_eta_min),
            cos_lr0=float(cfg.lr)))
        self.fused = bool(cfg.fused)
        assert L.fused == self.fused
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)   # frame counter (the acting Philox counter)
        self.obs_buf = torch.zeros(1, self.obs, **f32)
        self.phys = torch.zeros(1, 4, **f32)
        self.ep_len = torch.zeros(1, **i32)
        self.ep_ret = torch.zeros(1, **f32)
        self.ep_count = torch.zeros(1, **i32)
        self.log_cap = 4096
        self.ep_log = torch.zeros(self.log_cap, 2, **f32)
        self.act_idx = torch.zeros(1, **i32)
        self.env_act = torch.zeros(1, self.adim, **f32)
        self.eps = torch.zeros(1, **f32)
        self.reward = torch.zeros(1, **f32)
        self.done = torch.zeros(1, **f32)
        self.slot = torch.zeros(1, **i32)
        self.qbuf = torch.zeros(1, self.T, **f32)       # the frame's Q row (yardstick; fused: cfg.trace_q)
        self.amu = torch.zeros(1, self.T, self.adim, **f32)   # the yardstick's candidate set
        self.ws = torch.zeros(h.aql_workspace_floats(), **f32)
        self.beta = L.beta
        self.lr_used = L.norms_q[3:4]                   # the lr of the last SGD step (both Adams)
        if self.cont:
            sp = self.host_env.action_space
            self.low = torch.as_tensor(np.asarray(sp.low, dtype=np.float32).reshape(-1), **f32)
            self.high = torch.as_tensor(np.asarray(sp.high, dtype=np.float32).reshape(-1), **f32)
        else:
            self.low = self.high = torch.zeros(1, **f32)
        self.var = self.model.proposal.action_var.to(**f32).contiguous()
        if self.kind == 0:
            self.dynA = torch.as_tensor(self.host_env.unwrapped._A, **f32).contiguous()
            self.dynB = torch.as_tensor(self.host_env.unwrapped._B, **f32).contiguous()
            self.dynw = torch.as_tensor(self.host_env.unwrapped._w, **f32).contiguous()
        else:
            self.dynA = self.dynB = self.dynw = torch.zeros(1, **f32)
        self.seeds = frame_seeds(cfg.seed)
        limit = int(getattr(self.host_env, "_max_episode_steps", None) or 1_000_000)
        self.limit = int(limit if cfg.max_episode_steps is None else cfg.max_episode_steps)
        self.env = h.make_aql_env(dict(
            kind=self.kind, E=1, obs=self.obs, adim=self.adim, T=self.T, max_steps=self.limit,
            obs_buf=self.obs_buf.data_ptr(), phys=self.phys.data_ptr(), ep_len=self.ep_len.data_ptr(),
            ep_ret=self.ep_ret.data_ptr(), dynA=self.dynA.data_ptr(), dynB=self.dynB.data_ptr(),
            dynw=self.dynw.data_ptr(), seed=self.seeds["env"], counter=self.t.data_ptr(),
            ep_count=self.ep_count.data_ptr(), ep_log=self.ep_log.data_ptr(), log_cap=self.log_cap))
        self.ins = h.make_aql_insert(dict(r.table_ptrs(), C=r.capacity, filled=r.filled.data_ptr(),
                                          slots=self.slot.data_ptr()))
        self.net = L.fused_on._net(noisy=True)        # acting: the online net in train mode
        self.eval_net = L.fused_on._net(noisy=False)  # evaluation: the NoisyNet means
        self.F = h.make_aql_frame(self.net, self.env, self.ins, r.tree, dict(
            prop_seed=self.seeds["prop"], sel_seed=self.seeds["sel"], eps_seed=self.seeds["eps"],
            low=self.low.data_ptr(), high=self.high.data_ptr(), var=self.var.data_ptr(), t=self.t.data_ptr(),
            filled=r.filled.data_ptr(), max_prio=r.max_prio.data_ptr(), alpha=float(r.alpha),
            eps_hi=float(cfg.eps_hi), eps_lo=float(cfg.eps_lo), eps_p=float(cfg.eps_p),
            beta0=float(cfg.beta_start), beta_max_step=float(cfg.max_step), beta_out=self.beta.data_ptr(),
            act_idx=self.act_idx.data_ptr(), env_act=self.env_act.data_ptr(), eps_out=self.eps.data_ptr(),
            reward=self.reward.data_ptr(), done=self.done.data_ptr(),
            q_out=self.qbuf.data_ptr() if cfg.trace_q else 0))
        self.first_learning_frame = cfg.first_learning_frame()
        self.learning = True    # False: frames run the acting launch only (the insert path on its own)
        self.frames = 0         # host mirror of ``t``
        self.learn_steps = 0    # host mirror of the learner's step counter
        self.target_syncs: list[int] = []   # frames after which the target was synced (the last 4096)
        self._g_act = self._g_full = None
        self._ep_read = 0
        self.eval_limit = int(getattr(self.host_env, "_max_episode_steps", None) or 10_000)
        self._eval = None
        h.aql_env_reset(self.env, self._s())

    @staticmethod
    def _s() -> int:
        return torch.cuda.current_stream().cuda_stream

    # ------------------------------------------------------------------ the frame
    def act_insert(self) -> None:
        """The acting side of the frame: one launch (fused) or the yardstick's sequence."""
        h, s, r = self.hip, self._s(), self.replay
        if self.fused:
            h.aql_frame(self.F, s)
            return
        c = self.cfg
        self.beta.fill_(min(1.0, c.beta_start + self.frames * (1.0 - c.beta_start) / c.max_step))
        h.aql_propose(self.net, self.obs_buf.data_ptr(), 1, self.low.data_ptr(), self.high.data_ptr(),
                      self.var.data_ptr(), self.seeds["prop"], self.t.data_ptr(), self.amu.data_ptr(), 0, s)
        h.aql_candidate_q(self.net, self.ws.data_ptr(), self.obs_buf.data_ptr(), self.amu.data_ptr(), 1,
                          self.qbuf.data_ptr(), s)
        h.aql_frame_eps(self.seeds["eps"], self.t.data_ptr(), float(c.eps_hi), float(c.eps_lo), float(c.eps_p),
                        self.eps.data_ptr(), s)
        h.aql_select(self.qbuf.data_ptr(), self.amu.data_ptr(), 1, self.T, self.adim, self.eps.data_ptr(),
                     self.seeds["sel"], self.t.data_ptr(), self.act_idx.data_ptr(), self.env_act.data_ptr(), s)
        h.aql_env_step(self.env, self.env_act.data_ptr(), self.act_idx.data_ptr(), self.amu.data_ptr(), self.ins, s)
        sl = self.slot.long()
        self.reward.copy_(r.reward.index_select(0, sl))
        self.done.copy_(r.done.index_select(0, sl))
        h.per_write_leaves(r.tree, self.slot.data_ptr(), 0, 1, r.alpha, r.max_prio.data_ptr(), 0,
                           r.sorted_scratch.data_ptr(), r.filled.data_ptr(), 1, self.t.data_ptr(), 1, s)

    def set_learn_steps(self, k: int) -> None:
        """Set the SGD step counter (Adam's t, the cosine schedule's k, the PER draw's counter) on
        the device and its host mirror."""
        self.learn_steps = int(k)
        self.learner.step_ctr.fill_(int(k))

    def sgd_step(self) -> None:
        """One SGD step in ``AQL.py`` mode: four launches (fused) or the yardstick's sequence."""
        L = self.learner
        if self.fused:
            L.step()
            return
        h, r, s, c = self.hip, self.replay, self._s(), self.cfg
        h.per_sample(r.tree, self.B, r.filled.data_ptr(), 0, L.beta.data_ptr(), 0.0, r.seed ^ 0x51A7,
                     L.step_ctr.data_ptr(), L.idx.data_ptr(), L.w.data_ptr(), 0 if c.exact_mass else 1, s)
        h.aql_learn_fwd(L.L, s)
        h.aql_learn_bwd(L.L, s)
        h.per_write_batch(r.tree, 0, 0, 0, 0, L.idx.data_ptr(), 0, self.B, L.delta.data_ptr(), L.lw.data_ptr(),
                          L.prio.data_ptr(), L.loss_q.data_ptr(), 0, r.owner.data_ptr(), r.wlist.data_ptr(),
                          r.max_prio.data_ptr(), r.alpha, r.ticket.data_ptr(), s)
        h.aql_grad(L.G, s)
        hp = h.AdamParams(float(cosine_lr(self.learn_steps, c.lr, c.max_step, self.lr_eta_min)),
                          max_norm=c.max_norm)
        Pq, o = L.P_q, 4 * L.P_q
        h.adam_step2((L.flat.data_ptr(), L.grad.data_ptr(), L.m.data_ptr(), L.v.data_ptr(), Pq,
                      L.part.data_ptr(), L.nblk, L.norms_q.data_ptr()),
                     (L.flat.data_ptr() + o, L.grad.data_ptr() + o, L.m.data_ptr() + o, L.v.data_ptr() + o, L.P_p,
                      L.part.data_ptr() + 8 * L.nblk, L.nblk, L.norms_p.data_ptr()),
                     hp, L.step_ctr.data_ptr(), s)
        h.aql_post(L.post, 0, s)   # effective weights from the updated parameters, the noise stays
        L.step_ctr.add_(1)
        L._track_losses()

    def _full_frame(self) -> None:
        self.act_insert()
        self.sgd_step()

    def sync_target(self) -> None:
        """update_target: full state_dict copy, noise buffers included."""
        self.learner.sync_target()

    def _learns(self, t: int) -> bool:
        return self.learning and t >= self.first_learning_frame

    def _after(self, t: int, learned: bool) -> None:
        if learned:
            self.learn_steps += 1
        if t % self.cfg.target_update_interval == 0:
            self.sync_target()
            self.target_syncs.append(t)
            del self.target_syncs[:-4096]
        self.frames = t + 1

    def frame(self) -> None:
        """One iteration of ``AQL.py``'s loop at frame index ``self.frames``, launch by launch."""
        t = self.frames
        learned = self._learns(t)
        if learned:
            self._full_frame()
        else:
            self.act_insert()
        self._after(t, learned)

    def _capture(self, fn):
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        torch.cuda.synchronize(self.device)
        return g

    def run(self, n: int) -> float:
        """``n`` frames with no host sync between them; the wall time they took.  Fused with
        ``use_graphs``: the acting launch and the five launches of a learning frame are each
        captured as a hipGraph after their first eager run and replayed from then on; the target
        sync is issued eagerly between replays on the frames that are due."""
        graphs = self.fused and self.cfg.use_graphs
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        for _ in range(int(n)):
            t = self.frames
            learned = self._learns(t)
            g = self._g_full if learned else self._g_act
            if g is not None:
                g.replay()
            elif learned:
                self._full_frame()
                if graphs:
                    self._g_full = self._capture(self._full_frame)
            else:
                self.act_insert()
                if graphs:
                    self._g_act = self._capture(self.act_insert)
            self._after(t, learned)
        torch.cuda.synchronize(self.device)
        return time.perf_counter() - t0

    @property
    def launches_per_frame(self) -> int:
        """Kernel launches of one fused learning frame (without the optional loss tracking)."""
        return 5

    # ------------------------------------------------------------------ host views
    def __len__(self) -> int:
        return len(self.replay)

    def finished_episodes(self) -> list[tuple[float, int]]:
        """(return, length) of the episodes finished since the last call (host sync)."""
        n = int(self.ep_count.item())
        lo = max(self._ep_read, n - self.log_cap)
        out = []
        if n > lo:
            log = self.ep_log.cpu()
            out = [(float(log[k % self.log_cap, 0]), int(log[k % self.log_cap, 1])) for k in range(lo, n)]
        self._ep_read = n
        return out

    def stats(self) -> dict:
        """Host-side view of the last frame's scalars (forces a sync; call rarely)."""
        L = self.learner
        return {"frames": self.frames, "learn_steps": int(L.step_ctr.item()), "loss_q": float(L.loss_q.item()),
                "loss_proposal": float(L.loss_p.item()), "beta": float(self.beta.item()),
                "lr": float(self.lr_used.item()), "eps": float(self.eps.item()),
                "max_prio": float(self.replay.max_prio.item())}

    def state_dict(self):
        return self.model.state_dict()

    def save(self, t: int, save_dir: str = ".") -> str:
        """``model{t}.pth``: the reference ``state_dict`` of the online net (``q.*`` / ``proposal.*``
        keys, NoisyNet epsilon buffers included) + the ``.train.pt`` sidecar (Adam moments, step
        counter, target net, counters), as ``train_aql.py`` writes them."""
        path = os.path.join(save_dir, f"model{int(t)}.pth")
        torch.cuda.synchronize(self.device)
        L = self.learner
        save_train_state(path, target=self.target, counters={"frame": int(t), "learner_steps": self.learn_steps},
                         extra_tensors={"adam_m": L.m, "adam_v": L.v, "step_ctr": L.step_ctr})
        return save_model(self.model, path)

    # ------------------------------------------------------------------ evaluation
    # the stepwise greedy evaluator of the GPU AQL engine (eval-mode online net, an evaluation
    # shard of its own) and its rollout buffers on the online net's eval handle: they only touch
    # the attributes this engine shares with AQLEngine
    evaluate = AQLEngine.evaluate
    _eval_steps = property(lambda self: self.learn_steps)
    _eval_limit = AQLEngine._eval_limit
    _make_rollout = AQLEngine._make_rollout


def host_epsilons(seed: int, n: int, eps_hi: float = 0.5, eps_lo: float = 0.05, eps_p: float = 0.1,
                  uniform4=None) -> list[float]:
    """Host model of the engine's epsilon stream for ``cfg.seed = seed``, frames 0..n-1
    (``aql_frame_kernels.hip``): u = uniform4(eps key, stream 0, counter t)[0], epsilon = eps_hi
    when u > eps_p (compared in fp32), else eps_lo.  ``uniform4(seed, stream, counter)``: a
    Philox4x32-10 model returning the four fp32 uniforms (top 24 bits of each word x 2^-24)."""
    key = frame_seeds(seed)["eps"]
    p32 = np.float32(eps_p)
    return [float(np.float32(eps_hi if np.float32(uniform4(key, 0, t)[0]) > p32 else eps_lo)) for t in range(n)]
