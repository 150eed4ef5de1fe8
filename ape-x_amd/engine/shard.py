"""What every DQN actor shard shares: the n-step batcher's state, the epsilon ladder, the
per-step buffers and the action draw -- and the acting copy of the learner's network.

:class:`NStepShard` is the base of ``ActorShard`` (GPU sprite game), ``HostEnvShard`` (host
emulators) and ``VectorActorShard`` (classic control).  A subclass adds its front end: env
state, reset / step / ingest, staging sets, ``observe()`` and its own tree write after
:meth:`NStepShard._emit`.  The ``st`` layout is a contract with ``nstep_emit``
(ops/csrc/hip_bindings.cpp ``make_nstep``); :func:`nstep_state` is the one place it is written.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..algo.schedules import actor_epsilon
from ..models.fused import make_hip_net, make_workspace
from .learner import forward_q

ACT_SEED_XOR = 0x5E1EC7   # action-draw key = shard seed ^ this (the env's own draws use the seed)


def nstep_state(E: int, A: int, n: int, device) -> dict[str, torch.Tensor]:
    """The n-step batcher's per-env state: the open window (``win_*``), the rows being drained
    at an episode end (``drain_*``) and the frame-id stack ``hist``."""
    i32 = dict(dtype=torch.int32, device=device)
    f32 = dict(dtype=torch.float32, device=device)
    return {
        "win_ids": torch.zeros(E, n, 4, **i32), "win_a": torch.zeros(E, n, **i32),
        "win_r": torch.zeros(E, n, **f32), "win_q": torch.zeros(E, n, A, **f32),
        "win_meta": torch.zeros(E, 4, **i32), "hist": torch.zeros(E, 4, **i32),
        "drain_ids": torch.zeros(E, n, 4, **i32), "drain_a": torch.zeros(E, n, **i32),
        "drain_r": torch.zeros(E, n, **f32), "drain_q": torch.zeros(E, n, **f32),
        "drain_meta": torch.zeros(E, 2, **i32), "drain_s2": torch.zeros(E, 4, **i32),
    }


class NStepShard:
    """E envs' acting state over an ``HBMReplay``: epsilon ladder (actor ids are global:
    ``actor_offset`` + local index), per-step buffers and the n-step batcher handle."""

    def __init__(self, replay, n_envs: int, n_actions: int, n_step: int, gamma: float, eps_base: float,
                 eps_alpha: float, actor_offset: int, total_actors: int | None, seed: int, mode: str):
        self.hip = ops.hip()
        self.replay = replay
        self.E, self.A, self.n = int(n_envs), int(n_actions), int(n_step)
        if replay.n_envs != self.E:
            raise ValueError("replay slot layout is sized for this shard's env count")
        if mode not in ("reference", "textbook"):
            raise ValueError("mode must be 'reference' or 'textbook'")
        self.device = dev = replay.device
        self.seed = int(seed)
        E, A, n = self.E, self.A, self.n
        total = total_actors if total_actors is not None else E
        ids = np.arange(actor_offset, actor_offset + E, dtype=np.float64)
        self.eps = torch.as_tensor(np.atleast_1d(actor_epsilon(ids, total, eps_base, eps_alpha)), dtype=torch.float32,
                                   device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.new_frame = torch.zeros(E, **i32)
        self.ep_log = torch.zeros(E, 4, **f32)
        self.q = torch.zeros(E, A, **f32)
        self.actions = torch.zeros(E, **i32)
        self.reward = torch.zeros(E, **f32)
        self.done = torch.zeros(E, **f32)
        self.slot = torch.zeros(E, **i32)
        self.prio = torch.zeros(E, **f32)
        self.step_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.st = nstep_state(E, A, n, dev)
        self.nstep = self.make_nstep(gamma, mode, replay.trans_ptrs())

    def make_nstep(self, gamma: float, mode: str, rows: dict, **kw):
        """``nstep_emit`` handle over this shard's ``st`` that writes its rows into ``rows``."""
        return self.hip.make_nstep(self.E, self.A, self.n, self.replay.capacity, float(gamma),
                                   0 if mode == "reference" else 1, {k: v.data_ptr() for k, v in self.st.items()},
                                   rows, **kw)

    @staticmethod
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream

    @property
    def act_seed(self) -> int:
        return self.seed ^ ACT_SEED_XOR

    def act_args(self) -> tuple:
        """(eps, rng seed, step counter, actions) pointers for an inference kernel that
        picks the actions itself (``heads_fwd_multi``'s eps-greedy epilogue: the same
        draw as ``select_actions``)."""
        return (self.eps.data_ptr(), self.act_seed, self.step_counter.data_ptr(), self.actions.data_ptr())

    def select(self, q: torch.Tensor | None = None) -> None:
        """eps-greedy on ``self.q`` (or ``q``) with the standalone kernel: the same draw as the
        heads epilogue (for a policy that does not pick the actions itself)."""
        if q is not None and q.data_ptr() != self.q.data_ptr():
            self.q.copy_(q)
        self.hip.select_actions(self.q.data_ptr(), self.E, self.A, *self.act_args(), self._stream())

    def _emit(self, handle, slot: torch.Tensor, prio: torch.Tensor, bump: bool) -> None:
        """``nstep_emit`` of this step (``q``, ``actions``, ``reward``, ``done``, ``new_frame``)
        through ``handle``: emitted slots and actor priorities into ``slot`` / ``prio``.
        ``bump``: the kernel advances ``step_counter`` (else the tree write that follows does)."""
        self.hip.nstep_emit(handle, self.q.data_ptr(), self.actions.data_ptr(), self.reward.data_ptr(),
                            self.done.data_ptr(), self.new_frame.data_ptr(), self.step_counter.data_ptr(),
                            slot.data_ptr(), prio.data_ptr(), self._stream(), bump)

    def state_tensors(self) -> dict[str, torch.Tensor]:
        """The shard's persistent device state (full-state checkpoints): the n-step batcher's
        ``st`` and the per-step buffers a later step or the host reads.  A subclass adds its
        front end's."""
        out = {f"st.{k}": v for k, v in self.st.items()}
        for k in ("eps", "new_frame", "ep_log", "q", "actions", "reward", "done", "slot", "prio", "step_counter"):
            out[k] = getattr(self, k)
        return out

    def host_state(self) -> dict:
        """Host scalars of the shard: the key of its counter-based draws."""
        return {"seed": self.seed}

    def load_host_state(self, st: dict) -> None:
        self.seed = int(st["seed"])

    def frames_written(self) -> int:
        """Frame-ring positions written so far: a reset writes ``step * E + e``, a step
        ``(step + 1) * E + e`` (reads ``step_counter``: a host sync)."""
        return (int(self.step_counter.item()) + 1) * self.E

    def episode_stats(self) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(last episode return, last episode length, finished episode count) per env."""
        return self.ep_log[:, 0], self.ep_log[:, 1], self.ep_log[:, 2]


class ActorPolicy:
    """The acting copy of a learner's network: ``model`` (the caller's own: a deepcopy of the
    learner's, or an actor rank's) re-flattened and frozen, and for ``forward == "hip"`` the HIP
    net + workspace whose heads kernel writes Q into ``q`` in place (no copy)."""

    def __init__(self, model, E: int, A: int, device, forward: str, dtype: str, q: torch.Tensor):
        self.model = model
        model._flat = None
        self.flat = model.flatten_parameters()
        for p in model.parameters():
            p.requires_grad_(False)
            p.grad = None
        self.hip_net = forward == "hip"
        self.bf16 = dtype == "bf16"
        self.net = self.ws = None
        if self.hip_net:
            # actors act at the learner's precision (the reference's actors are fp32 too)
            self.net = make_hip_net(model, dtype)
            self.ws = make_workspace(E, A, device, dtype)
            self.ws.q = q

    def state_tensors(self) -> dict[str, torch.Tensor]:
        return {"flat": self.flat}

    def refresh_packed(self) -> None:
        """Re-derive the HIP net's packed copies after ``flat`` was written from outside."""
        if self.hip_net:
            self.net.repack()

    def publish_from(self, learner) -> None:
        """Learner -> acting weights (flat parameters, and the HIP net's packed copies)."""
        learner.copy_params_to(self.flat)
        if self.hip_net:
            self.net.copy_packed_from(learner.net)

    def forward(self, replay, shard: NStepShard) -> torch.Tensor | None:
        """HIP: conv1 reads the current stacks straight from the frame ring, the heads kernel
        writes Q into the shard's buffer and picks the eps-greedy actions (returns None).
        Otherwise Q of ``shard.observe()``, for the caller to select from."""
        if self.hip_net:
            self.net(replay.frames, self.ws, shard.st["hist"], act=shard.act_args())
            return None
        with torch.no_grad():
            return forward_q(self.model, shard.observe(), self.bf16)
