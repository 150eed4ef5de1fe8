"""Greedy evaluation on HOST envs beside the host-env vector Ape-X engine (reference:
origin_repo/eval.py -- epsilon 0, a process of its own that never holds up the learner).

:class:`VectorHostEvaluator` is the evaluator over any object of the
:class:`~apex_amd.envs.host_vector.HostVectorEnv` protocol: ``N <= 64`` extra envs, its own device
copy of their staging block (the host block is registered with HIP and read in place, as
:class:`~apex_amd.engine.vector_host.VectorHostShard` does), ``q`` / ``actions`` buffers, a pinned
action buffer, a side stream with an ``acted`` event, and TWO weight sets -- each a ``DuelingDQN``
(MLP form) over flat parameters with its ``VecNet`` handle.  Step ``k`` is

    H2D of the staging block (after ``reset`` for k = 0) -> act on its ``reset_obs`` rows ->
    actions D2H -> host step

where the act is, by ``kernel``:

``"step"``   the yardstick built from existing kernels only, over a private ring of ``4 N`` rows
             with its own ``hist`` / ``new_frame`` / ``reward`` / ``done`` / episode rows, zero
             ``eps`` and an int64 counter starting at 0: ``vec_host_tail`` (the reset form at
             k = 0) -> ``frame_hist_step`` (k > 0; it bumps the counter to k) -> ``vec_act``;
             3 launches per act.
``"fused"``  ``vec_host_eval_act`` (ops/csrc/vector_kernels.hip): one launch, ``vec_act``'s
             geometry, the observations straight from the staged ``reset_obs`` rows, the step
             ``k`` by value.  Bit-equal to the step form on ``q`` and ``actions``.

Draw seed: ``(eval_seed(seed) & (2^48 - 1)) ^ ACT_XOR``.  Evaluator env ``j`` is seeded
``eval_seed(seed) + j``: the caller builds the vector env with ``seed=eval_seed(seed)``
(:func:`make_pool` does).

Episodes are accounted on the host in float64 from the block's raw ``reward`` and its ``ended``
flags: no device read.  ``capped`` is the vector env's own notion: ended with ``done = 0`` (a
``max_episode_length`` reset).  Each finished episode is handed over once as ``(return, length,
capped, learn_step_at_end)``.

Weights (:class:`~apex_amd.engine.host_eval.WeightSets`): ``refresh()`` copies the online flat
parameters (``engine.learner.copy_params_to``) on the CURRENT (training) stream into the set no
act can be reading and records an event; later acts wait for it on the side stream and read that
set.  ``refresh`` returns ``False`` and does nothing while the act that last used the target set
has not completed.  The training stream never waits on the side stream.

:class:`VectorHostEvaluation` drives the evaluator over a
:class:`~apex_amd.envs.proc_host_vector.ProcHostVectorEnv` without ever blocking: the pump of
:class:`~apex_amd.engine.aql_host_eval.AQLHostEvaluation` (``pump()`` once per training iteration
performs at most one half-step).  Its launches are eager and sit between graph replays, so the
captured learner graph gains no node.  :meth:`VectorHostEvaluator.run` is the blocking,
deterministic form (in-process envs).
"""
from __future__ import annotations

import weakref

import numpy as np

from ..envs.host_vector import staging_views
from .aql_host_eval import MAX_ENVS, AQLHostEvaluation, _Ledger, make_pool
from .host_eval import KERNELS, WeightSets, _unregister, eval_seed

__all__ = ["MAX_ENVS", "VectorHostEvaluation", "VectorHostEvaluator", "make_pool"]

ACT_XOR = 0x5EC7   # the evaluator's action-draw seed = (eval_seed(seed) & (2^48 - 1)) ^ ACT_XOR


class VectorHostEvaluator:
    """``len(vec)`` (at most 64) greedy evaluator envs of a
    :class:`~apex_amd.engine.vector_host.VectorHostEngine`: the device state, both act forms, the
    weight sets and the blocking ``run``; see the module docstring."""

    def __init__(self, engine, vec, kernel: str = "fused", seed: int = 0):
        import torch

        from ..models.dqn import DuelingDQN
        from .vector import vec_net

        if kernel not in KERNELS:
            raise ValueError(f"kernel must be one of {KERNELS}, got {kernel!r}")
        N = len(vec)
        if not 1 <= N <= MAX_ENVS:
            raise ValueError(f"the vector host evaluator runs 1..{MAX_ENVS} envs, got {N}")
        if getattr(vec, "continuous", False):
            raise ValueError("the vector host evaluator takes a discrete action space; a continuous (Box) one is "
                             "AQL's (engine/aql_host_eval.py)")
        if int(vec.obs_dim) != engine.obs_dim or int(vec.n_actions) != engine.A:
            raise ValueError("the evaluator envs' obs_dim / n_actions differ from the model's")
        self.torch, self.hip = torch, engine.hip
        self.engine, self.vec, self.kernel = engine, vec, kernel
        self.device = dev = engine.device
        self.N, self.obs, self.A = N, engine.obs_dim, engine.A
        self.seed = int(seed)
        self.sd = eval_seed(self.seed) & 0xFFFFFFFFFFFF
        self.act_seed = self.sd ^ ACT_XOR
        # the staging block, registered with HIP and read in place, and its device copy
        st = vec.staging
        n = N * (2 * self.obs + 3)
        if not isinstance(st, np.ndarray) or st.dtype != np.float32 or st.shape != (n,) or not st.flags.c_contiguous:
            raise ValueError(f"staging must be a contiguous float32 array of {n} elements")
        self._stage_np = st
        self._views = staging_views(st, N, self.obs)
        self._stage_ptr, self._stage_bytes = int(st.ctypes.data), int(st.nbytes)
        self.hip.host_register(self._stage_ptr, self._stage_bytes)
        self._registered = weakref.finalize(self, _unregister, self.hip, self._stage_ptr, st)
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.stage_dev = torch.zeros(n, **f32)
        self.q = torch.zeros(N, self.A, **f32)
        self.actions = torch.zeros(N, **i32)
        self.act_host = torch.zeros(N, dtype=torch.int32).pin_memory()
        self.actions_np = self.act_host.numpy()
        # two weight sets: a DuelingDQN over flat parameters + its VecNet handle each
        L = engine.learner
        self.models, self.flats, self.nets = [], [], []
        for _ in range(2):
            m = DuelingDQN.from_shapes((self.obs,), self.A).to(dev)
            for p in m.parameters():
                p.requires_grad_(False)
            flat = m.flatten_parameters()
            if flat.numel() != L.P:
                raise ValueError("the evaluator's flat parameters differ in size from the learner's")
            L.copy_params_to(flat)
            self.models.append(m)
            self.flats.append(flat)
            self.nets.append(vec_net(self.hip, m))
        if kernel == "step":
            self._make_step_state()
        self._bind()
        self.stream = torch.cuda.Stream(device=dev)
        self.weights = WeightSets(torch.cuda.Event)
        self.acted = torch.cuda.Event()
        self.ledger = _Ledger(N)
        self.stream.wait_stream(torch.cuda.current_stream())   # (the buffers and weights above are set up)
        self.k = 0            # evaluator steps whose act has been enqueued
        self.learn_step = 0   # stamped on the episodes that end (the caller keeps it current)

    def _make_step_state(self) -> None:
        """The yardstick's private actor-shard state: a ring of 4 N observation rows and what
        ``vec_host_tail`` / ``frame_hist_step`` / ``vec_act`` keep beside it."""
        torch, N, dev = self.torch, self.N, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.F = 4 * N
        self.ring = torch.zeros(self.F, self.obs, **f32)
        self.hist = torch.zeros(N, 4, **i32)
        self.new_frame = torch.zeros(N, **i32)
        self.reward = torch.zeros(N, **f32)
        self.done = torch.zeros(N, **f32)
        self.ep_log = torch.zeros(N, 4, **f32)
        self.ep_ret = torch.zeros(N, **f32)
        self.ep_len = torch.zeros(N, **f32)
        self.eps = torch.zeros(N, **f32)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)

    def _bind(self) -> None:
        """The launch descriptors over the buffers as they are now (``q`` and ``actions`` are read
        here: a test re-seats them inside guarded buffers and binds again)."""
        h, N = self.hip, self.N
        self._acts = self._tail = self._step_acts = None
        if self.kernel == "fused":
            d = dict(N=N, seed=self.act_seed, stage=self.stage_dev.data_ptr(), q=self.q.data_ptr(),
                     actions=self.actions.data_ptr())
            self._acts = [h.make_vec_host_eval_act(net, d) for net in self.nets]
            return
        self._tail = h.make_vec_host_tail(dict(
            E=N, obs=self.obs, F=self.F, stage=self.stage_dev.data_ptr(), ring=self.ring.data_ptr(),
            step=self.counter.data_ptr(), reward=self.reward.data_ptr(), done=self.done.data_ptr(),
            new_frame=self.new_frame.data_ptr(), hist=self.hist.data_ptr(), ep_log=self.ep_log.data_ptr(),
            ep_ret=self.ep_ret.data_ptr(), ep_len=self.ep_len.data_ptr()))
        self._step_acts = [h.make_vec_act(net, self.ring.data_ptr(), self.hist.data_ptr(), N, self.eps.data_ptr(),
                                          self.act_seed, self.counter.data_ptr(), self.q.data_ptr(),
                                          self.actions.data_ptr()) for net in self.nets]

    # ------------------------------------------------------------------ weights
    def refresh(self) -> bool:
        """Take the online parameters as they are at this point of the current (training) stream.
        ``False`` and nothing done while the target set is still read."""
        return self.weights.refresh(lambda i: self.engine.learner.copy_params_to(self.flats[i]))

    # ------------------------------------------------------------------ device half (current stream)
    def ship(self) -> None:
        """H2D of the staging block on the current stream."""
        self.hip.memcpy_h2d_async(self.stage_dev.data_ptr(), self._stage_ptr, self._stage_bytes,
                                  self.torch.cuda.current_stream().cuda_stream)

    def act(self) -> None:
        """Step ``self.k``'s act + the actions' copy-out on the current stream; records ``acted``."""
        h, st = self.hip, self.torch.cuda.current_stream()
        s = st.cuda_stream
        i = self.weights.acquire(st)
        if self.kernel == "fused":
            h.vec_host_eval_act(self._acts[i], self.k, s)
        else:
            h.vec_host_tail(self._tail, self.k == 0, s)
            if self.k > 0:
                h.frame_hist_step(self.hist.data_ptr(), self.new_frame.data_ptr(), self.done.data_ptr(), self.N,
                                  self.counter.data_ptr(), s)
            h.vec_act(self._step_acts[i], s)
        self.weights.release()
        self.act_host.copy_(self.actions, non_blocking=True)
        self.acted.record()
        self.k += 1

    def took(self) -> None:
        """The host step has landed in the block: its raw reward / done / ended into the ledger."""
        v = self._views
        self.ledger.observe_block(v["reward"], v["done"], v["ended"], self.learn_step)

    # ------------------------------------------------------------------ blocking form
    def run(self, n_steps: int) -> None:
        """``n_steps`` whole evaluator steps on the side stream, the host waiting for each step's
        actions (on their event only).  Deterministic: the yardstick, and the form for in-process
        envs."""
        for _ in range(int(n_steps)):
            self.step_begin()
            self.step_end()

    def step_begin(self) -> None:
        """The device half of one blocking step, enqueued on the side stream."""
        with self.torch.cuda.stream(self.stream):
            if self.k == 0:
                self.vec.reset()
            self.ship()
            self.act()

    def step_end(self) -> None:
        """Wait for the step's actions (their event only) and step the envs."""
        self.acted.synchronize()
        self.vec.step(self.actions_np)
        self.took()

    def poll(self) -> list:
        """Finished episodes ``(return, length, capped, learn_step_at_end)``, each exactly once."""
        return self.ledger.poll()

    def close(self) -> None:
        """Wait for the side stream, let go of the registered staging block.  Idempotent."""
        if self._registered.alive:
            self.stream.synchronize()
            self._registered()
        self._stage_np = self._views = None


class VectorHostEvaluation(AQLHostEvaluation):
    """The non-blocking driver of a :class:`VectorHostEvaluator` over a worker pool: the pump of
    :class:`~apex_amd.engine.aql_host_eval.AQLHostEvaluation` as it is (nothing in it is
    AQL-specific); only ``refresh`` differs, the evaluator knowing its own source."""

    def refresh(self) -> bool:
        return self.ev.refresh()
