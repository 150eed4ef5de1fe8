"""Greedy evaluation on HOST envs beside the host-env AQL engine (reference: AQL_dis.py:151-167
-- ``q.eval()``, eps 0, env action ``a_mu[0][a]`` -- in a process of its own).

:class:`AQLHostEvaluator` is the evaluator over any object of the
:class:`~apex_amd.envs.host_vector.HostVectorEnv` protocol: ``N <= 64`` extra envs, its own device
copy of their staging block (the host block is registered with HIP and read in place, as
:class:`~apex_amd.engine.aql_host.AQLHostEngine` does), ``env_act`` / ``act_idx`` / counter
buffers, a pinned action buffer, a side stream with an ``acted`` event, and TWO weight sets -- each
an ``AQL`` module over flat parameters with an eval-mode handle (``FusedAQL(...)._net(noisy=False)``:
the NoisyNet means).  Step ``k`` is

    H2D of the staging block (after ``reset`` for k = 0) -> act on its ``reset_obs`` rows ->
    actions D2H -> host step

where the act is, by ``kernel``:

``"step"``   the yardstick built from existing kernels only: ``aql_propose`` ->
             ``aql_candidate_q`` -> ``aql_select`` (eps 0) and the counter add -- the three launches
             of ``AQLEngine.evaluate`` -- over the same buffers and seeds; 4 enqueues per act.
``"fused"``  ``aql_host_eval_act`` (ops/csrc/aql_host_eval_kernels.hip): one launch, one workgroup
             per env, the step ``k`` by value.  Bit-equal to the step form.

Device seeds: ``sd = eval_seed(seed) & (2^48 - 1)``, the proposal's ``sd ^ 0x9909`` and the
selection's ``sd ^ 0xA9C1`` (``AQLEngine.evaluate``'s derivation).  Evaluator env ``j`` is seeded
``eval_seed(seed) + j``: the caller builds the vector env with ``seed=eval_seed(seed)``
(:func:`make_pool` does).

Episodes are accounted on the host in float64 from the block's raw ``reward`` and its ``ended``
flags (:class:`~apex_amd.engine.host_eval.EpisodeLedger`): no device read.  ``capped`` is the
vector env's own notion: ended with ``done = 0`` (a ``max_episode_length`` reset).  Each finished
episode is handed over once as ``(return, length, capped, learn_step_at_end)``.

Weights (:class:`~apex_amd.engine.host_eval.WeightSets`): ``refresh(src_flat)`` copies the online
flat parameters (``engine.learner.flat``; evaluation reads the means, so no noise buffers) with
``copy_f32`` on the CURRENT (training) stream into the set no act can be reading and records an
event; later acts wait for it on the side stream and read that set.  ``refresh`` returns ``False``
and does nothing while the act that last used the target set has not completed.  The training
stream never waits on the side stream.

:class:`AQLHostEvaluation` drives the evaluator over a
:class:`~apex_amd.envs.proc_host_vector.ProcHostVectorEnv` without ever blocking: ``pump()`` once
per training iteration performs at most one half-step (block landed -> H2D, act, actions D2H on
the side stream | actions landed -> ``step_async``).  Its launches are eager and sit between graph
replays, so the captured learner graph gains no node.  :meth:`AQLHostEvaluator.run` is the
blocking, deterministic form (in-process envs).
"""
from __future__ import annotations

import weakref

import numpy as np

from ..envs.host_vector import staging_views
from .host_eval import KERNELS, EpisodeLedger, WeightSets, _unregister, eval_seed

MAX_ENVS = 64   # one workgroup per evaluator env and CU (aql_host_eval_act)


class _Ledger(EpisodeLedger):
    """:class:`EpisodeLedger` over ``ended``, with the vector env's ``capped``: ended with
    ``done = 0`` (the ledger's own length cap is off)."""

    def __init__(self, n: int):
        super().__init__(n, cap=0)

    def observe_block(self, reward, done, ended, learn_step: int = 0) -> None:
        ends = np.flatnonzero(np.asarray(ended))
        first = len(self.finished)
        self.observe(reward, ended, learn_step)
        for j, e in enumerate(ends):
            if not done[e]:
                ret, length, _, at = self.finished[first + j]
                self.finished[first + j] = (ret, length, True, at)
                self.capped += 1


def make_pool(env_id: str, n: int, workers: int, seed: int = 0, max_episode_length: int = 50000, **kw):
    """The evaluator's worker pool: ``n`` envs of ``env_id`` in ``workers`` processes, env ``j``
    seeded ``eval_seed(seed) + j``."""
    from ..envs.proc_host_vector import ProcHostVectorEnv

    return ProcHostVectorEnv(env_id, n, workers=workers, seed=eval_seed(seed), max_episode_length=max_episode_length,
                             **kw)


class AQLHostEvaluator:
    """``len(vec)`` (at most 64) greedy evaluator envs of an AQL engine: the device state, both act
    forms, the weight sets and the blocking ``run``; see the module docstring.  ``trace``: the
    fused act also writes the candidate sets ``amu`` and their Q rows ``q`` (the step form always
    does)."""

    def __init__(self, engine, vec, kernel: str = "fused", seed: int = 0, trace: bool = False):
        import torch

        from ..models.aql import AQL
        from ..models.aql_fused import FusedAQL
        from .aql import flatten_module_params

        if kernel not in KERNELS:
            raise ValueError(f"kernel must be one of {KERNELS}, got {kernel!r}")
        N = len(vec)
        if not 1 <= N <= MAX_ENVS:
            raise ValueError(f"the AQL host evaluator runs 1..{MAX_ENVS} envs (one workgroup per env and CU), got {N}")
        if int(vec.obs_dim) != engine.obs or int(vec.action_dim) != engine.adim or bool(vec.continuous) != engine.cont:
            raise ValueError("the evaluator envs' obs_dim / action_dim / action kind differ from the model's")
        self.torch, self.hip = torch, engine.hip
        self.engine, self.vec, self.kernel = engine, vec, kernel
        self.device = dev = engine.device
        self.N, self.obs, self.adim, self.T = N, engine.obs, engine.adim, engine.T
        self.seed = int(seed)
        self.sd = eval_seed(self.seed) & 0xFFFFFFFFFFFF
        self.prop_seed, self.sel_seed = self.sd ^ 0x9909, self.sd ^ 0xA9C1
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
        self._obs_ptr = self.stage_dev.data_ptr() + 4 * N * self.obs   # the reset_obs rows
        self.env_act = torch.zeros(N, self.adim, **f32)
        self.act_idx = torch.zeros(N, **i32)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.amu = torch.zeros(N, self.T, self.adim, **f32)
        self.q = torch.zeros(N, self.T, **f32)
        self.eps = torch.zeros(N, **f32)
        self.ws = torch.zeros(self.hip.aql_workspace_floats(), **f32) if kernel == "step" else None
        self.act_host = torch.zeros(N, self.adim, dtype=torch.float32).pin_memory()
        self.actions_np = self.act_host.numpy()
        # two weight sets: an AQL module over flat parameters + its eval-mode handle each
        cfg, L = engine.cfg, engine.learner
        s = torch.cuda.current_stream().cuda_stream
        self.models, self.flats, self.nets, self._fused = [], [], [], []
        for _ in range(2):
            m = AQL(env=engine.host_env, propose_sample=cfg.propose_sample, uniform_sample=cfg.uniform_sample,
                    action_var=cfg.action_var, device=dev).to(dev)
            for p in m.parameters():
                p.requires_grad_(False)
            flat = flatten_module_params(m)
            if flat.numel() != L.P:
                raise ValueError("the evaluator's flat parameters differ in size from the learner's")
            self.hip.copy_f32(flat.data_ptr(), L.flat.data_ptr(), L.P, s)
            f = FusedAQL(m)
            self.models.append(m)
            self.flats.append(flat)
            self._fused.append(f)
            self.nets.append(f._net(noisy=False))
        self._acts = None
        if kernel == "fused":
            d = dict(N=N, prop_seed=self.prop_seed, sel_seed=self.sel_seed, stage=self.stage_dev.data_ptr(),
                     low=engine.low.data_ptr(), high=engine.high.data_ptr(), var=engine.var.data_ptr(),
                     env_act=self.env_act.data_ptr(), act_idx=self.act_idx.data_ptr(), counter=self.counter.data_ptr())
            if trace:
                d.update(amu=self.amu.data_ptr(), q=self.q.data_ptr())
            self._acts = [self.hip.make_aql_host_eval_act(net, d) for net in self.nets]
        self.stream = torch.cuda.Stream(device=dev)
        self.weights = WeightSets(torch.cuda.Event)
        self.acted = torch.cuda.Event()
        self.ledger = _Ledger(N)
        self.stream.wait_stream(torch.cuda.current_stream())   # (the buffers and weights above are set up)
        self.k = 0            # evaluator steps whose act has been enqueued
        self.learn_step = 0   # stamped on the episodes that end (the caller keeps it current)

    # ------------------------------------------------------------------ weights
    def _copy_weights(self, i: int, src_flat) -> None:
        self.hip.copy_f32(self.flats[i].data_ptr(), src_flat.data_ptr(), self.flats[i].numel(),
                          self.torch.cuda.current_stream().cuda_stream)

    def refresh(self, src_flat) -> bool:
        """Take the online flat parameters as they are at this point of the current (training)
        stream.  ``False`` and nothing done while the target set is still read."""
        return self.weights.refresh(lambda i: self._copy_weights(i, src_flat))

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
            h.aql_host_eval_act(self._acts[i], self.k, s)
        else:
            e, net = self.engine, self.nets[i]
            h.aql_propose(net, self._obs_ptr, self.N, e.low.data_ptr(), e.high.data_ptr(), e.var.data_ptr(),
                          self.prop_seed, self.counter.data_ptr(), self.amu.data_ptr(), 0, s)
            h.aql_candidate_q(net, self.ws.data_ptr(), self._obs_ptr, self.amu.data_ptr(), self.N, self.q.data_ptr(), s)
            h.aql_select(self.q.data_ptr(), self.amu.data_ptr(), self.N, self.T, self.adim, self.eps.data_ptr(),
                         self.sel_seed, self.counter.data_ptr(), self.act_idx.data_ptr(), self.env_act.data_ptr(), s)
            self.counter.add_(1)
        self.weights.release()
        self.act_host.copy_(self.env_act, non_blocking=True)
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


class AQLHostEvaluation:
    """The non-blocking driver of an :class:`AQLHostEvaluator` over a worker pool (``reset`` /
    ``step_async`` / ``poll``).  ``stream`` / ``event`` / ``stream_ctx`` default to the
    evaluator's and ``torch.cuda``'s (host tests pass fakes)."""

    def __init__(self, evaluator, pool, stream=None, event=None, stream_ctx=None):
        self.ev, self.pool = evaluator, pool
        self.stream = evaluator.stream if stream is None else stream
        if stream_ctx is None:
            import torch

            stream_ctx = torch.cuda.stream
        self._ctx = stream_ctx
        self.acted = evaluator.acted if event is None else event()
        self._closed = False
        self.pumps = 0
        pool.reset()          # (start-up: the one blocking call, before training runs)
        self._issue()

    def _issue(self) -> None:
        with self._ctx(self.stream):
            self.ev.ship()
            self.ev.act()
            if self.acted is not self.ev.acted:
                self.acted.record()
        self._state = "acting"

    @property
    def state(self) -> str:
        """``"acting"`` (the act and the actions' copy-out are in flight) or ``"stepping"`` (the
        workers step the envs)."""
        return self._state

    def refresh(self, src_flat) -> bool:
        return self.ev.refresh(src_flat)

    def pump(self, learn_step: int | None = None) -> None:
        """At most one half-step; never a blocking wait."""
        if self._closed:
            return
        self.pumps += 1
        ev, pool = self.ev, self.pool
        if learn_step is not None:
            ev.learn_step = int(learn_step)
        if self._state == "acting":
            if self.acted.query():
                pool.step_async(ev.actions_np)
                self._state = "stepping"
            return
        if not pool.poll():
            return
        ev.took()
        self._issue()

    def poll(self) -> list:
        return self.ev.poll()

    def close(self) -> None:
        """Synchronise the side stream, unregister the staging block, close the pool.  Idempotent."""
        if self._closed:
            return
        self._closed = True
        self.stream.synchronize()
        self.ev.close()
        self.pool.close()
