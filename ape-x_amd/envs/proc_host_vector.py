"""Process-pool host vector env: :class:`~apex_amd.envs.host_vector.HostVectorEnv` over worker
processes, the way :mod:`apex_amd.envs.proc_vector` wraps ``raw_vector``.

:class:`ProcHostVectorEnv` provides the ``HostVectorEnv`` protocol (``__len__``, ``obs_dim``,
``action_dim``, ``n_actions``, ``continuous``, ``low``, ``high``, ``max_episode_steps``,
``max_episode_length``, ``staging``, ``reset()``, ``step(actions)``, ``close()``) with the envs
stepped in ``workers`` child processes.  Worker ``w`` owns the contiguous env range
``banks[w] = bank_ranges(n, workers)[w]``, builds a ``HostVectorEnv`` over it and seeds env ``i``
with ``seed + i`` -- per-env RNG is the only randomness, so the pool computes what the in-process
``HostVectorEnv`` computes, byte for byte, whatever the timing of its workers.

Bulk data lives in ONE ``multiprocessing.shared_memory`` block.  Its first ``N * (2 * obs + 3)``
floats are ``staging``, exactly ``HostVectorEnv.staging``'s layout over all N envs::

    next_obs [N, obs] | reset_obs [N, obs] | reward [N] | done [N] | ended [N]

and each worker's ``HostVectorEnv`` writes the rows of its own envs there in place (its five views
are re-seated on the block).  The actions ``[N, action_dim]`` fp32 follow in the same block.
Control goes over one pipe per worker.

Non-blocking form: ``step_async(actions)`` starts one step on every worker; ``poll()`` returns
``True`` exactly once per step, when every bank has landed, and never waits; ``wait(timeout)``
is the bounded blocking form.  ``step(actions)`` is ``step_async`` + ``wait``.

Process rules and failure handling are :mod:`~apex_amd.envs.proc_vector`'s (its helpers and its
pipe plumbing are imported, not copied): fresh daemon children of the ``spawn`` context; this module
imports numpy and ``apex_amd.envs`` only, so a worker never loads torch or opens the GPU; the
thread-count variables are set for the child; no wait is unbounded; a worker that raises, exits
or stays silent past ``timeout`` seconds makes the call raise ``RuntimeError`` naming the worker
and its env range, the pool is then broken and every later call raises; ``close()`` is
idempotent, runs from ``__exit__`` and a finalizer and unlinks the block.
``factory="module:function"`` replaces ``envs.core.make`` in the child
(:func:`~apex_amd.envs.proc_vector.worker_info` tells it which worker it runs in).
"""
from __future__ import annotations

import multiprocessing as mp
import os
import signal
import time
import traceback
import weakref
from multiprocessing import shared_memory

import numpy as np

from . import proc_vector as _pv
from .host_vector import HostVectorEnv, staging_views
from .proc_vector import (_START_TIMEOUT, _THREAD_VARS, ProcRawAtariVector, _cleanup, _env_lock, _resolve,
                          bank_ranges)


def _block_views(buf, n: int, obs: int, adim: int):
    """``(staging, actions)`` of the shared block: ``n * (2 * obs + 3)`` floats, then ``[n, adim]``."""
    ns = n * (2 * obs + 3)
    staging = np.ndarray((ns,), dtype=np.float32, buffer=buf, offset=0)
    actions = np.ndarray((n, adim), dtype=np.float32, buffer=buf, offset=4 * ns)
    return staging, actions


# ---------------------------------------------------------------------------- child
def _worker_main(conn, w, e0, e1, env_id, seed, factory, max_episode_length):
    """One worker: build the bank's ``HostVectorEnv``, report its geometry, attach the shared block
    (the vector's five views move onto its rows), then serve reset / step until a stop message or
    the parent's end of the pipe closes."""
    _pv._WORKER = (w, e0, e1)                       # (what proc_vector.worker_info() answers in this child)
    signal.signal(signal.SIGINT, signal.SIG_IGN)    # the parent decides when a worker stops
    shm = None
    actions = None
    vec = None
    try:
        try:
            make_fn = _resolve(factory)
            vec = HostVectorEnv([lambda: make_fn(env_id)] * (e1 - e0), seed=int(seed) + e0,
                                max_episode_length=max_episode_length)
            conn.send(("ready", vec.obs_dim, vec.action_dim, vec.n_actions, vec.continuous,
                       tuple(float(x) for x in vec.low), tuple(float(x) for x in vec.high), vec.max_episode_steps))
        except BaseException:
            conn.send(("err", traceback.format_exc()))
            return
        while True:
            try:
                msg = conn.recv()
            except (EOFError, OSError):
                return                              # the parent is gone
            try:
                op = msg[0]
                if op == "stop":
                    return
                if op == "attach":
                    shm = shared_memory.SharedMemory(name=msg[1])
                    staging, actions = _block_views(shm.buf, msg[2], vec.obs_dim, vec.action_dim)
                    v = staging_views(staging, msg[2], vec.obs_dim)
                    vec.staging = None              # (the bank has no block of its own any more)
                    vec.next_obs, vec.reset_obs = v["next_obs"][e0:e1], v["reset_obs"][e0:e1]
                    vec.reward, vec.done, vec.ended = v["reward"][e0:e1], v["done"][e0:e1], v["ended"][e0:e1]
                    del staging, v
                elif op == "reset":
                    vec.reset()
                elif op == "step":
                    vec.step(actions[e0:e1])
                else:
                    raise ValueError(f"unknown message {op!r}")
                conn.send(("ok",))
            except Exception:
                conn.send(("err", traceback.format_exc()))
                return
    finally:
        actions = None
        if vec is not None:
            vec.next_obs = vec.reset_obs = vec.reward = vec.done = vec.ended = None
        if shm is not None:
            try:
                shm.close()
            except BufferError:
                pass
        conn.close()


# ---------------------------------------------------------------------------- parent
class ProcHostVectorEnv:
    def __init__(self, env_id: str, n: int, workers: int = 2, seed: int = 0, max_episode_length: int = 50000,
                 factory: str | None = None, timeout: float = 60.0):
        n, workers = int(n), int(workers)
        self.banks = bank_ranges(n, workers)        # (ValueError before any process starts)
        if factory is not None and (":" not in factory or not all(factory.partition(":")[::2])):
            raise ValueError(f"factory must be 'module:function', got {factory!r}")
        self.env_id, self.seed, self.timeout = env_id, int(seed), float(timeout)
        self.max_episode_length = int(max_episode_length)
        self._n = n
        self._procs, self._conns, self._shared = [], [], {}
        self._broken = None
        self._closed = False
        self._pending, self._inflight = set(), False
        self._deadline = 0.0
        self._finalizer = weakref.finalize(self, _cleanup, self._procs, self._conns, self._shared)
        try:
            self._start(factory)
        except BaseException:
            self.close()
            raise

    def _start(self, factory) -> None:
        ctx = mp.get_context("spawn")
        with _env_lock:                             # the child inherits the environment of this moment
            saved = {k: os.environ.get(k) for k in _THREAD_VARS}
            try:
                os.environ.update({k: "1" for k in _THREAD_VARS})
                for w, (e0, e1) in enumerate(self.banks):
                    ours, theirs = ctx.Pipe(duplex=True)
                    p = ctx.Process(target=_worker_main, name=f"apex-host-env-worker-{w}", daemon=True,
                                    args=(theirs, w, e0, e1, self.env_id, self.seed, factory,
                                          self.max_episode_length))
                    p.start()
                    theirs.close()
                    self._procs.append(p)
                    self._conns.append(ours)
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        geo = self._gather(set(range(len(self.banks))), time.monotonic() + max(self.timeout, _START_TIMEOUT))
        shapes = {m[1:] for m in geo.values()}
        if len(shapes) != 1 or any(m[0] != "ready" for m in geo.values()):
            raise RuntimeError(f"ProcHostVectorEnv: the workers disagree on the env geometry: {sorted(map(str, shapes))}")
        (obs, adim, n_actions, cont, low, high, limit), = shapes
        self.obs_dim, self.action_dim, self.n_actions = int(obs), int(adim), int(n_actions)
        self.continuous = bool(cont)
        self.low, self.high = np.asarray(low, dtype=np.float32), np.asarray(high, dtype=np.float32)
        self.max_episode_steps = None if limit is None else int(limit)
        shm = shared_memory.SharedMemory(create=True, size=4 * self._n * (2 * self.obs_dim + 3 + self.action_dim))
        self._shared["shm"] = shm
        v = _block_views(shm.buf, self._n, self.obs_dim, self.action_dim)
        self._shared["views"] = v
        self.staging, self._actions = v
        self.staging[:] = 0.0
        self._actions[:] = 0.0
        self._seat()
        self._call([("attach", shm.name, self._n)] * len(self.banks))

    def _seat(self) -> None:
        v = {} if self.staging is None else staging_views(self.staging, self._n, self.obs_dim)
        for k in ("next_obs", "reset_obs", "reward", "done", "ended"):
            setattr(self, k, v.get(k))

    # -- plumbing: proc_vector's, over this pool's pipes, processes, banks and time limit
    _send, _poll, _answer, _blame = (ProcRawAtariVector._send, ProcRawAtariVector._poll, ProcRawAtariVector._answer,
                                     ProcRawAtariVector._blame)
    _gather, _call = ProcRawAtariVector._gather, ProcRawAtariVector._call

    def _fail(self, w: int, what: str):
        e0, e1 = self.banks[w]
        self._broken = f"ProcHostVectorEnv: worker {w} (envs [{e0}, {e1})) {what}"
        raise RuntimeError(self._broken)

    def _usable(self) -> None:
        if self._closed:
            raise RuntimeError("ProcHostVectorEnv is closed")
        if self._broken:
            raise RuntimeError(self._broken + " (earlier; the pool is broken)")

    def _idle(self) -> None:
        self._usable()
        if self._inflight:
            raise RuntimeError("ProcHostVectorEnv: a step is in flight: take it with poll() / wait() first")

    # -- the protocol
    def __len__(self) -> int:
        return self._n

    def reset(self) -> np.ndarray:
        """Start every env; the first observations fill ``reset_obs`` (returned)."""
        self._idle()
        self._call([("reset",)] * len(self.banks))
        return self.reset_obs

    def step(self, actions) -> None:
        self.step_async(actions)
        self.wait()

    # -- the non-blocking form
    def step_async(self, actions) -> None:
        """Start one step of every env with ``actions`` (fp32 ``[N, action_dim]``)."""
        self._idle()
        a = np.asarray(actions, dtype=np.float32)
        if a.size != self._n * self.action_dim:
            raise ValueError(f"actions must have shape ({self._n}, {self.action_dim}), got {a.shape}")
        self._actions[:] = a.reshape(self._n, self.action_dim)
        self._deadline = time.monotonic() + self.timeout
        self._pending = set(range(len(self.banks)))
        self._inflight = True
        for w in range(len(self.banks)):
            self._send(w, ("step",))

    def _collect(self, deadline: float, block: bool) -> bool:
        self._usable()
        if not self._inflight:
            raise RuntimeError("ProcHostVectorEnv: no step in flight (it was taken)")
        while self._pending:
            got = self._poll(self._pending, deadline, block=block)
            for w, _ in got:
                self._pending.discard(w)
            if not block:
                break
        if self._pending:
            return False
        self._inflight = False
        return True

    def poll(self) -> bool:
        """``True`` exactly once per step, when every bank has landed in ``staging``; ``False`` at
        once while a worker is still stepping.  A worker that raised, exited or has been silent past
        the step's time limit raises."""
        return self._collect(self._deadline, block=False)

    def wait(self, timeout: float | None = None) -> None:
        """Block until the step in flight has landed, for at most ``timeout`` seconds (default: what
        is left of the step's time limit); a worker still silent then raises."""
        self._collect(self._deadline if timeout is None else time.monotonic() + float(timeout), block=True)

    # -- teardown
    @property
    def processes(self):
        """The worker ``multiprocessing.Process`` objects (kept after :meth:`close`)."""
        return list(self._procs)

    def close(self) -> None:
        self._closed = True
        self.staging = self._actions = None
        self._seat()
        self._finalizer()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()
