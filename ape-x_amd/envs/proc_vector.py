"""Process-pool raw vector env: :class:`RawAtariVector` over worker processes.

:class:`ProcRawAtariVector` provides the vector-env protocol of :mod:`apex_amd.envs.raw_vector`
(``__len__``, ``raw_shape``, ``n_actions``, ``reset(out)``, ``step(actions, out)``) with the
emulators stepped in ``workers`` child processes.  Worker ``w`` owns the contiguous env range
``banks[w] = (e0, e1)`` (a *bank*), builds ``RawAtariVector([make(env_id) ...], spec)`` over it
and seeds env ``i`` with ``seed + i`` -- per-env RNG is the only randomness, so the pool computes
what the in-process vector computes, byte for byte, whatever the timing of its workers.

Bulk data lives in ONE ``multiprocessing.shared_memory`` block: ``staging`` (``[N, 2, H, W, 3]``
uint8, each worker writes the pairs of its own envs), rewards, dones and actions.  Control goes
over one pipe per worker.  ``reset(out)`` / ``step(actions, out)`` with ``out is vec.staging``
copy nothing; any other ``out`` is filled by a copy.

Banked form: ``step_async(actions)`` starts one agent step on every worker and
``wait_bank() -> (b, reward[e0:e1], done[e0:e1])`` hands back each bank exactly once per step, in
completion order (the slices are views of the shared block, valid until the next step starts) --
a consumer can ship bank ``b`` to the GPU while the other workers are still emulating.
``poll_bank()`` is ``wait_bank()`` with a zero wait: the next finished bank, or ``None`` at once
while every pending worker is still stepping (same exactly-once bookkeeping, same failure handling).
``max_episode_steps`` is handed to every worker's ``RawAtariVector`` (0 = no cap).

Failure handling: no wait is unbounded.  A worker that raises, exits or stays silent past
``timeout`` seconds makes the call raise ``RuntimeError`` naming the worker and its env range (an
exception in the child arrives with its traceback text; of several failed workers the lowest-numbered
one is named, whatever the order their failures arrived in); the pool is then broken, every later
call raises, and ``close()`` still returns.  ``close()`` is idempotent, runs from ``__exit__`` and
from a finalizer, stops the workers (stop message, then ``terminate``, then ``kill``, each with a
short join) and unlinks the shared block.

Process rules: children are fresh daemon processes of the ``spawn`` context (never a fork of a
process that may hold a GPU).  This module imports numpy and ``apex_amd.envs`` only, so a worker
never loads torch or opens the GPU.  Each worker runs single-threaded: the BLAS / OpenMP
thread-count variables are set in the environment the child is started with (and put back in the
parent at once).  The worker count is the caller's; nothing here looks at the CPU count.

``factory="module:function"`` replaces ``envs.core.make``: the CHILD imports ``module`` and calls
``function(env_id)`` per env (:func:`worker_info` tells it which worker it runs in).
"""
from __future__ import annotations

import collections
import importlib
import multiprocessing as mp
import multiprocessing.connection as mpc
import os
import signal
import threading
import time
import traceback
import weakref
from multiprocessing import shared_memory

import numpy as np

from . import spaces
from .preprocess import PreprocessSpec
from .raw_vector import RawAtariVector

_THREAD_VARS = ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "NUMEXPR_NUM_THREADS",
                "VECLIB_MAXIMUM_THREADS", "BLIS_NUM_THREADS")
_START_TIMEOUT = 60.0   # floor of the bound on worker start-up (interpreter + imports + env construction)
_JOIN = 0.5             # the "short join" after stop / terminate / kill
_BLAME = 2.0            # grace for lower-numbered workers to report a failure of their own (see _blame)
_env_lock = threading.Lock()
_WORKER = None


def worker_info():
    """``(worker index, e0, e1)`` inside a worker process, ``None`` anywhere else."""
    return _WORKER


def bank_ranges(n_envs: int, workers: int):
    """``workers`` contiguous ranges covering ``[0, n_envs)`` in order, sizes differing by <= 1."""
    if workers < 1 or workers > n_envs:
        raise ValueError(f"workers must be in [1, n_envs = {n_envs}], got {workers}")
    q, r = divmod(n_envs, workers)
    out, e = [], 0
    for w in range(workers):
        n = q + (1 if w < r else 0)
        out.append((e, e + n))
        e += n
    return out


def _layout(n_envs: int, raw_shape):
    """Byte offsets of (staging, reward f64, action i64, done bool) in the shared block, and its size."""
    pair = 2 * int(np.prod(raw_shape))
    off_r = -(-n_envs * pair // 64) * 64
    off_a = off_r + 8 * n_envs
    off_d = off_a + 8 * n_envs
    return off_r, off_a, off_d, off_d + -(-n_envs // 64) * 64


def _views(buf, n_envs: int, raw_shape):
    off_r, off_a, off_d, _ = _layout(n_envs, raw_shape)
    staging = np.ndarray((n_envs, 2) + tuple(raw_shape), dtype=np.uint8, buffer=buf, offset=0)
    reward = np.ndarray((n_envs,), dtype=np.float64, buffer=buf, offset=off_r)
    action = np.ndarray((n_envs,), dtype=np.int64, buffer=buf, offset=off_a)
    done = np.ndarray((n_envs,), dtype=np.bool_, buffer=buf, offset=off_d)
    return staging, reward, action, done


# ---------------------------------------------------------------------------- child
def _resolve(factory):
    if factory is None:
        from .core import make

        return make
    mod, _, fn = factory.partition(":")
    if not mod or not fn:
        raise ValueError(f"factory must be 'module:function', got {factory!r}")
    return getattr(importlib.import_module(mod), fn)


def _worker_main(conn, w, e0, e1, env_id, spec, seed, factory, max_episode_steps=0):
    """One worker: build the bank's vector, report its geometry, attach the shared block, then
    serve reset / step / seed / noops until a stop message or the parent's end of the pipe closes."""
    global _WORKER
    _WORKER = (w, e0, e1)
    signal.signal(signal.SIGINT, signal.SIG_IGN)   # the parent decides when a worker stops
    shm = None
    views = None
    try:
        try:
            make_fn = _resolve(factory)
            vec = RawAtariVector([make_fn(env_id) for _ in range(e0, e1)], spec, max_episode_steps)
            if seed is not None:
                vec.seed(seed + e0)
            conn.send(("ready", tuple(vec.raw_shape), int(vec.n_actions)))
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
                    views = _views(shm.buf, msg[2], vec.raw_shape)
                elif op == "reset":
                    vec.reset(views[0][e0:e1])
                elif op == "step":
                    staging, reward, action, done = views
                    r, d = vec.step(action[e0:e1], staging[e0:e1])
                    reward[e0:e1] = r
                    done[e0:e1] = d
                elif op == "seed":
                    vec.seed(msg[1] + e0)
                elif op == "noops":
                    vec.fixed_noops = list(msg[1])
                else:
                    raise ValueError(f"unknown message {op!r}")
                conn.send(("ok",))
            except Exception:
                conn.send(("err", traceback.format_exc()))
                return
    finally:
        views = None
        if shm is not None:
            try:
                shm.close()
            except BufferError:
                pass
        conn.close()


# ---------------------------------------------------------------------------- parent
def _stop_workers(procs, conns):
    for c in conns:
        try:
            c.send(("stop",))
        except (OSError, ValueError):
            pass
    for step in ("join", "terminate", "kill"):
        alive = [p for p in procs if p.is_alive()]
        if not alive:
            break
        if step != "join":
            for p in alive:
                getattr(p, step)()
        deadline = time.monotonic() + _JOIN
        for p in alive:
            p.join(max(0.0, deadline - time.monotonic()))
    for c in conns:
        try:
            c.close()
        except OSError:
            pass


def _cleanup(procs, conns, holder):
    """The whole teardown, free of any reference to the pool object (it is the finalizer)."""
    _stop_workers(procs, conns)
    shm = holder.pop("shm", None)
    holder.clear()                                  # drops the pool's own views of the block
    if shm is not None:
        try:
            shm.close()
        except BufferError:                         # someone still holds a view: the mapping lives on with it
            _parked.append(shm)
        try:
            shm.unlink()
        except FileNotFoundError:
            pass


_parked = []   # blocks unlinked while a caller still held a view of them (kept mapped, never reopened)


class ProcRawAtariVector:
    def __init__(self, env_id: str, n_envs: int, spec: PreprocessSpec = PreprocessSpec(), workers: int = 2,
                 seed: int | None = None, factory: str | None = None, timeout: float = 60.0,
                 max_episode_steps: int = 0):
        n_envs, workers = int(n_envs), int(workers)
        if int(max_episode_steps) < 0:
            raise ValueError("max_episode_steps must be >= 0 (0 = no cap)")
        self.max_episode_steps = int(max_episode_steps)
        self.banks = bank_ranges(n_envs, workers)   # (ValueError before any process starts)
        if factory is not None and (":" not in factory or not all(factory.partition(":")[::2])):
            raise ValueError(f"factory must be 'module:function', got {factory!r}")
        self.env_id, self.spec, self.timeout = env_id, spec, float(timeout)
        self._n = n_envs
        self._procs, self._conns, self._shared = [], [], {}
        self._broken = None
        self._closed = False
        self._pending, self._ready = set(), collections.deque()
        self._deadline = 0.0
        self._finalizer = weakref.finalize(self, _cleanup, self._procs, self._conns, self._shared)
        try:
            self._start(seed, factory)
        except BaseException:
            self.close()
            raise

    def _start(self, seed, factory) -> None:
        ctx = mp.get_context("spawn")
        with _env_lock:                             # the child inherits the environment of this moment
            saved = {k: os.environ.get(k) for k in _THREAD_VARS}
            try:
                os.environ.update({k: "1" for k in _THREAD_VARS})
                for w, (e0, e1) in enumerate(self.banks):
                    ours, theirs = ctx.Pipe(duplex=True)
                    p = ctx.Process(target=_worker_main, name=f"apex-env-worker-{w}", daemon=True,
                                    args=(theirs, w, e0, e1, self.env_id, self.spec, seed, factory,
                                          self.max_episode_steps))
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
            raise RuntimeError(f"ProcRawAtariVector: the workers disagree on the env geometry: {sorted(shapes)}")
        (raw_shape, n_actions), = shapes
        self.raw_shape = tuple(int(x) for x in raw_shape)
        self.n_actions = int(n_actions)
        self.action_space = spaces.Discrete(self.n_actions)
        size = _layout(self._n, self.raw_shape)[3]
        shm = shared_memory.SharedMemory(create=True, size=size)
        self._shared["shm"] = shm
        self.shm_name = shm.name
        v = _views(shm.buf, self._n, self.raw_shape)
        self._shared["views"] = v
        self.staging, self._reward, self._action, self._done = v
        self._noops = [None] * self._n
        self._call([("attach", shm.name, self._n)] * len(self.banks))

    # -- plumbing
    def _fail(self, w: int, what: str):
        e0, e1 = self.banks[w]
        self._broken = f"ProcRawAtariVector: worker {w} (envs [{e0}, {e1})) {what}"
        raise RuntimeError(self._broken)

    def _usable(self) -> None:
        if self._closed:
            raise RuntimeError("ProcRawAtariVector is closed")
        if self._broken:
            raise RuntimeError(self._broken + " (earlier; the pool is broken)")

    def _send(self, w: int, msg) -> None:
        try:
            self._conns[w].send(msg)
        except (OSError, ValueError) as e:
            self._fail(w, f"is gone: {type(e).__name__}: {e}")

    def _poll(self, pending, deadline: float, block: bool = True):
        """Block until at least one worker of ``pending`` has answered (bounded by ``deadline``);
        return ``[(w, message)]`` in the order the answers were seen.  ``block=False``: look once
        without waiting; nothing ready is ``[]`` while the deadline has not passed."""
        objs = {}
        for w in sorted(pending):
            objs[self._conns[w]] = w
            objs[self._procs[w].sentinel] = w
        ready = mpc.wait(list(objs), max(0.0, deadline - time.monotonic()) if block else 0.0)
        if not ready:
            if not block and time.monotonic() < deadline:
                return []
            self._fail(min(pending), f"gave no answer within the time limit ({self.timeout:g} s)")
        out, seen, failed = [], set(), {}
        for o in ready:
            w = objs[o]
            if w in seen:
                continue
            seen.add(w)
            msg, what = self._answer(w)
            if what is not None:
                failed[w] = what
            else:
                out.append((w, msg))
        if failed:
            self._blame(failed, {w for w in pending if w not in seen and w < min(failed)}, deadline)
        return out

    def _answer(self, w: int):
        """Worker ``w`` has something to say: ``(message, None)``, or ``(None, what went wrong)``."""
        conn, msg = self._conns[w], None
        try:
            if conn.poll(0):                    # (also true at end-of-file)
                msg = conn.recv()
        except (EOFError, OSError):
            msg = None
        if msg is None:
            self._procs[w].join(_JOIN)
            return None, f"exited unexpectedly (exit code {self._procs[w].exitcode})"
        if msg[0] == "err":
            return None, "raised:\n" + msg[1]
        return msg, None

    def _blame(self, failed: dict, lower: set, deadline: float):
        """Raise for the LOWEST-numbered failed worker.  A fault common to all workers (a bad
        factory, a missing env) reaches the parent in any order, so the lower-numbered workers still
        pending get a short grace (``_BLAME`` s, within ``deadline``) to report theirs: which worker
        the error names does not depend on the timing of the workers."""
        end = min(deadline, time.monotonic() + _BLAME)
        while lower:
            objs = {}
            for w in lower:
                objs[self._conns[w]] = w
                objs[self._procs[w].sentinel] = w
            ready = mpc.wait(list(objs), max(0.0, end - time.monotonic()))
            if not ready:
                break
            for w in {objs[o] for o in ready}:
                lower.discard(w)
                what = self._answer(w)[1]       # (an answer that is no failure is dropped: the pool is broken)
                if what is not None:
                    failed[w] = what
        w = min(failed)
        self._fail(w, failed[w])

    def _gather(self, pending, deadline: float) -> dict:
        got, pending = {}, set(pending)
        while pending:
            for w, msg in self._poll(pending, deadline):
                got[w] = msg
                pending.discard(w)
        return got

    def _call(self, msgs) -> None:
        """One message per worker, then every worker's acknowledgement."""
        for w, m in enumerate(msgs):
            self._send(w, m)
        self._gather(set(range(len(msgs))), time.monotonic() + self.timeout)

    def _idle(self) -> None:
        self._usable()
        if self._pending or self._ready:
            raise RuntimeError("ProcRawAtariVector: a step is in flight: take every bank with wait_bank() first")

    def _check(self, out) -> None:
        want = (self._n, 2) + self.raw_shape
        if tuple(out.shape) != want or out.dtype != np.uint8:
            raise ValueError(f"out must be uint8 {want}, got {out.dtype} {tuple(out.shape)}")

    # -- the protocol
    def __len__(self) -> int:
        return self._n

    def reset(self, out: np.ndarray) -> None:
        self._check(out)
        self._idle()
        self._call([("reset",)] * len(self.banks))
        if out is not self.staging:
            out[...] = self.staging

    def step(self, actions, out: np.ndarray):
        self._check(out)
        self.step_async(actions)
        for _ in self.banks:
            self.wait_bank()
        if out is not self.staging:
            out[...] = self.staging
        return self._reward.copy(), self._done.copy()

    def seed(self, seed: int) -> None:
        self._idle()
        self._call([("seed", int(seed))] * len(self.banks))

    @property
    def fixed_noops(self):
        return list(self._noops)

    @fixed_noops.setter
    def fixed_noops(self, value) -> None:
        value = list(value)
        if len(value) != self._n:
            raise ValueError(f"fixed_noops needs one entry per env ({self._n}), got {len(value)}")
        self._idle()
        self._call([("noops", value[e0:e1]) for e0, e1 in self.banks])
        self._noops = value

    # -- the banked form
    def step_async(self, actions) -> None:
        """Start one agent step of every env; collect the banks with :meth:`wait_bank`."""
        self._idle()
        a = np.asarray(actions)
        if a.shape != (self._n,):
            raise ValueError(f"actions must have shape ({self._n},), got {a.shape}")
        self._action[:] = a
        self._deadline = time.monotonic() + self.timeout
        self._pending = set(range(len(self.banks)))
        for w in range(len(self.banks)):
            self._send(w, ("step",))

    def wait_bank(self, timeout: float | None = None):
        """``(b, reward[e0:e1], done[e0:e1])`` of the next bank to finish; each bank once per step."""
        self._usable()
        if not self._ready:
            if not self._pending:
                raise RuntimeError("ProcRawAtariVector: no step in flight (every bank was taken)")
            deadline = self._deadline if timeout is None else time.monotonic() + float(timeout)
            for w, _ in self._poll(self._pending, deadline):
                self._pending.discard(w)
                self._ready.append(w)
        b = self._ready.popleft()
        e0, e1 = self.banks[b]
        return b, self._reward[e0:e1], self._done[e0:e1]

    def poll_bank(self):
        """:meth:`wait_bank` with a zero wait: the next finished bank, or ``None`` at once while
        every pending worker is still stepping.  Each bank still arrives exactly once per step; a
        worker that raised, exited or has been silent past the step's time limit raises as there."""
        self._usable()
        if not self._ready:
            if not self._pending:
                raise RuntimeError("ProcRawAtariVector: no step in flight (every bank was taken)")
            for w, _ in self._poll(self._pending, self._deadline, block=False):
                self._pending.discard(w)
                self._ready.append(w)
            if not self._ready:
                return None
        b = self._ready.popleft()
        e0, e1 = self.banks[b]
        return b, self._reward[e0:e1], self._done[e0:e1]

    # -- teardown
    @property
    def processes(self):
        """The worker ``multiprocessing.Process`` objects (kept after :meth:`close`)."""
        return list(self._procs)

    def close(self) -> None:
        self._closed = True
        self.staging = self._reward = self._action = self._done = None
        self._finalizer()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()
