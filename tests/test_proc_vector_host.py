"""CPU tests of the process-pool vector env (``envs/proc_vector.py``): bit equality with the
in-process ``RawAtariVector`` (synthetic Seaquest and Breakout, a scripted short-episode
emulator, fixed no-op counts), bank geometry, the banked form, the no-copy staging path, and
failure handling (a worker that raises, exits or stays silent) with a clean teardown after each."""
import importlib
import time
from multiprocessing import shared_memory

import numpy as np
import pytest

from apex_amd.envs.core import make
from apex_amd.envs.preprocess import PreprocessSpec
from apex_amd.envs.proc_vector import ProcRawAtariVector, bank_ranges, worker_info
from apex_amd.envs.raw_vector import RawAtariVector

from . import proc_vector_fixtures as fx

FIX = "tests.proc_vector_fixtures"
SEAQUEST, BREAKOUT = "SeaquestNoFrameskip-v4", "BreakoutNoFrameskip-v4"


def _local(env_id, n, seed, factory=None):
    build = make if factory is None else getattr(importlib.import_module(factory.split(":")[0]), factory.split(":")[1])
    v = RawAtariVector([build(env_id) for _ in range(n)], PreprocessSpec())
    v.seed(seed)
    return v


def _assert_closed(vec):
    """Every child gone, the shared block unlinked."""
    assert vec.processes and all(not p.is_alive() for p in vec.processes)
    with pytest.raises(FileNotFoundError):
        shared_memory.SharedMemory(name=vec.shm_name)


def _compare(env_id, steps, factory=None, noops=None, seed=31):
    """(dones per env) after comparing pool and in-process vector after reset and every step."""
    N = 5
    ref = _local(env_id, N, seed, factory)
    with ProcRawAtariVector(env_id, N, workers=2, seed=seed, factory=factory) as vec:
        assert vec.banks == [(0, 3), (3, 5)]
        assert len(vec) == N and vec.raw_shape == ref.raw_shape and vec.n_actions == ref.n_actions
        assert vec.action_space == ref.action_space
        if noops is not None:
            ref.fixed_noops = list(noops)
            vec.fixed_noops = list(noops)
            assert vec.fixed_noops == list(noops)
        want = np.zeros((N, 2) + ref.raw_shape, np.uint8)
        ref.reset(want)
        vec.reset(vec.staging)
        assert np.array_equal(vec.staging, want)
        rng = np.random.default_rng(seed)
        n_done = np.zeros(N, np.int64)
        for t in range(steps):
            acts = rng.integers(0, ref.n_actions, N)
            r_ref, d_ref = ref.step(acts, want)
            r, d = vec.step(acts, vec.staging)
            assert r.dtype == np.float64 and d.dtype == bool
            assert np.array_equal(r, r_ref) and np.array_equal(d, d_ref), t
            assert np.array_equal(vec.staging, want), t
            n_done += d_ref
    _assert_closed(vec)
    return n_done


def test_pool_equals_in_process_seaquest():
    _compare(SEAQUEST, 20)


def test_pool_equals_in_process_breakout_fire_start():
    assert _local(BREAKOUT, 1, 0).fire
    _compare(BREAKOUT, 20)


def test_pool_equals_in_process_short_episodes_auto_reset():
    n_done = _compare(SEAQUEST, 60, factory=f"{FIX}:short")
    assert n_done[:3].sum() >= 1 and n_done[3:].sum() >= 1   # each bank compared the auto-reset path
    assert (n_done >= 1).all()


def test_pool_equals_in_process_with_fixed_noops():
    _compare(SEAQUEST, 6, noops=[3, 1, 7, 2, 12])


@pytest.mark.parametrize("N,W,want", [(5, 2, [(0, 3), (3, 5)]), (4, 4, [(0, 1), (1, 2), (2, 3), (3, 4)]),
                                      (7, 3, [(0, 3), (3, 5), (5, 7)])])
def test_bank_geometry(N, W, want):
    banks = bank_ranges(N, W)
    assert banks == want
    assert banks[0][0] == 0 and banks[-1][1] == N and all(a[1] == b[0] for a, b in zip(banks, banks[1:]))
    sizes = [e1 - e0 for e0, e1 in banks]
    assert max(sizes) - min(sizes) <= 1


@pytest.mark.parametrize("workers", [0, 6])
def test_bad_worker_count_starts_nothing(workers, monkeypatch):
    import multiprocessing.context as ctx

    started = []
    monkeypatch.setattr(ctx.SpawnProcess, "start", lambda self: started.append(self))
    with pytest.raises(ValueError):
        ProcRawAtariVector(SEAQUEST, 5, workers=workers)
    assert not started
    import multiprocessing

    assert not [p for p in multiprocessing.active_children() if p.name.startswith("apex-env-worker")]


def test_worker_info_is_none_in_the_parent():
    assert worker_info() is None


def test_workers_are_torch_free_single_threaded_daemons(monkeypatch):
    """The factory runs in the child and fails its start-up if torch is loaded or the thread-count
    variables are not 1; the parent's own environment is what it was."""
    import os

    monkeypatch.setenv("OMP_NUM_THREADS", "5")
    monkeypatch.delenv("OPENBLAS_NUM_THREADS", raising=False)
    with ProcRawAtariVector(SEAQUEST, 2, workers=2, seed=0, factory=f"{FIX}:checked") as vec:
        assert all(p.daemon and p.is_alive() for p in vec.processes)
        assert os.environ["OMP_NUM_THREADS"] == "5" and "OPENBLAS_NUM_THREADS" not in os.environ
    with pytest.raises(RuntimeError, match="worker 0"):
        ProcRawAtariVector(SEAQUEST, 2, workers=2, factory=f"{FIX}:no_such_function")


def test_banked_form_staging_identity_and_context_manager():
    N = 5
    with ProcRawAtariVector(SEAQUEST, N, workers=2, seed=4) as a, ProcRawAtariVector(SEAQUEST, N, workers=2,
                                                                                       seed=4) as b:
        addr = a.staging.__array_interface__["data"][0]
        a.reset(a.staging)
        foreign = np.zeros_like(b.staging)
        b.reset(foreign)                                   # a foreign out is filled
        assert np.array_equal(foreign, a.staging) and foreign.any()
        rng = np.random.default_rng(0)
        for t in range(4):
            acts = rng.integers(0, a.n_actions, N)
            a.step_async(acts)
            with pytest.raises(RuntimeError):
                a.step_async(acts)                         # no bank was taken yet
            first = a.wait_bank()
            with pytest.raises(RuntimeError):
                a.step_async(acts)                         # one bank is still out
            second = a.wait_bank(timeout=30.0)
            assert sorted([first[0], second[0]]) == [0, 1]  # every bank exactly once
            with pytest.raises(RuntimeError):
                a.wait_bank()                              # nothing left to take
            r, d = np.zeros(N), np.zeros(N, bool)
            for bank, rb, db in (first, second):
                e0, e1 = a.banks[bank]
                assert rb.shape == (e1 - e0,) and db.shape == (e1 - e0,)
                r[e0:e1], d[e0:e1] = rb, db
            foreign[...] = 0
            r2, d2 = b.step(acts, foreign)                 # the blocking form, into a foreign buffer
            assert np.array_equal(r, r2) and np.array_equal(d, d2)
            assert np.array_equal(a.staging, foreign), t
            assert a.staging.__array_interface__["data"][0] == addr   # out is staging: nothing was copied
        with pytest.raises(ValueError):
            a.step(np.zeros(N, np.int64), np.zeros((N, 210, 160, 3), np.uint8))
        with pytest.raises(ValueError):
            a.step(np.zeros(N, np.int64), np.zeros(a.staging.shape, np.float32))
    _assert_closed(a)
    _assert_closed(b)
    a.close()                                              # idempotent
    with pytest.raises(RuntimeError):
        a.step_async(np.zeros(N, np.int64))


@pytest.mark.parametrize("how,timeout,text", [("raises", 30.0, "ZeroDivisionError: scripted emulator failure"),
                                             ("exits", 30.0, "exit code 3"), ("sleeps", 1.0, "time limit")])
def test_worker_failure_raises_and_close_returns(how, timeout, text):
    N = 5
    vec = ProcRawAtariVector(SEAQUEST, N, workers=2, seed=1, factory=f"{FIX}:{how}", timeout=timeout)
    try:
        vec.reset(vec.staging)
        ok = np.zeros(N, np.int64)
        vec.step(ok, vec.staging)
        vec.step(ok, vec.staging)
        t0 = time.monotonic()
        with pytest.raises(RuntimeError) as ei:            # the third step: worker 1's emulators misbehave
            vec.step(np.full(N, fx.TRIGGER), vec.staging)
        assert time.monotonic() - t0 < timeout + 5.0
        msg = str(ei.value)
        assert "worker 1" in msg and "[3, 5)" in msg and text in msg
        if how == "raises":
            assert "Traceback" in msg and "proc_vector_fixtures" in msg
        with pytest.raises(RuntimeError):
            vec.step(ok, vec.staging)                      # the pool stays broken
    finally:
        vec.close()
    _assert_closed(vec)
    vec.close()
