"""Host checks of the host vector env's worker pool (``envs/proc_host_vector.py``): bit equality
with the in-process ``HostVectorEnv``, the non-blocking form and the failure handling."""
import time

import numpy as np
import pytest

from apex_amd.envs.host_vector import HostVectorEnv, staging_views
from apex_amd.envs.proc_host_vector import ProcHostVectorEnv
from apex_amd.envs.proc_vector import bank_ranges

PROTOCOL = ("obs_dim", "action_dim", "n_actions", "continuous", "max_episode_steps", "max_episode_length")


def _actions(rng, vec, n):
    if vec.continuous:
        return rng.uniform(vec.low, vec.high, size=(n, vec.action_dim)).astype(np.float32)
    a = rng.integers(0, vec.n_actions, size=(n, 1)).astype(np.float32)
    a[:2] = 0.0      # envs 0 and 1 always push the same way: CartPole falls after 9 or 10 steps
    return a


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---------------------------------------------------------------------------- bit equality
# CartPole cannot fall in fewer than 9 steps from its reset range (|theta| <= 0.05, threshold 0.2095,
# a constant push), so under a cap of 7 every episode end is a cap reset and no ``done = 1`` can
# occur; the cap-10 case is the one in which both kinds of end occur, and it asserts both.
@pytest.mark.parametrize("env_id,n,workers,steps,cap,want", [
    ("CartPole-v0", 5, 2, 60, 7, (0, 1)), ("CartPole-v0", 5, 2, 60, 10, (1, 1)), ("Pendulum-v0", 3, 3, 25, 50000, (0, 0))])
def test_pool_equals_the_in_process_vector_bit_for_bit(env_id, n, workers, steps, cap, want):
    seed = 21
    ref = HostVectorEnv(env_id, n, seed=seed, max_episode_length=cap)
    with ProcHostVectorEnv(env_id, n, workers=workers, seed=seed, max_episode_length=cap, timeout=30.0,
                           factory="tests.proc_host_vector_fixtures:checked") as pool:
        assert pool.banks == bank_ranges(n, workers) and len(pool) == n == len(ref)
        if env_id == "CartPole-v0":
            assert [e1 - e0 for e0, e1 in pool.banks] == [3, 2]        # ragged banks
        for k in PROTOCOL:
            assert getattr(pool, k) == getattr(ref, k), k
        assert np.array_equal(pool.low, ref.low) and np.array_equal(pool.high, ref.high)
        assert pool.staging.dtype == np.float32 and pool.staging.shape == ref.staging.shape
        assert pool.staging.flags.c_contiguous
        first = pool.reset()
        ref.reset()
        assert first is pool.reset_obs
        assert np.array_equal(_bits(pool.staging), _bits(ref.staging))
        rng = np.random.default_rng(5)
        natural = capped = 0
        for t in range(steps):
            a = _actions(rng, ref, n)
            pool.step(a)
            ref.step(a)
            assert np.array_equal(_bits(pool.staging), _bits(ref.staging)), t
            natural += int((ref.done == 1).sum())                       # (from the in-process run alone)
            capped += int(((ref.ended == 1) & (ref.done == 0)).sum())
        v = staging_views(pool.staging, n, ref.obs_dim)
        assert all(np.shares_memory(v[k], getattr(pool, k)) for k in v)
    ref.close()
    print(env_id, "done", natural, "capped", capped)
    assert natural >= want[0] and capped >= want[1]      # the kinds of episode end the case is there for


# ---------------------------------------------------------------------------- non-blocking form
def test_step_async_and_poll_hand_each_step_over_exactly_once():
    n, seed = 4, 3
    ref = HostVectorEnv("Pendulum-v0", n, seed=seed, max_episode_length=6)
    with ProcHostVectorEnv("Pendulum-v0", n, workers=2, seed=seed, max_episode_length=6, timeout=30.0) as pool:
        pool.reset()
        ref.reset()
        with pytest.raises(RuntimeError):
            pool.poll()                            # no step in flight
        rng = np.random.default_rng(2)
        falses = 0
        for t in range(10):
            a = _actions(rng, ref, n)
            pool.step_async(a)
            with pytest.raises(RuntimeError):
                pool.step_async(a)                 # a step is in flight
            t0 = time.perf_counter()
            got = pool.poll()                      # at once, whatever the workers are doing
            assert time.perf_counter() - t0 < 1.0
            deadline = time.monotonic() + 30.0
            while not got:
                falses += 1
                assert time.monotonic() < deadline, "the pool never finished its step"
                time.sleep(0.001)
                got = pool.poll()
            assert got is True
            with pytest.raises(RuntimeError):
                pool.poll()                        # ... and not a second time
            ref.step(a)
            assert np.array_equal(_bits(pool.staging), _bits(ref.staging)), t
        pool.step_async(_actions(rng, ref, n))
        pool.wait(10.0)                            # the bounded blocking form
        with pytest.raises(RuntimeError):
            pool.wait(1.0)
    ref.close()
    print("poll answered False", falses, "times")


# ---------------------------------------------------------------------------- failure
def test_a_raising_env_names_its_worker_and_breaks_the_pool():
    pool = ProcHostVectorEnv("CartPole-v0", 3, workers=2, seed=1, timeout=30.0,
                             factory="tests.proc_host_vector_fixtures:raises_third")
    try:
        assert pool.banks == [(0, 2), (2, 3)]
        pool.reset()
        a = np.zeros((3, 1), np.float32)
        pool.step(a)
        pool.step(a)
        with pytest.raises(RuntimeError, match=r"worker 1 \(envs \[2, 3\)\) raised") as ei:
            pool.step(a)                           # worker 1's env raises on its 3rd step
        assert "scripted env failure" in str(ei.value)
        for call in (lambda: pool.step(a), pool.reset, lambda: pool.step_async(a), pool.poll):
            with pytest.raises(RuntimeError, match="worker 1"):
                call()                             # the pool is broken
    finally:
        pool.close()
        pool.close()                               # idempotent
    assert all(not p.is_alive() for p in pool.processes)
    with pytest.raises(RuntimeError, match="closed"):
        pool.reset()


def test_bad_arguments_raise_before_any_process_starts():
    with pytest.raises(ValueError):
        ProcHostVectorEnv("CartPole-v0", 2, workers=3)
    with pytest.raises(ValueError):
        ProcHostVectorEnv("CartPole-v0", 2, workers=0)
    with pytest.raises(ValueError):
        ProcHostVectorEnv("CartPole-v0", 2, workers=1, factory="no_colon")
