"""Host checks of the host-env evaluator: the pinned free-running cases, the episode cap of the raw
vector envs, the pool's non-blocking ``poll_bank`` and the non-blocking driver with fake stream /
event / pool (the style of tests/test_evaluation_host.py)."""
import time

import numpy as np
import pytest

from apex_amd.engine.host_eval import EpisodeLedger, HostEnvEvaluation, WeightSets, eval_seed
from apex_amd.envs.core import make
from apex_amd.envs.preprocess import AtariPreprocess, PreprocessSpec
from apex_amd.envs.proc_vector import ProcRawAtariVector
from apex_amd.envs.raw_vector import RawAtariVector

from . import host_eval_fixtures as fx
from .host_env_util import Shortened
from .proc_vector_fixtures import short


# ---------------------------------------------------------------------------- pinned cases
@pytest.mark.parametrize("case", sorted(fx.CASES))
def test_pinned_cases_keep_their_gap_actions_and_dones(case):
    ok, g = fx.gap_ok(case)
    r = fx.host_greedy(case)
    print(case, "gap", g, "actions", sorted(set(r["actions"].ravel().tolist())), "dones", int(r["dones"].sum()))
    assert ok and g >= fx.GAP
    assert len(set(r["actions"].ravel().tolist())) >= 3
    assert int(r["dones"].sum()) >= 4
    assert len(r["episodes"]) == int(r["dones"].sum())


# ---------------------------------------------------------------------------- cap
def _short_envs(n, seed):
    # (lives of different lengths, so a cap of 5 agent steps cuts some episodes and not others)
    return [Shortened(make("SeaquestNoFrameskip-v4"), life_every=(19, 29, 37)[i % 3]) for i in range(n)]


def test_cap_equals_a_twin_reset_by_hand():
    n, cap, seed = 3, 5, 11
    spec = PreprocessSpec(clip_rewards=False)
    raw = RawAtariVector(_short_envs(n, seed), spec, max_episode_steps=cap)
    ref = AtariPreprocess(_short_envs(n, seed), spec)
    for p in (raw, ref):
        p.seed(seed)
        p.fixed_noops = [2 + i for i in range(n)]
    from .host_env_util import warp_plane

    out = np.zeros((n, 2) + raw.raw_shape, np.uint8)
    raw.reset(out)
    obs = ref.reset()
    for e in range(n):
        assert np.array_equal(warp_plane(out[e]), obs[e, 3].reshape(-1))
    rng = np.random.default_rng(3)
    length, capped, natural = np.zeros(n, np.int64), 0, 0
    for t in range(40):
        a = rng.integers(0, raw.n_actions, n)
        r, d = raw.step(a, out)
        o2, r2, d2, _ = ref.step(a)
        length += 1
        want = d2 | (length >= cap)
        assert np.array_equal(d, want), t
        assert np.array_equal(r, r2), t
        natural += int(d2.sum())
        capped += int((~d2 & want).sum())
        for e in range(n):
            plane = ref.reset_one(e)[3] if want[e] else o2[e, 3]
            assert np.array_equal(warp_plane(out[e]), plane.reshape(-1)), (t, e)
            if want[e]:
                length[e] = 0
    print("capped", capped, "natural", natural)
    assert capped >= 3 and natural >= 3   # both kinds of episode end were seen


def test_cap_zero_is_the_vector_without_the_argument():
    n, seed = 2, 4
    a_vec = RawAtariVector(_short_envs(n, seed))
    b_vec = RawAtariVector(_short_envs(n, seed), max_episode_steps=0)
    for p in (a_vec, b_vec):
        p.seed(seed)
    oa, ob = (np.zeros((n, 2) + a_vec.raw_shape, np.uint8) for _ in range(2))
    a_vec.reset(oa)
    b_vec.reset(ob)
    assert np.array_equal(oa, ob)
    rng = np.random.default_rng(0)
    for _ in range(30):
        a = rng.integers(0, a_vec.n_actions, n)
        ra, da = a_vec.step(a, oa)
        rb, db = b_vec.step(a, ob)
        assert np.array_equal(oa, ob) and np.array_equal(ra, rb) and np.array_equal(da, db)
    with pytest.raises(ValueError):
        RawAtariVector(_short_envs(1, 0), max_episode_steps=-1)


# ---------------------------------------------------------------------------- pool
def test_poll_bank_hands_every_bank_over_once_and_equals_the_in_process_vector():
    n, seed, cap = 4, 9, 6
    spec = PreprocessSpec()
    ref = RawAtariVector([short("PongNoFrameskip-v4") for _ in range(n)], spec, max_episode_steps=cap)
    ref.seed(seed)
    want = np.zeros((n, 2) + ref.raw_shape, np.uint8)
    with ProcRawAtariVector("PongNoFrameskip-v4", n, spec, workers=2, seed=seed, max_episode_steps=cap,
                            factory="tests.proc_vector_fixtures:short", timeout=30.0) as pool:
        pool.reset(pool.staging)
        ref.reset(want)
        assert np.array_equal(pool.staging, want)
        with pytest.raises(RuntimeError):
            pool.poll_bank()                       # no step in flight
        rng = np.random.default_rng(1)
        nones = 0
        for t in range(12):
            a = rng.integers(0, ref.n_actions, n)
            pool.step_async(a)
            t0 = time.perf_counter()
            first = pool.poll_bank()               # at once, whatever the workers are doing
            assert time.perf_counter() - t0 < 1.0
            seen, r, d = [], np.zeros(n), np.zeros(n, bool)
            got, deadline = first, time.monotonic() + 30.0
            while len(seen) < 2:
                if got is None:
                    nones += 1
                    assert time.monotonic() < deadline, "the pool never finished its step"
                    time.sleep(0.001)
                else:
                    b, rb, db = got
                    e0, e1 = pool.banks[b]
                    seen.append(b)
                    r[e0:e1], d[e0:e1] = rb, db
                if len(seen) < 2:
                    got = pool.poll_bank()
            assert sorted(seen) == [0, 1], t       # every bank exactly once per step
            with pytest.raises(RuntimeError):
                pool.poll_bank()                   # ... and not a second time
            rr, dd = ref.step(a, want)
            assert np.array_equal(r, rr) and np.array_equal(d, dd), t
            assert np.array_equal(pool.staging, want), t
    print("poll_bank answered None", nones, "times")


def test_poll_bank_returns_none_at_once_while_a_worker_steps():
    """Worker 1's emulator sleeps at the trigger action: bank 0 arrives, bank 1 is ``None`` at once."""
    from .proc_vector_fixtures import TRIGGER

    with ProcRawAtariVector("SeaquestNoFrameskip-v4", 2, PreprocessSpec(), workers=2, seed=3,
                            factory="tests.proc_vector_fixtures:sleeps", timeout=2.0) as pool:
        pool.reset(pool.staging)
        pool.step_async(np.array([0, TRIGGER]))
        deadline = time.monotonic() + 1.5
        got = None
        while got is None and time.monotonic() < deadline:
            got = pool.poll_bank()
        assert got is not None and got[0] == 0
        t0 = time.perf_counter()
        assert pool.poll_bank() is None            # worker 1 is still stepping
        assert time.perf_counter() - t0 < 0.5


def test_a_failure_common_to_all_workers_names_worker_zero_whatever_the_order():
    """Every worker's factory raises, worker 0's 0.3 s after the others': the error still names
    worker 0 (the lowest-numbered failed worker), with its own traceback."""
    with pytest.raises(RuntimeError, match=r"worker 0 \(envs \[0, 1\)\) raised") as ei:
        ProcRawAtariVector("PongNoFrameskip-v4", 3, workers=3, factory="tests.proc_blame_fixtures:all_fail_zero_last")
    assert "scripted start-up failure in worker 0" in str(ei.value)


# ---------------------------------------------------------------------------- ledger, weight sets
def test_ledger_hands_each_episode_over_once():
    led = EpisodeLedger(2, cap=3)
    led.observe([1.0, 2.0], [False, True], learn_step=7)
    led.observe([0.5, 1.0], [False, False], learn_step=8)
    led.observe([0.25, 1.0], [True, False], learn_step=9)
    assert led.poll() == [(2.0, 1, False, 7), (1.75, 3, True, 9)]
    assert led.poll() == []
    assert (led.episodes, led.capped, led.steps) == (2, 1, 3)
    led.observe([4.0, 0.0], [True, True], learn_step=10)
    assert led.poll() == [(4.0, 1, False, 10), (2.0, 3, True, 10)]


def test_weight_sets_conflate_and_never_write_a_set_in_use():
    ws = WeightSets(fx.FakeEvent)
    st = fx.FakeStream()
    copies = []
    assert ws.acquire(st) == 0 and st.waits == 0          # no refresh yet: set 0, nothing to wait for
    ws.release()
    ws.last_use[0].done = False                            # that act is in flight
    assert ws.refresh(copies.append) and copies == [1]     # set 1 was never read
    assert not ws.refresh(copies.append) and copies == [1]  # target 0: its last act has not completed
    assert ws.conflated == 1 and ws.cur == 1
    assert ws.acquire(st) == 1 and st.waits == 1           # the act waits for the copies once
    ws.release()
    assert ws.acquire(st) == 1 and st.waits == 1
    ws.release()
    assert not ws.refresh(copies.append)
    ws.last_use[0].done = True
    assert ws.refresh(copies.append) and copies == [1, 0]
    assert ws.acquire(st) == 0 and st.waits == 2 and ws.refreshes == 2


# ---------------------------------------------------------------------------- driver
class _FakePool:
    """Two banks; ``finish(b)`` makes bank b's answer available."""

    def __init__(self, n=4):
        self.banks = [(0, 2), (2, 4)]
        self.n = n
        self.staging = np.zeros((n, 2, 84, 84, 3), np.uint8)
        self.ready, self.pending = [], set()
        self.log = []
        self.t = 0
        self.closed = 0

    def __len__(self):
        return self.n

    def reset(self, out):
        assert out is self.staging
        self.log.append("reset")

    def step_async(self, actions):
        assert not self.pending and not self.ready
        self.pending = {0, 1}
        self.t += 1
        self.log.append("step_async")

    def finish(self, b):
        self.pending.discard(b)
        self.ready.append(b)

    def poll_bank(self):
        if not self.ready:
            assert self.pending, "no step in flight"
            return None
        b = self.ready.pop(0)
        e0, e1 = self.banks[b]
        done = np.zeros(e1 - e0, bool)
        done[0] = self.t % 2 == 0 and b == 1      # env 2 ends an episode every second step
        return b, np.full(e1 - e0, float(self.t)), done

    def wait_bank(self, timeout=None):
        raise AssertionError("a blocking wait on the pool")

    step = wait_bank

    def close(self):
        self.closed += 1


class _FakeEvaluator:
    def __init__(self, n=4):
        import torch

        self.stream = fx.FakeStream()
        self.acted = fx.FakeEvent()
        self.actions_host = torch.zeros(n, dtype=torch.int32)
        self.ledger = EpisodeLedger(n)
        self.weights = WeightSets(fx.FakeEvent)
        self.learn_step = 0
        self.log = []
        self.closed = 0

    def ship(self, reset):
        self.log.append(("ship", bool(reset)))

    def act(self):
        self.weights.acquire(self.stream)
        self.weights.release()
        self.log.append("act")
        self.acted.record()

    def took(self, r, d):
        self.ledger.observe(r, d, self.learn_step)

    def refresh(self, flat, net=None):
        return self.weights.refresh(lambda i: self.log.append(("copy", i)))

    def poll(self):
        return self.ledger.poll()

    def close(self):
        self.closed += 1


def test_driver_pumps_without_blocking_and_hands_episodes_over_once():
    ev, pool = _FakeEvaluator(), _FakePool()
    drv = HostEnvEvaluation(ev, pool, stream=ev.stream, event=fx.FakeEvent, stream_ctx=fx.fake_ctx)
    assert pool.log == ["reset"] and ev.log == [("ship", True), "act"]
    drv.acted.done = False
    drv.pump(learn_step=1)                         # the act has not landed: nothing happens
    assert pool.log == ["reset"]
    drv.acted.done = True
    drv.pump(learn_step=2)                         # half-step 1: actions landed -> step_async
    assert pool.log == ["reset", "step_async"] and len(ev.log) == 2
    drv.pump(learn_step=3)                         # no bank yet
    pool.finish(1)
    drv.pump(learn_step=4)                         # one bank of two: taken, still waiting
    assert len(ev.log) == 2
    pool.finish(0)
    drv.pump(learn_step=5)                         # half-step 2: all banks in -> ship + act
    assert ev.log[2:] == [("ship", False), "act"] and pool.log.count("step_async") == 1
    assert drv.poll() == []
    drv.pump(learn_step=6)                         # step 2 starts; env 2 ends its episode in it
    pool.finish(0)
    pool.finish(1)
    drv.pump(learn_step=7)
    assert drv.poll() == [(3.0, 2, False, 7)]      # 1.0 + 2.0 over two steps, stamped with the learner step
    assert drv.poll() == []                        # ... exactly once
    assert ev.stream.syncs == 0                    # (FakeEvent.synchronize / wait_bank raise: nothing ever blocked)


def test_driver_refresh_conflates_and_close_is_idempotent():
    ev, pool = _FakeEvaluator(), _FakePool()
    drv = HostEnvEvaluation(ev, pool, stream=ev.stream, event=fx.FakeEvent, stream_ctx=fx.fake_ctx)
    ev.weights.last_use[0].done = False                      # the first act (set 0) is in flight
    assert drv.refresh(None)                                 # set 1 was never read
    assert not drv.refresh(None) and not drv.refresh(None)   # set 0 is still read: conflated
    assert [x for x in ev.log if x[0] == "copy"] == [("copy", 1)]
    drv.pump()
    pool.finish(0)
    pool.finish(1)
    drv.pump()                                               # the next act reads set 1
    assert ev.weights.cur == 1 and ev.stream.waits == 1
    ev.weights.last_use[0].done = True
    assert drv.refresh(None)
    assert [x for x in ev.log if x[0] == "copy"] == [("copy", 1), ("copy", 0)]
    drv.close()
    drv.close()
    assert (ev.closed, pool.closed, ev.stream.syncs) == (1, 1, 1)
    drv.pump()                                               # a closed driver does nothing
    assert pool.log.count("step_async") == 1


def test_eval_seeds_are_disjoint_from_the_training_envs():
    assert eval_seed(1122) - 1122 >= 1_000_000
