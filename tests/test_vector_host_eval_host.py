"""Host checks of the host-env vector evaluator (``engine/vector_host_eval.py``): the command line's
rules, the non-blocking driver with fake stream / events / pool (the style of
tests/test_aql_host_eval_host.py), and the ledger's ``capped``."""
import numpy as np
import pytest

from apex_amd.engine.host_eval import WeightSets
from apex_amd.engine.vector_host_eval import MAX_ENVS, VectorHostEvaluation, _Ledger, make_pool
from apex_amd.envs.host_vector import staging_views

from . import host_eval_fixtures as fx

N, OBS = 3, 2
BASE = ["--host-envs", "--env", "CartPole-v0", "--envs", "4", "--eval-envs", "2", "--eval-workers", "1",
        "--eval-interval", "2"]


# ------------------------------------------------------------------ the command line
@pytest.mark.parametrize("argv", [
    ["--env", "CartPole-v0", "--eval-envs", "2", "--eval-interval", "2"],                      # no --host-envs
    ["--host-envs", "--eval-envs", "2", "--eval-interval", "0"],
    ["--host-envs", "--eval-envs", "2"],                                                       # (the default interval is 0)
    ["--host-envs", "--eval-envs", "65", "--eval-interval", "2"],
    ["--host-envs", "--eval-envs", "-1", "--eval-interval", "2"],
    ["--host-envs", "--eval-envs", "2", "--eval-interval", "2", "--eval-workers", "0"],
    ["--host-envs", "--eval-envs", "2", "--eval-interval", "2", "--eval-workers", "3"],
    ["--host-envs", "--eval-workers", "1"],                                                    # --eval-workers alone
    ["--eval-workers", "1"],
    ["--host-envs", "--eval-envs", "2", "--eval-interval", "2", "--eval-kernel", "graph"],
    ["--host-envs", "--eval-envs", "2", "--eval-interval", "2", "--eval-mode", "async"]])      # the --eval-mode rule stays
def test_cli_parser_errors(argv):
    from apex_amd import train_vector

    with pytest.raises(SystemExit) as e:
        train_vector.parser().parse_args(argv)
    assert e.value.code == 2


def test_cli_parser_defaults():
    from apex_amd import train_vector

    p = train_vector.parser
    ok = p().parse_args(BASE)
    assert (ok.eval_envs, ok.eval_workers, ok.eval_interval, ok.eval_kernel) == (2, 1, 2, "fused")
    for n in (1, 2, 5, 64):
        a = p().parse_args(["--host-envs", "--eval-envs", str(n), "--eval-interval", "1"])
        assert a.eval_workers == min(2, n)
    assert p().parse_args(BASE + ["--eval-kernel", "step"]).eval_kernel == "step"
    # without the new flags nothing changes: off, and the blocking cadence is as it was
    a = p().parse_args(["--host-envs", "--eval-interval", "30"])
    assert (a.eval_envs, a.eval_workers, a.eval_interval) == (0, None, 30)
    a = p().parse_args([])
    assert (a.eval_envs, a.eval_workers) == (0, None)
    assert MAX_ENVS == 64 and callable(make_pool)


# ------------------------------------------------------------------ the pump
class _FakePool:
    """The pool's non-blocking protocol; ``finish()`` lands the step in flight.  Env 1 ends an
    episode every second step: at step 2 by ``done``, at step 4 by the length cap."""

    def __init__(self):
        self.staging = np.zeros(N * (2 * OBS + 3), np.float32)
        self.v = staging_views(self.staging, N, OBS)
        self.inflight = self.landed = False
        self.log = []
        self.t = 0
        self.closed = 0

    def __len__(self):
        return N

    def reset(self):
        self.log.append("reset")

    def step_async(self, actions):
        assert not self.inflight and actions.shape == (N,) and actions.dtype == np.int32
        self.inflight, self.landed = True, False
        self.t += 1
        self.log.append("step_async")

    def finish(self):
        assert self.inflight
        self.v["reward"][:] = float(self.t)
        self.v["ended"][:] = 0.0
        self.v["done"][:] = 0.0
        if self.t % 2 == 0:
            self.v["ended"][1] = 1.0
            self.v["done"][1] = 1.0 if self.t % 4 == 2 else 0.0
        self.landed = True

    def poll(self):
        assert self.inflight, "no step in flight"
        if not self.landed:
            return False
        self.inflight = False
        return True

    def wait(self, timeout=None):
        raise AssertionError("a blocking wait on the pool")

    step = wait

    def close(self):
        self.closed += 1


class _FakeEvaluator:
    """The evaluator's host half over the fake pool's block; the device half is a log."""

    def __init__(self, pool):
        self.stream = fx.FakeStream()
        self.acted = fx.FakeEvent()
        self.actions_np = np.zeros(N, np.int32)
        self.ledger = _Ledger(N)
        self.weights = WeightSets(fx.FakeEvent)
        self.v = pool.v
        self.learn_step = 0
        self.log = []
        self.closed = 0

    def ship(self):
        self.log.append("ship")

    def act(self):
        self.weights.acquire(self.stream)
        self.weights.release()
        self.log.append("act")
        self.acted.record()

    def took(self):
        self.ledger.observe_block(self.v["reward"], self.v["done"], self.v["ended"], self.learn_step)

    def refresh(self):
        return self.weights.refresh(lambda i: self.log.append(("copy", i)))

    def poll(self):
        return self.ledger.poll()

    def close(self):
        self.closed += 1


def _driver():
    pool = _FakePool()
    ev = _FakeEvaluator(pool)
    return ev, pool, VectorHostEvaluation(ev, pool, stream=ev.stream, event=fx.FakeEvent, stream_ctx=fx.fake_ctx)


def test_driver_does_at_most_one_half_step_per_pump_and_never_waits():
    ev, pool, drv = _driver()
    assert pool.log == ["reset"] and ev.log == ["ship", "act"] and drv.state == "acting"
    drv.acted.done = False
    drv.pump(learn_step=1)                         # the act has not landed: nothing happens
    assert pool.log == ["reset"] and drv.state == "acting" and len(ev.log) == 2
    drv.acted.done = True
    states = []
    for k in range(2, 18):                         # every pump: at most one half-step, the state alternates
        before = (pool.log.count("step_async"), ev.log.count("act"))
        if drv.state == "stepping" and k % 3 == 0:
            pool.finish()
        drv.pump(learn_step=k)
        after = (pool.log.count("step_async"), ev.log.count("act"))
        assert (after[0] - before[0]) + (after[1] - before[1]) <= 1
        assert ev.log.count("ship") == ev.log.count("act")
        assert after[0] in (after[1], after[1] - 1)                           # act k+1 only after step k landed
        assert drv.state == ("acting" if after[0] == after[1] - 1 else "stepping")
        states.append(drv.state)
    assert "acting" in states and "stepping" in states
    assert ev.ledger.steps >= 4 and ev.ledger.steps == ev.log.count("act") - 1
    assert ev.stream.syncs == 0                    # (FakeEvent.synchronize / pool.wait raise: nothing ever blocked)
    assert drv.pumps == 17


def test_driver_hands_episodes_over_once_with_capped_and_the_learn_step():
    ev, pool, drv = _driver()
    got = []
    k = 0
    while ev.ledger.steps < 4:
        k += 1
        if drv.state == "stepping":
            pool.finish()
        drv.pump(learn_step=k)
        got += drv.poll()
    # env 1: steps 1 + 2 end by done, steps 3 + 4 by the cap (ended with done = 0)
    assert [e[:3] for e in got] == [(3.0, 2, False), (7.0, 2, True)]
    assert got[0][3] < got[1][3] <= k and drv.poll() == []
    assert (ev.ledger.episodes, ev.ledger.capped, ev.ledger.steps) == (2, 1, 4)


def test_driver_refresh_surfaces_the_weight_sets_refusal_and_close_is_idempotent():
    ev, pool, drv = _driver()
    ev.weights.last_use[0].done = False                      # the first act (set 0) is in flight
    assert drv.refresh() is True                             # set 1 was never read
    assert drv.refresh() is False and drv.refresh() is False   # set 0 is still read: refused
    assert [x for x in ev.log if x[0] == "copy"] == [("copy", 1)] and ev.weights.conflated == 2
    drv.pump()
    pool.finish()
    drv.pump()                                               # the next act reads set 1
    assert ev.weights.cur == 1 and ev.stream.waits == 1
    ev.weights.last_use[0].done = True
    assert drv.refresh() is True
    assert [x for x in ev.log if x[0] == "copy"] == [("copy", 1), ("copy", 0)]
    drv.close()
    drv.close()
    assert (ev.closed, pool.closed, ev.stream.syncs) == (1, 1, 1)
    n_act, n_step, pumps = ev.log.count("act"), pool.log.count("step_async"), drv.pumps
    drv.pump()                                               # a closed driver does nothing
    assert (ev.log.count("act"), pool.log.count("step_async"), drv.pumps) == (n_act, n_step, pumps)


# ------------------------------------------------------------------ the ledger
def test_ledger_capped_means_ended_without_done():
    led = _Ledger(3)
    led.observe_block([1.0, 2.0, 3.0], [0, 1, 0], [0, 1, 1], learn_step=4)
    assert led.poll() == [(2.0, 1, False, 4), (3.0, 1, True, 4)]
    led.observe_block([1.0, 1.0, 1.0], [0, 0, 0], [1, 0, 0], learn_step=5)
    assert led.poll() == [(2.0, 2, True, 5)] and led.poll() == []
    led.observe_block([0.5, 0.25, -1.0], [0, 0, 0], [0, 0, 0], learn_step=6)
    led.observe_block([0.5, 0.25, -1.0], [1, 1, 0], [1, 1, 0], learn_step=7)
    assert led.poll() == [(1.0, 2, False, 7), (1.5, 3, False, 7)]
    assert (led.episodes, led.capped, led.steps) == (5, 2, 4)
