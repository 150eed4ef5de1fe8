"""Host checks of the host-env AQL evaluator's non-blocking driver (``engine/aql_host_eval.py``)
with fake stream / events / pool (the style of tests/test_host_eval_host.py), and of its ledger."""
import numpy as np

from apex_amd.engine.aql_host_eval import AQLHostEvaluation, _Ledger
from apex_amd.engine.host_eval import WeightSets
from apex_amd.envs.host_vector import staging_views

from . import host_eval_fixtures as fx

N, OBS = 3, 2


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
        assert not self.inflight and actions.shape == (N, 1)
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
        self.actions_np = np.zeros((N, 1), np.float32)
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

    def refresh(self, flat):
        return self.weights.refresh(lambda i: self.log.append(("copy", i)))

    def poll(self):
        return self.ledger.poll()

    def close(self):
        self.closed += 1


def _driver():
    pool = _FakePool()
    ev = _FakeEvaluator(pool)
    return ev, pool, AQLHostEvaluation(ev, pool, stream=ev.stream, event=fx.FakeEvent, stream_ctx=fx.fake_ctx)


def test_driver_pumps_without_blocking_and_hands_episodes_over_once():
    ev, pool, drv = _driver()
    assert pool.log == ["reset"] and ev.log == ["ship", "act"] and drv.state == "acting"
    drv.acted.done = False
    drv.pump(learn_step=1)                         # the act has not landed: nothing happens
    assert pool.log == ["reset"] and drv.state == "acting" and len(ev.log) == 2
    drv.acted.done = True
    drv.pump(learn_step=2)                         # half-step 1: actions landed -> step_async
    assert pool.log == ["reset", "step_async"] and len(ev.log) == 2 and drv.state == "stepping"
    drv.pump(learn_step=3)                         # the block has not landed: nothing happens
    assert drv.state == "stepping" and len(ev.log) == 2
    pool.finish()
    drv.pump(learn_step=4)                         # half-step 2: block landed -> ship + act
    assert ev.log[2:] == ["ship", "act"] and pool.log.count("step_async") == 1 and drv.state == "acting"
    assert drv.poll() == []
    drv.pump(learn_step=5)                         # step 2 starts; env 1 ends its episode in it (done)
    pool.finish()
    drv.pump(learn_step=6)
    assert drv.poll() == [(3.0, 2, False, 6)]      # 1.0 + 2.0 over two steps, stamped with the learner step
    assert drv.poll() == []                        # ... exactly once
    for k in (7, 8, 9, 10):                        # steps 3 and 4; env 1 ends again, by the cap (done = 0)
        if drv.state == "stepping":
            pool.finish()
        drv.pump(learn_step=k)
    assert drv.poll() == [(7.0, 2, True, 10)] and drv.poll() == []
    assert (ev.ledger.episodes, ev.ledger.capped, ev.ledger.steps) == (2, 1, 4)
    assert ev.stream.syncs == 0                    # (FakeEvent.synchronize / pool.wait raise: nothing ever blocked)
    assert drv.pumps == 10


def test_driver_refresh_surfaces_the_weight_sets_refusal_and_close_is_idempotent():
    ev, pool, drv = _driver()
    ev.weights.last_use[0].done = False                      # the first act (set 0) is in flight
    assert drv.refresh(None) is True                         # set 1 was never read
    assert drv.refresh(None) is False and drv.refresh(None) is False   # set 0 is still read: refused
    assert [x for x in ev.log if x[0] == "copy"] == [("copy", 1)] and ev.weights.conflated == 2
    drv.pump()
    pool.finish()
    drv.pump()                                               # the next act reads set 1
    assert ev.weights.cur == 1 and ev.stream.waits == 1
    ev.weights.last_use[0].done = True
    assert drv.refresh(None) is True
    assert [x for x in ev.log if x[0] == "copy"] == [("copy", 1), ("copy", 0)]
    drv.close()
    drv.close()
    assert (ev.closed, pool.closed, ev.stream.syncs) == (1, 1, 1)
    drv.pump()                                               # a closed driver does nothing
    assert pool.log.count("step_async") == 1


def test_ledger_capped_means_ended_without_done():
    led = _Ledger(3)
    led.observe_block([1.0, 2.0, 3.0], [0, 1, 0], [0, 1, 1], learn_step=4)
    assert led.poll() == [(2.0, 1, False, 4), (3.0, 1, True, 4)]
    led.observe_block([1.0, 1.0, 1.0], [0, 0, 0], [1, 0, 0], learn_step=5)
    assert led.poll() == [(2.0, 2, True, 5)] and led.poll() == []
    assert (led.episodes, led.capped, led.steps) == (3, 2, 2)
