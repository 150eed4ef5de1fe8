"""Host checks of ``engine/evaluation.py``: the conflating side-stream state machine every
asynchronous evaluator inherits, driven with fake stream and event objects through three tiny
subclasses shaped like the Atari, vector and AQL evaluators; the shared rollout buffers; and the
greedy-rollout front of the engines."""
import contextlib
import types

import pytest
import torch

from apex_amd.engine.evaluation import GreedyRollouts, RolloutBuffers, RolloutEvaluation, SideStreamEvaluation


class _Event:
    def __init__(self):
        self.done, self.records, self.syncs = True, 0, 0

    def record(self, *a):
        self.records += 1
        self.done = False  # in flight until the test lets it land

    def query(self):
        return self.done

    def synchronize(self):
        self.syncs += 1
        self.done = True


class _Stream:
    def __init__(self):
        self.waits = []

    def wait_event(self, ev):
        self.waits.append(ev)


def _fakes(log):
    @contextlib.contextmanager
    def ctx(stream):
        log.append("enter")
        yield
        log.append("exit")

    return dict(stream=_Stream(), event=_Event, stream_ctx=ctx)


class _AtariShaped(SideStreamEvaluation):
    """``launch(src, n_steps, tag)``; a result depends on the previous one (a running count), as
    ``AtariEvaluator``'s ``_seen`` does."""

    def __init__(self, log, **side):
        super().__init__("cpu", **side)
        self.log, self.weights, self.count = log, None, 0
        self.host = {"value": torch.zeros(1), "count": torch.zeros(1)}
        self._seen = 0

    def launch(self, src, n_steps, tag=None):
        def snapshot():
            self.log.append("snapshot")
            self.weights = float(src)

        def play():
            self.log.append("play")
            self.count += int(n_steps)
            self.host["value"].fill_(self.weights)
            self.host["count"].fill_(self.count)

        return self._launch(tag, snapshot, play)

    def _result(self):
        count = int(self.host["count"])
        new, self._seen = count - self._seen, count
        return {"value": float(self.host["value"]), "new": new}


class _Buffers(RolloutBuffers):
    def __init__(self, log, owner, n):
        super().__init__(n, "cpu")
        self.log, self.owner = log, owner

    def pinned(self):
        return {k: torch.zeros_like(getattr(self, k)) for k in self.KEYS}

    def launch(self, seed, max_steps):
        self.log.append("play")
        self.returns.fill_(self.owner.flat[0])
        self.lengths.fill_(max_steps)
        self.ended.fill_(seed)


class _Engine(GreedyRollouts):
    device = "cpu"
    cfg = types.SimpleNamespace(seed=3)
    limit = 9

    def __init__(self, log=None):
        self.log = [] if log is None else log
        self.steps = 0
        self.flat = torch.zeros(2)
        self.made = []

    _eval_steps = property(lambda self: self.steps)
    _eval_limit = property(lambda self: self.limit)

    def _make_rollout(self, n):
        self.made.append(n)
        return _Buffers(self.log, self, n)


class _VectorShaped(RolloutEvaluation):
    """``launch(seed, tag)``; the snapshot is the learner's copy into the evaluator's parameters."""

    def __init__(self, log, **side):
        self.log, self.flat = log, torch.zeros(2)
        super().__init__(_Engine(log), _Buffers(log, self, 2), 7, **side)

    def launch_value(self, value, tag):
        self.engine.flat.fill_(value)
        return self.launch(seed=5, tag=tag)

    def _snapshot(self):
        self.log.append("snapshot")
        self.flat.copy_(self.engine.flat)


class _AQLShaped(_VectorShaped):
    """As the vector one, the snapshot a flat copy out of the engine's learner."""

    def __init__(self, log, **side):
        super().__init__(log, **side)
        self.engine.learner = types.SimpleNamespace(flat=self.engine.flat, P=2)

    def _snapshot(self):
        self.log.append("snapshot")
        L = self.engine.learner
        self.flat[:L.P] = L.flat


def _atari(log):
    ev = _AtariShaped(log, **_fakes(log))
    return ev, (lambda value, tag: ev.launch(value, 4, tag=tag)), (lambda r: r["value"])


def _rollout(cls):
    def make(log):
        ev = cls(log, **_fakes(log))
        return ev, ev.launch_value, (lambda r: r["returns"][0])

    return make


SHAPES = {"atari": _atari, "vector": _rollout(_VectorShaped), "aql": _rollout(_AQLShaped)}
ACCEPTED = ["snapshot", "enter", "play", "exit"]


@pytest.fixture(params=sorted(SHAPES))
def shaped(request):
    log = []
    ev, launch, value = SHAPES[request.param](log)
    return ev, launch, value, log


def test_launch_order_and_one_record_per_accepted_launch(shaped):
    ev, launch, value, log = shaped
    assert ev.poll() is None and ev.wait() is None and ev.latest() is None and ev.latest(block=True) is None
    assert ev.results_landed.syncs == 0          # nothing launched: nothing to wait for
    assert launch(1.0, "a") is True
    # the snapshot on the current stream, the play inside the side stream's context
    assert log == ACCEPTED
    assert ev.stream.waits == [ev.snapshot_taken]
    assert ev.snapshot_taken.records == 1 and ev.results_landed.records == 1 and ev.launches == 1


def test_second_launch_while_pending_does_nothing(shaped):
    ev, launch, value, log = shaped
    assert launch(1.0, "a") is True
    assert launch(2.0, "b") is False
    assert log == ACCEPTED                       # neither snapshot nor play
    assert len(ev.stream.waits) == 1 and ev.launches == 1
    assert ev.snapshot_taken.records == 1 and ev.results_landed.records == 1
    assert ev.poll() is None                     # still in flight: nothing is delivered
    ev.results_landed.done = True
    got = ev.poll()
    assert got["tag"] == "a" and value(got) == 1.0   # the refused launch left the first one's result alone
    assert ev.poll() is None and ev.wait() is None


def test_landed_result_is_harvested_before_the_buffers_are_reused(shaped):
    ev, launch, value, log = shaped
    assert launch(1.0, "a") is True
    ev.results_landed.done = True                # "a" lands and is not polled
    assert launch(3.0, "c") is True              # harvests "a", then overwrites the pinned buffers
    assert log == ACCEPTED * 2
    ev.results_landed.done = True
    first, second = ev.poll(), ev.poll()
    assert (first["tag"], value(first)) == ("a", 1.0)       # oldest first, each exactly once
    assert (second["tag"], value(second)) == ("c", 3.0)
    assert list(first)[0] == "tag" and "tag" not in ev._result()
    assert ev.poll() is None and ev.wait() is None
    assert ev.snapshot_taken.records == 2 and ev.results_landed.records == 2 and len(ev.stream.waits) == 2
    assert ev.results_landed.syncs == 0 and ev.snapshot_taken.syncs == 0


def test_wait_blocks_on_the_results_event_only(shaped):
    ev, launch, value, log = shaped
    assert launch(4.0, "d") is True
    assert ev.poll() is None
    got = ev.wait()
    assert (got["tag"], value(got)) == ("d", 4.0)
    assert ev.results_landed.syncs == 1 and ev.snapshot_taken.syncs == 0
    assert ev.wait() is None and ev.results_landed.syncs == 1   # nothing in flight: no further sync
    # a landed result is handed over by wait() without a sync
    assert launch(5.0, "e") is True
    ev.results_landed.done = True
    assert launch(6.0, "f") is True
    assert ev.wait()["tag"] == "e" and ev.results_landed.syncs == 1
    assert ev.wait()["tag"] == "f" and ev.results_landed.syncs == 2
    assert ev.wait() is None


def test_latest_returns_the_newest_and_drops_older(shaped):
    ev, launch, value, log = shaped
    assert launch(1.0, "a") is True
    assert ev.latest() is None                   # in flight: latest() does not block
    assert ev.results_landed.syncs == 0
    ev.results_landed.done = True
    assert launch(2.0, "b") is True
    ev.results_landed.done = True
    got = ev.latest()
    assert (got["tag"], value(got)) == ("b", 2.0)
    assert ev.latest() is None and ev.poll() is None and ev.wait() is None   # "a" was dropped
    assert ev.results_landed.syncs == 0


def test_latest_block_waits_out_the_one_in_flight(shaped):
    ev, launch, value, log = shaped
    assert launch(1.0, "a") is True
    ev.results_landed.done = True
    assert launch(2.0, "b") is True              # "a" harvested, "b" in flight
    got = ev.latest(block=True)
    assert (got["tag"], value(got)) == ("b", 2.0) and ev.results_landed.syncs == 1
    assert ev.latest(block=True) is None and ev.results_landed.syncs == 1


def test_results_that_depend_on_harvest_order():
    """The Atari-shaped result counts what is new since the previous one: harvesting before the
    buffers are reused keeps every count."""
    log = []
    ev, launch, _ = _atari(log)
    for tag in "abc":
        assert launch(1.0, tag) is True
        ev.results_landed.done = True
    assert [(r["tag"], r["new"]) for r in iter(ev.poll, None)] == [("a", 4), ("b", 4), ("c", 4)]


def test_rollout_evaluation_plays_the_snapshot_with_the_engines_seed():
    log = []
    ev = _VectorShaped(log, **_fakes(log))
    ev.engine.flat.fill_(2.5)
    assert ev.launch(tag=1) is True              # default seed: the engine's, at launch time
    ev.engine.flat.fill_(9.0)                    # training goes on: the snapshot is what is played
    ev.engine.steps = 100
    res = ev.wait()
    want = 3 * 7919 + 0xE7A1
    assert res == {"tag": 1, "returns": [2.5, 2.5], "lengths": [7, 7], "ended": [want, want]}
    assert ev.launch(seed=6, tag=2) is True
    res = ev.wait()
    assert res["returns"] == [9.0, 9.0] and res["ended"] == [6, 6]


def test_rollout_buffers():
    ro = RolloutBuffers(3, "cpu")
    assert ro.n == 3 and ro.KEYS == ("returns", "lengths", "ended")
    assert [(getattr(ro, k).dtype, tuple(getattr(ro, k).shape)) for k in ro.KEYS] == [
        (torch.float32, (3,)), (torch.int32, (3,)), (torch.int32, (3,))]
    ro.returns.copy_(torch.tensor([1.0, 2.0, 3.0]))
    ro.lengths.fill_(5)
    host = {k: torch.zeros_like(getattr(ro, k)) for k in ro.KEYS}
    ro.copy_to(host)
    assert host["returns"].tolist() == [1.0, 2.0, 3.0] and host["lengths"].tolist() == [5, 5, 5]
    assert host["ended"].tolist() == [0, 0, 0]


def test_greedy_rollouts_seed_and_buffer_reuse():
    eng = _Engine()
    assert eng._eval_seed(None) == 3 * 7919 + 0xE7A1
    eng.steps = 41
    assert eng._eval_seed(None) == 3 * 7919 + 0xE7A1 + 41       # the engine's step counter
    assert eng._eval_seed(12) == 12
    assert eng._eval_seed(-1) == 0xFFFFFFFFFFFF and eng._eval_seed(1 << 48) == 0   # 48 bits
    eng.flat.fill_(1.5)
    assert eng.rollout_evaluate(2, seed=8) == [1.5, 1.5]
    assert eng._rollout.lengths.tolist() == [9, 9] and eng._rollout.ended.tolist() == [8, 8]   # the default limit
    first = eng._rollout
    assert eng.rollout_evaluate(2, seed=8, max_episode_steps=4) == [1.5, 1.5]
    assert eng._rollout is first and first.lengths.tolist() == [4, 4]   # same episode count: same buffers
    assert eng.rollout_evaluate(3) == [1.5, 1.5, 1.5]
    assert eng.made == [2, 3] and eng._rollout.ended.tolist() == [3 * 7919 + 0xE7A1 + 41] * 3


def test_the_evaluators_and_engines_share_the_base():
    from apex_amd.engine.aql import AQLEngine, AQLEvaluator, AQLRolloutBuffers
    from apex_amd.engine.aql_frame import AQLFrameEngine
    from apex_amd.engine.dqn import DQNFrameEngine
    from apex_amd.engine.evaluator import AtariEvaluator
    from apex_amd.engine.vector import VecRolloutBuffers, VectorApexEngine, VectorEvaluator

    for cls in (AtariEvaluator, VectorEvaluator, AQLEvaluator):
        assert issubclass(cls, SideStreamEvaluation), cls
        for name in ("_launch", "_harvest", "poll", "wait", "latest"):
            assert name not in vars(cls), (cls, name)
    for cls in (VecRolloutBuffers, AQLRolloutBuffers):
        assert issubclass(cls, RolloutBuffers), cls
    for cls in (VectorApexEngine, DQNFrameEngine, AQLEngine, AQLFrameEngine):
        assert issubclass(cls, GreedyRollouts), cls
        assert "_eval_seed" not in vars(cls) and "rollout_evaluate" not in vars(cls), cls
    assert DQNFrameEngine.evaluate is GreedyRollouts.rollout_evaluate
    assert AQLFrameEngine.evaluate is AQLEngine.evaluate
