"""Host checks of the one-launch Atari evaluator: the fixture's Q gaps, the CLI switch, and the
conflation logic of ``AtariEvaluator`` against a fake evaluator and fake events."""
import contextlib

import numpy as np
import pytest
import torch

from . import atari_rollout_fixtures as fx


@pytest.mark.parametrize("case", sorted(fx.CASES))
def test_fixture_gaps(case):
    """Every step of the fp64 host rollout keeps the top-2 Q gap >= 1e-3 x max|Q| (2.5x what two
    in-bound fp32 kernels may disagree by), takes several distinct actions and meets the time
    limit three times per env -- what the free-running GPU comparisons rely on."""
    ok, g = fx.gap_ok(case)
    r = fx.host_rollout(case)
    print(f"{case}: smallest relative top-2 gap {g:.3e}, distinct actions {len(np.unique(r['actions']))}, "
          f"dones {int(r['dones'].sum())}")
    assert ok, g
    assert r["q"].shape == (fx.STEPS, fx.E, fx.CASES[case][0])
    assert len(np.unique(r["actions"])) >= 3
    assert int(r["dones"].sum()) >= 3 * fx.E
    for n_envs in (1, 3):
        for steps in (1, 5, 24):
            assert fx.gap_ok(case, n_envs, steps)[0]


def test_parser_eval_mode():
    from apex_amd import train

    p = train.parser()
    assert p.parse_args([]).eval_mode == "step"
    for mode in ("step", "rollout", "async"):
        assert p.parse_args(["--eval-mode", mode]).eval_mode == mode
    with pytest.raises(SystemExit):
        p.parse_args(["--eval-mode", "graph"])


def test_ring_episodes_order_and_overflow():
    from apex_amd.engine.evaluator import GPUEvaluator

    R = 4
    ring = torch.zeros(2, R, 2)
    for i in range(6):          # env 0 finished episodes 0..5: the ring keeps 2..5
        ring[0, i % R] = torch.tensor([10.0 * i, float(i)])
    ring[1, 0] = torch.tensor([7.0, 3.0])
    got = GPUEvaluator.ring_episodes(ring, torch.tensor([6.0, 1.0]), torch.tensor([0.0, 0.0]))
    assert got == [(20.0, 2.0), (30.0, 3.0), (40.0, 4.0), (50.0, 5.0), (7.0, 3.0)]
    assert GPUEvaluator.ring_episodes(ring, torch.tensor([6.0, 1.0]), torch.tensor([5.0, 1.0])) == [(50.0, 5.0)]


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
        self.waits = 0

    def wait_event(self, ev):
        self.waits += 1


class _FakeEvaluator:
    """Each rollout of n steps ends one episode per env of return = the snapshot's value."""
    E, RING = 2, 16
    device = "cpu"

    def __init__(self):
        self.calls = []
        self.weights = None
        self.count = 0
        self.ring = torch.zeros(self.E, self.RING, 2)

    def snapshot(self, flat, net):
        self.calls.append(("snapshot", float(flat[0])))
        self.weights = float(flat[0])

    def rollout(self, n):
        self.calls.append(("rollout", n))
        self.ring[:, self.count % self.RING] = torch.tensor([self.weights, float(n)])
        self.count += 1

    def host_results(self):
        return {"ring": torch.zeros(self.E, self.RING, 2), "counts": torch.zeros(self.E),
                "running": torch.zeros(self.E, 2)}

    def copy_results(self, host):
        self.calls.append(("copy",))
        host["ring"].copy_(self.ring)
        host["counts"].fill_(self.count)
        host["running"].fill_(self.weights)


def test_async_evaluator_conflates_and_delivers_once():
    from apex_amd.engine.evaluator import AtariEvaluator

    ev = _FakeEvaluator()
    stream = _Stream()
    ae = AtariEvaluator(ev, stream=stream, event=_Event, stream_ctx=lambda s: contextlib.nullcontext())
    assert ae.poll() is None and ae.wait() is None
    assert ae.launch(torch.tensor([1.0]), None, 11, tag="a") is True
    n_calls = len(ev.calls)
    assert ev.calls == [("snapshot", 1.0), ("rollout", 11), ("copy",)] and stream.waits == 1
    # in flight: a second launch does nothing at all, nothing is delivered
    assert ae.launch(torch.tensor([2.0]), None, 12, tag="b") is False
    assert len(ev.calls) == n_calls and stream.waits == 1 and ev.weights == 1.0
    assert ae.snapshot_taken.records == 1 and ae.results_landed.records == 1
    assert ae.poll() is None
    ae.results_landed.done = True   # the first lands
    assert ae.launch(torch.tensor([3.0]), None, 13, tag="c") is True   # harvests "a" before reusing the buffers
    ae.results_landed.done = True
    first, second = ae.poll(), ae.poll()
    assert first["tag"] == "a" and first["episodes"] == [(1.0, 11.0), (1.0, 11.0)] and first["total_episodes"] == 2
    assert first["running_return"] == [1.0, 1.0]
    assert second["tag"] == "c" and second["episodes"] == [(3.0, 13.0), (3.0, 13.0)]
    assert second["total_episodes"] == 4
    assert ae.poll() is None and ae.wait() is None     # each exactly once
    # wait() blocks on the results event only
    assert ae.launch(torch.tensor([4.0]), None, 14, tag="d") is True
    assert ae.poll() is None
    got = ae.wait()
    assert got["tag"] == "d" and ae.results_landed.syncs == 1 and got["episodes"] == [(4.0, 14.0), (4.0, 14.0)]
    assert ae.wait() is None and ae.launches == 3
