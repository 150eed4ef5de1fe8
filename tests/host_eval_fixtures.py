"""Pinned cases and the fp64 greedy host run shared by the host-evaluator tests (host self-checks
and GPU tests).

The free-running GPU comparisons (fused act against the stepwise act, both against the fp64 greedy
run on the ``AtariPreprocess`` twin) are only meaningful while every network picks the same greedy
action, so two (game, model) cases are pinned whose fp64 top-2 Q gap stays above
``atari_rollout_fixtures.GAP`` x max|Q| at every step.  ``gap_ok`` is asserted by the host test and
re-asserted (never skipped) by every GPU test that relies on equal actions.
"""
from __future__ import annotations

import functools

import numpy as np

from apex_amd.envs.preprocess import PreprocessSpec

from . import atari_rollout_fixtures as rf
from .host_env_util import twins

GAP = rf.GAP
CASES = {"seaquest": ("Seaquest", 18, 0), "pong": ("Pong", 6, 2)}   # name -> (game, actions, model seed)
N, SEED, LIFE_EVERY, STEPS = 3, 21, 37, 24
SPEC = PreprocessSpec(clip_rewards=False)   # the twin reports game points, as the raw vector does


def make_twins(case: str, n: int = N, cap: int = 0):
    """(RawAtariVector with the episode cap, AtariPreprocess twin) of a case."""
    raw, ref = twins(CASES[case][0], n, seed=SEED, spec=SPEC, life_every=LIFE_EVERY)
    raw.max_episode_steps = int(cap)
    return raw, ref


def model(case: str):
    _, A, ms = CASES[case]
    return rf.make_model(A, ms)


@functools.lru_cache(maxsize=None)
def host_greedy(case: str, steps: int = STEPS, cap: int = 0, n: int = N):
    """The fp64 greedy run of a case on the ``AtariPreprocess`` twin (``reset_one`` after every
    done, and by hand after ``cap`` agent steps): per step Q [steps, n, A], actions, raw rewards,
    dones, the relative top-2 gap, and the finished episodes (return, length, capped) in the
    order the evaluator's ledger reports them.  Cached; do not modify."""
    _, ref = make_twins(case, n)
    f = rf.q64_fn(model(case).double())
    obs = ref.reset()
    ret, length = np.zeros(n), np.zeros(n, np.int64)
    qs, acts, rews, dones, episodes = [], [], [], [], []
    for _ in range(steps):
        q = f(obs)
        a = q.argmax(1)
        obs, r, d, _ = ref.step(a)
        obs = np.array(obs)
        ret += r
        length += 1
        d = d | ((cap > 0) & (length >= cap))
        for e in np.flatnonzero(d):
            episodes.append((float(ret[e]), int(length[e]), bool(0 < cap <= length[e])))
            ret[e], length[e] = 0.0, 0
            obs[e] = ref.reset_one(e)
        qs.append(q)
        acts.append(a.astype(np.int32))
        rews.append(np.asarray(r, np.float64))
        dones.append(d.copy())
    q = np.stack(qs)
    top = np.sort(q, axis=2)
    gap = (top[:, :, -1] - top[:, :, -2]) / np.abs(q).max(axis=(1, 2))[:, None]
    out = {"q": q, "actions": np.stack(acts), "rewards": np.stack(rews), "dones": np.stack(dones), "gap": gap}
    for v in out.values():
        v.setflags(write=False)
    out["episodes"] = tuple(episodes)
    return out


def gap_ok(case: str, steps: int = STEPS, cap: int = 0) -> tuple[bool, float]:
    g = float(host_greedy(case, steps, cap)["gap"].min())
    return g >= GAP, g


# ---------------------------------------------------------------------------- fakes (driver tests)
class FakeEvent:
    """``torch.cuda.Event`` for host tests: ``done`` is what ``query()`` answers; a blocking wait
    is an error."""

    def __init__(self):
        self.done = True
        self.records = 0

    def record(self, stream=None):
        self.records += 1

    def query(self):
        return self.done

    def synchronize(self):
        raise AssertionError("a blocking wait on an event")

    wait = synchronize


class FakeStream:
    def __init__(self):
        self.waits = 0
        self.syncs = 0

    def wait_event(self, ev):
        self.waits += 1

    def synchronize(self):
        self.syncs += 1


class fake_ctx:
    def __init__(self, stream):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False
