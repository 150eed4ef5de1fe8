#!/usr/bin/env python
"""Greedy evaluation of the vector engine: the stepwise ``evaluate()`` against the one-launch
``rollout_evaluate()``, and what each ``train_vector --eval-mode`` costs training.  One process,
one box.

(a) ``--part eval``: wall time of ``evaluate(10)`` and ``rollout_evaluate(10)`` with the same
    hand-set policy in the online weights (``tests/vector_policies.py``): the balancing policy on
    CartPole-v0 (200-step episodes) and CartPole-v1 (500), the pump policy on MountainCar-v0.
    Median of ``--calls`` (20) calls after ``--warmups`` (3); the returns of both are compared.
(b) ``--part train``: ``train_vector`` on CartPole-v0, 256 envs, lr 2.5e-4, ``--train-steps``
    (20k) steps, a log line every 1000: no evaluation, then ``--eval-interval 1000`` in each of
    the three modes.  The rate is steps / wall time from the end of graph capture to the end of
    ``train()``, device idle.  The four runs are repeated ``--reps`` (3) times in alternation; the
    table holds each mode's median rate and its lowest and highest, so a difference can be read
    against the spread of one mode.

``--part rollout`` only issues the rollout calls of (a) (a rocprofv3 --kernel-trace target).
Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POLICIES = (("CartPole-v0", "balance", 1, 0.02), ("CartPole-v1", "balance", 1, 0.02),
            ("MountainCar-v0", "pump", 20, 0.1))


def _median_ms(fn, calls, warmups):
    import torch

    for _ in range(warmups):
        out = fn()
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()  # (returns a host list: the read-back is inside)
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts), out


def part_eval(a, rollout_only=False):
    from apex_amd.engine.vector import VectorApexEngine, VectorEngineConfig
    from tests import vector_policies as vp

    rows = []
    for env_id, recipe, seed, noise in POLICIES:
        eng = VectorApexEngine(VectorEngineConfig(env_id=env_id, n_envs=64, replay_capacity=8192), "cuda:0")
        vp.load_policy(eng, vp.make_policy(env_id, recipe, seed, noise))
        row = {"env": env_id, "policy": recipe, "episodes": a.episodes}
        ms_r, ret_r = _median_ms(lambda: eng.rollout_evaluate(a.episodes, seed=5), a.calls, a.warmups)
        row.update(rollout_ms=ms_r, mean_return=sum(ret_r) / len(ret_r))
        if not rollout_only:
            ms_s, ret_s = _median_ms(lambda: eng.evaluate(a.episodes, seed=5), a.calls, a.warmups)
            row.update(step_ms=ms_s, speedup=ms_s / ms_r, same_returns=ret_s == ret_r)
        rows.append(row)
    return rows


def part_train(a):
    import torch

    from apex_amd import train_vector
    from apex_amd.engine.vector import VectorApexEngine

    marks = []
    capture = VectorApexEngine.capture

    def timed_capture(self, *args, **kw):
        capture(self, *args, **kw)
        marks.append(time.perf_counter())

    VectorApexEngine.capture = timed_capture
    modes = (("none", []), ("step", ["--eval-interval", "1000", "--eval-mode", "step"]),
             ("rollout", ["--eval-interval", "1000", "--eval-mode", "rollout"]),
             ("async", ["--eval-interval", "1000", "--eval-mode", "async"]))
    rates = {name: [] for name, _ in modes}
    last = {}
    try:
        for _ in range(a.reps):
            for name, extra in modes:
                with tempfile.TemporaryDirectory() as d:
                    args = train_vector.parser().parse_args(
                        ["--env", "CartPole-v0", "--envs", "256", "--lr", "2.5e-4", "--max-step", str(a.train_steps),
                         "--log-interval", "1000", "--save-interval", str(10 ** 9), "--save-dir", d, *extra])
                    with contextlib.redirect_stdout(io.StringIO()):
                        last[name] = train_vector.train(args)
                    torch.cuda.synchronize()
                    rates[name].append(a.train_steps / (time.perf_counter() - marks[-1]))
    finally:
        VectorApexEngine.capture = capture
    med = {name: statistics.median(v) for name, v in rates.items()}
    rows = [{"eval": name, "sgd_steps_per_s": med[name], "min": min(v), "max": max(v),
             "of_no_eval": med[name] / med["none"], "greedy_mean_return": last[name].get("greedy_mean_return"),
             "greedy_step": last[name].get("greedy_step")} for name, v in rates.items()]
    return rows, abs(med["none"] - med["async"]) < abs(med["none"] - med["step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "eval", "train", "rollout"])
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    out = {}
    if a.part in ("all", "eval", "rollout"):
        out["eval"] = part_eval(a, rollout_only=a.part == "rollout")
        if a.part != "rollout":
            out["rollout_faster_everywhere"] = all(r["speedup"] > 1 for r in out["eval"])
    if a.part in ("all", "train"):
        out["train"], out["async_nearer_no_eval_than_step"] = part_train(a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
