#!/usr/bin/env python
"""Greedy evaluation of the GPU AQL engine: the host evaluator (``train_aql.greedy_eval``), the
stepwise device evaluator (``AQLEngine.evaluate``) and the one-launch rollout
(``AQLEngine.rollout_evaluate``), and what each ``train_aql --eval-mode`` costs training.

(a) ``--part eval``: per env (Pendulum-v0, CartPole-v0; the default 51 candidates, 10 episodes)
    the wall time of one evaluation by each of the three, device-synced before the clock
    starts, the read-back inside: median of ``--calls`` (10) calls after ``--warmups`` (2); the
    host evaluator, seconds per call on Pendulum, gets ``--host-calls`` (3) after one.  The
    stepwise and rollout returns are compared (they must be equal).
(b) ``--part train``: ``train_aql`` on ``--train-env`` (Pendulum-v0), 256 envs, ``--iters``
    (2000) iterations, ``--eval-interval`` (500), under ``--eval-mode`` host / rollout / async
    and with evaluation off.  The rate is iterations / wall time from the end of graph capture
    to the end of ``train()``, device idle.  The four variants are repeated ``--reps`` (3) times
    in alternation; the table holds each one's median rate with its lowest and highest.

Every measurement runs in a process of its own (this driver never opens the GPU) under its own
time limit; a child that fails or runs out of time stops the script.  Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = ("Pendulum-v0", "CartPole-v0")
MODES = ("none", "host", "rollout", "async")


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


def child_eval(a):
    from apex_amd import train_aql
    from apex_amd.engine.aql import AQLEngine, AQLEngineConfig

    eng = AQLEngine(AQLEngineConfig(env_id=a.env, n_envs=64, capacity=8192, use_graphs=False), "cuda:0")
    n = a.episodes
    ms_r, ret_r = _median_ms(lambda: eng.rollout_evaluate(n, seed=5), a.calls, a.warmups)
    ms_s, ret_s = _median_ms(lambda: eng.evaluate(n, seed=5), a.calls, a.warmups)
    ms_h, ret_h = _median_ms(lambda: train_aql.greedy_eval(eng, n, seed=5), a.host_calls, 1)
    steps = sum(eng._rollout.lengths.tolist())
    longest = max(eng._rollout.lengths.tolist())
    return {"env": a.env, "episodes": n, "candidates": eng.T, "host_ms": ms_h, "step_ms": ms_s, "rollout_ms": ms_r,
            "rollout_vs_step": ms_s / ms_r, "rollout_vs_host": ms_h / ms_r, "same_returns": ret_s == ret_r,
            "env_steps": steps, "longest_episode": longest, "rollout_us_per_step": 1e3 * ms_r / longest,
            "mean_return_device": sum(ret_r) / n, "mean_return_host": sum(ret_h) / n}


def child_train(a):
    import torch

    from apex_amd import train_aql
    from apex_amd.engine.aql import AQLEngine

    marks = []
    capture = AQLEngine.capture

    def timed_capture(self, *args, **kw):
        capture(self, *args, **kw)
        marks.append(time.perf_counter())

    AQLEngine.capture = timed_capture
    extra = [] if a.mode == "none" else ["--eval-interval", str(a.eval_interval), "--eval-mode", a.mode,
                                        "--eval-episodes", str(a.episodes)]
    with tempfile.TemporaryDirectory() as d:
        args = train_aql.parser().parse_args(
            ["--env", a.train_env, "--n-envs", "256", "--capacity", "1000000", "--max-step", str(a.iters), "--no-tb",
             "--log-interval", str(a.eval_interval), "--save-interval", str(10 ** 9), "--save-dir", d, *extra])
        with contextlib.redirect_stdout(io.StringIO()):
            last = train_aql.train(args)
        torch.cuda.synchronize()
        dt = time.perf_counter() - marks[-1]
    return {"mode": a.mode, "iterations_per_s": a.iters / dt, "sgd_steps_per_s": last["learner_steps"] / dt,
            "greedy_mean_return": last.get("greedy_mean_return"), "greedy_iteration": last.get("greedy_iteration")}


def _run_child(a, limit, *extra):
    """One measurement in a fresh process under its own time limit; a failure stops the script."""
    cmd = [sys.executable, os.path.abspath(__file__), "--episodes", str(a.episodes), "--calls", str(a.calls),
           "--warmups", str(a.warmups), "--host-calls", str(a.host_calls), "--iters", str(a.iters),
           "--eval-interval", str(a.eval_interval), "--train-env", a.train_env, *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {extra} failed with {p.returncode}: stopping")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "eval", "train"])
    ap.add_argument("--child", default=None, choices=["eval", "train"])
    ap.add_argument("--env", default=ENVS[0])
    ap.add_argument("--mode", default="none", choices=MODES)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--train-env", default="Pendulum-v0")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--eval-interval", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_eval(a) if a.child == "eval" else child_train(a)), flush=True)
        return
    out = {}
    if a.part in ("all", "eval"):
        out["eval"] = [_run_child(a, a.child_timeout, "--child", "eval", "--env", e) for e in ENVS]
        out["rollout_faster_than_stepwise"] = all(r["rollout_vs_step"] > 1 for r in out["eval"])
    if a.part in ("all", "train"):
        rates = {m: [] for m in MODES}
        last = {}
        for _ in range(a.reps):
            for m in MODES:  # alternated: every variant sees the same drift of the box
                last[m] = _run_child(a, a.child_timeout, "--child", "train", "--mode", m)
                rates[m].append(last[m]["iterations_per_s"])
        med = {m: statistics.median(v) for m, v in rates.items()}
        out["train"] = [{"eval": m, "env": a.train_env, "iterations": a.iters, "eval_interval": a.eval_interval,
                         "iterations_per_s": med[m], "min": min(v), "max": max(v), "of_no_eval": med[m] / med["none"],
                         "greedy_mean_return": last[m]["greedy_mean_return"]} for m, v in rates.items()]
        out["rollout_over_host"] = med["rollout"] / med["host"]
        out["async_over_rollout"] = med["async"] / med["rollout"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
