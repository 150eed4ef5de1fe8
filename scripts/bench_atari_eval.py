#!/usr/bin/env python
"""Greedy evaluation of the Atari Ape-X engine: the stepwise evaluator (eager and as the
captured 100-step graph) against the one-launch rollout (``GPUEvaluator.rollout``), and what
each ``train.py --eval-mode`` costs training.

(a) ``--part eval``: ``--steps`` (1000) greedy steps of ``--envs`` (8) evaluator envs, 18 actions,
    three ways -- ``step()`` eager, ``run()`` over the captured 100-step graph, ``rollout()`` --
    device-synced before and after: median ms of ``--calls`` (5) calls after one warm-up.
(b) ``--part train``: the ``train.py`` loop for ``--iters`` (3000) learner steps with evaluation
    off, ``--eval-mode`` step / rollout / async at ``--eval-interval 50 --eval-steps 25``, and
    step / async with ``--eval-steps auto``.  The rate is the mean ``learner/BPS`` of the log
    lines after the first (``--bps_interval 500``).  The variants are repeated ``--reps`` (2) times
    in alternation; the table holds each one's median with its lowest and highest.

Every measurement runs in a process of its own (this driver never opens the GPU) under its own
time limit; a child that fails or runs out of time stops the script.  Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name -> (--eval-mode or None for evaluation off, --eval-steps)
VARIANTS = {"off": (None, "25"), "step": ("step", "25"), "rollout": ("rollout", "25"), "async": ("async", "25"),
            "step_auto": ("step", "auto"), "async_auto": ("async", "auto")}


def _median_ms(fn, calls, warmups=1):
    import torch

    for _ in range(warmups):
        fn()
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def child_eval(a):
    import torch

    from apex_amd.engine.evaluator import GPUEvaluator
    from apex_amd.models.dqn import DuelingDQN

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = DuelingDQN.from_shapes((4, 84, 84), 18).to(dev)

    def make():
        return GPUEvaluator(model, n_envs=a.envs, n_actions=18, device=dev, seed=5)

    n = a.steps
    ev = make()
    ms_roll = _median_ms(lambda: ev.rollout(n), a.calls)
    ev = make()
    ms_eager = _median_ms(lambda: ev.run(n), a.calls)
    ev = make()
    ev.capture(100)
    ms_graph = _median_ms(lambda: ev.run(n), a.calls)
    return {"envs": a.envs, "steps": n, "eager_ms": ms_eager, "graph_ms": ms_graph, "rollout_ms": ms_roll,
            "rollout_us_per_step": 1e3 * ms_roll / n, "rollout_vs_graph": ms_graph / ms_roll,
            "rollout_vs_eager": ms_eager / ms_roll}


def child_train(a):
    from apex_amd import train

    mode, steps = VARIANTS[a.variant]
    extra = ["--eval-envs", "0"] if mode is None else ["--eval-envs", str(a.envs), "--eval-interval", "50",
                                                       "--eval-steps", steps, "--eval-mode", mode]
    buf = io.StringIO()
    with tempfile.TemporaryDirectory() as d:
        argv = ["--n-envs", "256", "--replay_buffer_size", "131072", "--threshold_size", "8192",
                "--bps_interval", "500", "--save_interval", "0", "--max-step", str(a.iters), "--no-tb", "--save-path", os.path.join(d, "m.pth"),
                *extra]
        with contextlib.redirect_stdout(buf):
            rc = train.main(argv)
    assert rc == 0
    bps = [float(x) for x in re.findall(r"learner/BPS=(\S+)", buf.getvalue())]
    episodes = re.findall(r"evaluator/episodes=(\S+)", buf.getvalue())
    chunks = re.findall(r"evaluator/chunks=(\S+)", buf.getvalue())  # async: chunks started of iters / 50
    return {"variant": a.variant, "learner_steps_per_s": statistics.mean(bps[1:] or bps), "log_lines": len(bps),
            "evaluator_episodes": float(episodes[-1]) if episodes else 0.0,
            "async_chunks": float(chunks[-1]) if chunks else None}


def _run_child(a, limit, *extra):
    """One measurement in a fresh process under its own time limit; a failure stops the script."""
    cmd = [sys.executable, os.path.abspath(__file__), "--envs", str(a.envs), "--steps", str(a.steps), "--calls",
           str(a.calls), "--iters", str(a.iters), *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {extra} failed with {p.returncode}: stopping")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "eval", "train"])
    ap.add_argument("--child", default=None, choices=["eval", "train"])
    ap.add_argument("--variant", default="off", choices=sorted(VARIANTS))
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_eval(a) if a.child == "eval" else child_train(a)), flush=True)
        return
    out = {}
    if a.part in ("all", "eval"):
        out["eval"] = _run_child(a, a.child_timeout, "--child", "eval")
        out["rollout_faster_than_graph"] = out["eval"]["rollout_vs_graph"] > 1
    if a.part in ("all", "train"):
        rates = {v: [] for v in VARIANTS}
        last = {}
        for _ in range(a.reps):
            for v in VARIANTS:  # alternated: every variant sees the same drift of the box
                last[v] = _run_child(a, a.child_timeout, "--child", "train", "--variant", v)
                rates[v].append(last[v]["learner_steps_per_s"])
                print(json.dumps(last[v]), file=sys.stderr, flush=True)
        med = {v: statistics.median(r) for v, r in rates.items()}
        out["train"] = [{"variant": v, "eval_mode": VARIANTS[v][0], "eval_steps": VARIANTS[v][1], "iters": a.iters,
                         "learner_steps_per_s": med[v], "min": min(r), "max": max(r), "of_no_eval": med[v] / med["off"],
                         "evaluator_episodes": last[v]["evaluator_episodes"], "async_chunks": last[v]["async_chunks"]}
                        for v, r in rates.items()]
        out["async_meets_0.90"] = med["async"] / med["off"] >= 0.90
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
