#!/usr/bin/env python
"""Host-env AQL evaluator (``engine/aql_host_eval.py``) measurements (profiles/aql_host_eval.md);
one process per variant, one JSON line each.

``--mode step``   one evaluator step's device half (staging H2D + act + actions D2H; the host step
                  excluded) of ``--kernel fused`` (1 launch) or ``step`` (3 launches + the counter
                  add) at ``--eval-envs`` Pendulum-shaped envs and ``--candidates`` candidates: the
                  host's enqueue time per step, and the per-step time from device events over
                  ``--steps`` back-to-back steps on the evaluator's side stream.  For KERNEL time run
                  this mode under ``rocprofv3 --kernel-trace --stats`` in a run of its own.
``--mode train``  ``AQLHostEngine.iteration`` rate (``--envs`` host envs, ``--k`` SGD steps per
                  iteration, captured learner graph) for ``--seconds`` with ``--eval``:
                  ``none``  no evaluation;
                  ``host``  the blocking ``train_aql.greedy_eval`` every ``--eval-interval`` iterations;
                  ``pool``  ``--eval-envs`` evaluator envs in ``--eval-workers`` processes, refreshed
                            every ``--eval-interval`` iterations and pumped every iteration.
``--mode ab``     runs ``--variants`` (``mode:flag=value,...`` items; see the profile) as child
                  processes, alternated, ``--repeat`` rounds: the form for A/Bs and their noise pairs.

Host clocks end in a device synchronize."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _engine(a, envs):
    from apex_amd.engine.aql import AQLEngineConfig
    from apex_amd.engine.aql_host import AQLHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    cfg = AQLEngineConfig(env_id=a.env, n_envs=envs, capacity=a.capacity, batch_size=a.batch, learner_steps=a.k,
                          seed=a.seed, uniform_sample=a.candidates - 1, propose_sample=1)
    return AQLHostEngine(cfg, HostVectorEnv(a.env, envs, seed=a.seed, max_episode_length=50000), "cuda:0")


def mode_step(a):
    import torch

    from apex_amd.engine.aql_host_eval import AQLHostEvaluator
    from apex_amd.engine.host_eval import eval_seed
    from apex_amd.envs.host_vector import HostVectorEnv

    eng = _engine(a, 4)
    vec = HostVectorEnv(a.env, a.eval_envs, seed=eval_seed(a.seed))
    ev = AQLHostEvaluator(eng, vec, kernel=a.kernel, seed=a.seed)
    ev.run(3)   # reset + first steps: every kernel's first launch is behind us
    dev_us, enq_us = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.repeat):
        with torch.cuda.stream(ev.stream):
            for _ in range(a.warmup):
                ev.ship()
                ev.act()
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ev.ship()
                ev.act()
            t1 = time.perf_counter()
            e1.record()
        torch.cuda.synchronize()
        dev_us.append(round(1e3 * e0.elapsed_time(e1) / a.steps, 2))
        enq_us.append(round(1e6 * (t1 - t0) / a.steps, 2))
    ev.close()
    eng.close()
    return {"kernel": a.kernel, "eval_envs": a.eval_envs, "candidates": eng.T, "steps": a.steps,
            "enqueues_per_step": {"fused": 3, "step": 6}[a.kernel], "event_us_per_step": dev_us,
            "enqueue_us_per_step": enq_us}


def mode_train(a):
    import torch

    from apex_amd.engine.aql_host_eval import AQLHostEvaluation, AQLHostEvaluator, make_pool
    from apex_amd.train_aql import greedy_eval

    eng = _engine(a, a.envs)
    drv = None
    try:
        eng.fill(a.fill)
        eng.capture()
        if a.eval == "pool":
            pool = make_pool(a.env, a.eval_envs, a.eval_workers, seed=a.seed)
            drv = AQLHostEvaluation(AQLHostEvaluator(eng, pool, kernel=a.kernel, seed=a.seed), pool)
        state = {"it": 0, "evals": 0, "t_eval": 0.0}

        def iterate():
            eng.iteration()
            state["it"] += 1
            due = state["it"] % a.eval_interval == 0
            if drv is not None:
                if due:
                    drv.refresh(eng.learner.flat)
                drv.pump(eng.learner_steps)
            elif a.eval == "host" and due:
                t = time.perf_counter()
                greedy_eval(eng, a.eval_episodes, seed=a.seed + 7 * state["it"])
                state["t_eval"] += time.perf_counter() - t
                state["evals"] += 1

        for _ in range(50):
            iterate()
        torch.cuda.synchronize()
        state.update(evals=0, t_eval=0.0)
        s0 = drv.ev.ledger.steps if drv else 0
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < a.seconds:
            iterate()
            n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"eval": a.eval, "E": a.envs, "K": eng.K, "batch": a.batch, "candidates": eng.T,
                "eval_interval": a.eval_interval, "sgd_steps_per_s": round(n * eng.K / dt, 1),
                "iterations_per_s": round(n / dt, 1), "blocking_evals": state["evals"],
                "blocking_eval_share": round(state["t_eval"] / dt, 3),
                "eval_envs": a.eval_envs if drv else 0, "eval_workers": a.eval_workers if drv else 0,
                "eval_kernel": a.kernel if drv else None,
                "evaluator_steps_per_s": round((drv.ev.ledger.steps - s0) / dt, 1) if drv else 0.0,
                "evaluator_episodes": drv.ev.ledger.episodes if drv else 0,
                "refreshes": drv.ev.weights.refreshes if drv else 0}
    finally:
        if drv is not None:
            drv.close()
        eng.close()


def mode_ab(a):
    """Each variant is ``mode:flag=value,flag=value`` -> ``--mode mode --flag value ...`` in a fresh
    child process (this parent never opens the GPU); the variants alternate ``--repeat`` times."""
    out = []
    for r in range(a.repeat):
        for v in a.variants:
            mode, _, rest = v.partition(":")
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode]
            for kv in filter(None, rest.split(",")):
                k, _, val = kv.partition("=")
                cmd += ["--" + k, val]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"variant {v!r} failed with exit status {p.returncode}")
            rec = {"round": r, "variant": v, **json.loads(p.stdout.strip().splitlines()[-1])}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return {"mode": "ab", "runs": len(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["step", "train", "ab"])
    ap.add_argument("--env", default="Pendulum-v0")
    ap.add_argument("--kernel", choices=["fused", "step"], default="fused")
    ap.add_argument("--candidates", type=int, default=51)
    ap.add_argument("--eval", choices=["none", "host", "pool"], default="pool")
    ap.add_argument("--eval-envs", type=int, default=8)
    ap.add_argument("--eval-workers", type=int, default=2)
    ap.add_argument("--eval-interval", type=int, default=500)
    ap.add_argument("--eval-episodes", type=int, default=10)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--fill", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--variants", nargs="+", default=[])
    ap.add_argument("--child-timeout", type=float, default=180.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    res = {"mode": a.mode, **{"step": mode_step, "train": mode_train, "ab": mode_ab}[a.mode](a)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
