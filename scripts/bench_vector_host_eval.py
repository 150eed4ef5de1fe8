#!/usr/bin/env python
"""Host-env vector evaluator (``engine/vector_host_eval.py``) measurements
(profiles/vector_host_eval.md); one process per variant, one JSON line each.

``--mode step``   one evaluator step's device half (staging H2D + act + actions D2H; the host step
                  excluded) of ``--kernel fused`` (1 launch) or ``step`` (``vec_host_tail`` +
                  ``frame_hist_step`` + ``vec_act``) at ``--eval-envs`` CartPole envs: the host's
                  enqueue time per step, and the per-step time from device events over ``--steps``
                  back-to-back steps on the evaluator's side stream.  For KERNEL time run this mode
                  under ``rocprofv3 --kernel-trace --stats`` in a run of its own.
``--mode train``  ``train_vector --host-envs``'s loop (``--envs`` host envs, ``--k`` SGD steps per
                  iteration, captured learner graph, the CLI's defaults otherwise) for ``--seconds``
                  with ``--eval``:
                  ``none``  no evaluation;
                  ``host``  the blocking ``VectorHostEngine.evaluate`` whenever ``learn_steps``
                            crosses a multiple of ``--eval-interval``;
                  ``pool``  ``--eval-envs`` evaluator envs in ``--eval-workers`` processes, refreshed
                            at that cadence and pumped every iteration.
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


def _args(a, envs):
    """``train_vector``'s namespace for this run: its defaults + the flags of the profile."""
    from apex_amd import train_vector

    return train_vector.parser().parse_args(
        ["--host-envs", "--env", a.env, "--envs", str(envs), "--lr", str(a.lr), "--learner-steps", str(a.k),
         "--seed", str(a.seed)])


def _engine(a, envs):
    from apex_amd import train_vector

    ta = _args(a, envs)
    return train_vector.make_engine(ta, train_vector.config_from_args(ta))


def mode_step(a):
    import torch

    from apex_amd.engine.host_eval import eval_seed
    from apex_amd.engine.vector_host_eval import VectorHostEvaluator
    from apex_amd.envs.host_vector import HostVectorEnv

    eng = _engine(a, 4)
    vec = HostVectorEnv(a.env, a.eval_envs, seed=eval_seed(a.seed))
    ev = VectorHostEvaluator(eng, vec, kernel=a.kernel, seed=a.seed)
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
    vec.close()
    eng.close()
    return {"kernel": a.kernel, "eval_envs": a.eval_envs, "steps": a.steps,
            "enqueues_per_step": {"fused": 3, "step": 5}[a.kernel], "event_us_per_step": dev_us,
            "enqueue_us_per_step": enq_us}


def mode_train(a):
    import torch

    from apex_amd.engine.vector_host_eval import VectorHostEvaluation, VectorHostEvaluator, make_pool

    eng = _engine(a, a.envs)
    drv = None
    try:
        eng.fill()
        eng.capture()
        if a.eval == "pool":
            pool = make_pool(a.env, a.eval_envs, a.eval_workers, seed=a.seed)
            try:
                drv = VectorHostEvaluation(VectorHostEvaluator(eng, pool, kernel=a.kernel, seed=a.seed), pool)
            except BaseException:
                pool.close()
                raise
        state = {"evals": 0, "t_eval": 0.0, "t_pump": 0.0}

        def iterate():
            prev = eng.learn_steps
            eng.train_step()
            t = eng.learn_steps
            due = t // a.eval_interval > prev // a.eval_interval
            if drv is not None:
                c = time.perf_counter()
                if due:
                    drv.refresh()
                drv.pump(t)
                state["t_pump"] += time.perf_counter() - c
            elif a.eval == "host" and due:
                c = time.perf_counter()
                eng.evaluate(a.eval_episodes)
                state["t_eval"] += time.perf_counter() - c
                state["evals"] += 1

        for _ in range(50):
            iterate()
        torch.cuda.synchronize()
        state.update(evals=0, t_eval=0.0, t_pump=0.0)
        s0 = drv.ev.ledger.steps if drv else 0
        p0 = drv.pumps if drv else 0
        h0 = eng.shard.host_seconds
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < a.seconds:
            iterate()
            n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"eval": a.eval, "E": a.envs, "K": eng.K, "eval_interval": a.eval_interval,
                "sgd_steps_per_s": round(n * eng.K / dt, 1), "iterations_per_s": round(n / dt, 1),
                "host_env_share": round((eng.shard.host_seconds - h0) / dt, 3), "blocking_evals": state["evals"],
                "blocking_eval_share": round(state["t_eval"] / dt, 3),
                "pump_share": round(state["t_pump"] / dt, 3),
                "pump_us": round(1e6 * state["t_pump"] / max(drv.pumps - p0, 1), 2) if drv else 0.0,
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
    ap.add_argument("--env", default="CartPole-v0")
    ap.add_argument("--kernel", choices=["fused", "step"], default="fused")
    ap.add_argument("--eval", choices=["none", "host", "pool"], default="pool")
    ap.add_argument("--eval-envs", type=int, default=8)
    ap.add_argument("--eval-workers", type=int, default=2)
    ap.add_argument("--eval-interval", type=int, default=1000)
    ap.add_argument("--eval-episodes", type=int, default=10)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--lr", type=float, default=2.5e-4)
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
