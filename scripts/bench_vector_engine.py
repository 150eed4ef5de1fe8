#!/usr/bin/env python
"""Vector-observation Ape-X engine vs the host-structured trainer, same box, same session.

* engine: ``VectorApexEngine`` (batch 64, ``--envs`` GPU envs), ``--steps`` train steps (one
  SGD step + one step of all envs each) through hipGraphs after a ``--warmup`` run-in.
* baseline: ``trainers.apex_single.train_DQN.learn_step`` with ``device="cuda"`` on a
  pre-filled host buffer (random-policy transitions), batch 64 -- the way the same learner
  step ran before the engine existed.  It only learns; the engine's figure includes acting.

Prints one JSON line with both rates and their ratio.  ``--trace-steps K`` instead runs K
eager train steps after the warm-up and exits (a rocprofv3 --kernel-trace target)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench_engine(a):
    import torch

    from apex_amd.engine.vector import VectorApexEngine, VectorEngineConfig

    cfg = VectorEngineConfig(env_id=a.env, n_envs=a.envs, batch_size=a.batch, replay_capacity=a.capacity)
    eng = VectorApexEngine(cfg, "cuda:0")
    eng.fill()
    if a.trace_steps:
        for _ in range(a.warmup):
            eng.train_step()
        torch.cuda.synchronize()
        for _ in range(a.trace_steps):
            eng.train_step()
        torch.cuda.synchronize()
        return {"traced_steps": a.trace_steps}
    if a.graphs:
        eng.capture()
    for _ in range(a.warmup):
        eng.train_step()
    dt = eng.run(a.steps)
    st = eng.learner.stats()
    assert all(v == v for v in st.values()), st
    env_steps = a.steps * cfg.actor_steps_per_learner_step * a.envs
    return {"sgd_steps_per_s": a.steps / dt, "env_steps_per_s": env_steps / dt, "us_per_train_step": 1e6 * dt / a.steps,
            "loss": st["loss"]}


def bench_baseline(a):
    import numpy as np
    import torch

    from apex_amd import envs
    from apex_amd.trainers.apex_single import train_DQN
    from apex_amd.utils.tb import NullWriter

    t = train_DQN(a.env, n_workers=1, batch_size=a.batch, device="cuda", writer=NullWriter(), buffer_size=a.capacity)
    try:
        env = envs.make(a.env)
        env.seed(0)
        rng = np.random.RandomState(0)
        s = env.reset()
        while len(t.buffer) < a.prefill:
            act = int(rng.randint(env.action_space.n))
            s2, r, d, _ = env.step(act)
            t.buffer.add(s, act, float(r), s2, float(d), 1.0)
            s = env.reset() if d else s2
        for _ in range(a.warmup):
            t.learn_step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.baseline_steps):
            t.learn_step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        t.batch_recorder.cleanup()
    return {"sgd_steps_per_s": a.baseline_steps / dt, "us_per_learn_step": 1e6 * dt / a.baseline_steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MountainCar-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--graphs", type=int, default=1)
    ap.add_argument("--baseline-steps", type=int, default=2000)
    ap.add_argument("--prefill", type=int, default=4096)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--trace-steps", type=int, default=0)
    a = ap.parse_args()
    out = {"env": a.env, "envs": a.envs, "batch": a.batch, "engine": bench_engine(a)}
    if not a.no_baseline and not a.trace_steps:
        out["baseline"] = bench_baseline(a)
        out["engine_over_baseline"] = out["engine"]["sgd_steps_per_s"] / out["baseline"]["sgd_steps_per_s"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
