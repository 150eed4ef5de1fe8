#!/usr/bin/env python
"""GPU DQN.py engine vs the host loop of ``trainers/dqn.py``, same box, same session.

* engine: ``DQNFrameEngine`` (``DQN.py``'s defaults, ``--envs`` envs), ``--frames`` frames
  through the hipGraph after a ``--warmup`` run-in; every frame acts, steps the env, inserts
  and takes one SGD step.
* baseline: ``trainers.dqn.train_DQN.train()`` for the same number of frames on
  ``--host-device`` (default: the trainer's own default, cuda:0 when there is a GPU); its first
  ``batch_size`` frames do not learn, exactly as the engine's.

Prints one JSON line with both rates and their ratio.  ``--trace-frames K`` instead runs K
eager learning frames after the warm-up and exits (a rocprofv3 --kernel-trace target)."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench_engine(a):
    import torch

    from apex_amd.engine.dqn import DQNEngineConfig, DQNFrameEngine

    cfg = DQNEngineConfig(env_id=a.env, n_envs=a.envs, batch_size=a.batch)
    eng = DQNFrameEngine(cfg, "cuda:0")
    if a.trace_frames:
        for _ in range(eng.first_learning_frame + a.warmup):
            eng.frame()
        torch.cuda.synchronize()
        for _ in range(a.trace_frames):
            eng.frame()
        torch.cuda.synchronize()
        return {"traced_frames": a.trace_frames, "first_traced_frame": eng.frames - a.trace_frames}
    if a.graphs:
        eng.capture()
    for _ in range(a.warmup):
        eng.frame()
    dt = eng.run(a.frames)
    st = eng.stats()
    assert all(v == v for v in st.values()), st
    return {"frames_per_s": a.frames / dt, "env_steps_per_s": a.frames * a.envs / dt,
            "us_per_frame": 1e6 * dt / a.frames, "loss": st["loss"], "episodes": st["episodes"]}


def bench_host(a):
    import torch

    from apex_amd.trainers.dqn import train_DQN
    from apex_amd.utils.tb import NullWriter

    with tempfile.TemporaryDirectory() as tmp:
        t = train_DQN(a.env, max_step=a.frames, batch_size=a.batch, device=a.host_device, seed=0, save_dir=tmp,
                      writer=NullWriter(), save_interval=10 ** 9, log_every=10 ** 9)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            t.train()
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        t.env.close()
    return {"frames_per_s": a.frames / dt, "us_per_frame": 1e6 * dt / a.frames, "device": str(t.device)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="CartPole-v0")
    ap.add_argument("--envs", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--graphs", type=int, default=1)
    ap.add_argument("--host-device", default=None)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--trace-frames", type=int, default=0)
    a = ap.parse_args()
    out = {"env": a.env, "envs": a.envs, "batch": a.batch, "frames": a.frames, "engine": bench_engine(a)}
    if not a.no_baseline and not a.trace_frames:
        out["host"] = bench_host(a)
        out["engine_over_host"] = out["engine"]["frames_per_s"] / out["host"]["frames_per_s"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
