#!/usr/bin/env python
"""GPU AQL.py engine vs the host loop of ``trainers/aql.py:train_AQL``, same box, same session.

* engine: ``AQLFrameEngine`` (``AQL.py``'s defaults: Pendulum-v0, T = 200 candidates, batch 32,
  capacity 100 000), ``--frames`` frames (>= 20 000 by default) through ``run()`` -- the two
  captured hipGraphs -- after a ``--warmup`` run-in that passes the first learning frame; every
  timed frame acts, steps the env, inserts and takes one SGD step: five launches.
* baseline: ``train_AQL.train()`` for ``--host-frames`` frames on ``--host-device`` (default: the
  trainer's own default, cuda:0 when there is a GPU); its first ``batch_size`` frames do not
  learn, exactly as the engine's.

Prints one JSON line with both rates and their ratio.  ``--trace-frames K`` instead runs K eager
learning frames after the warm-up and exits (a rocprofv3 --kernel-trace target)."""
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

    from apex_amd.engine.aql_frame import AQLFrameConfig, AQLFrameEngine

    cfg = AQLFrameConfig(env_id=a.env, batch_size=a.batch, propose_sample=a.propose, uniform_sample=a.uniform,
                         use_graphs=bool(a.graphs))
    eng = AQLFrameEngine(cfg, "cuda:0")
    warm = eng.first_learning_frame + max(a.warmup, 2)
    if a.trace_frames:
        for _ in range(warm):
            eng.frame()
        torch.cuda.synchronize()
        for _ in range(a.trace_frames):
            eng.frame()
        torch.cuda.synchronize()
        return {"traced_frames": a.trace_frames, "first_traced_frame": eng.frames - a.trace_frames}
    eng.run(warm)   # (captures both graphs)
    dt = eng.run(a.frames)
    st = eng.stats()
    assert all(v == v for v in st.values()), st
    return {"frames_per_s": a.frames / dt, "us_per_frame": 1e6 * dt / a.frames,
            "launches_per_frame": eng.launches_per_frame, "candidates": eng.T, "loss_q": st["loss_q"],
            "loss_proposal": st["loss_proposal"], "lr": st["lr"], "beta": st["beta"],
            "episodes": len(eng.finished_episodes())}


def bench_host(a):
    import torch

    from apex_amd.trainers.aql import train_AQL
    from apex_amd.utils.tb import NullWriter

    n = a.host_frames
    with tempfile.TemporaryDirectory() as tmp:
        t = train_AQL(a.env, max_step=n, batch_size=a.batch, propose_sample=a.propose, uniform_sample=a.uniform,
                      device=a.host_device, seed=0, save_dir=tmp, writer=NullWriter(), save_interval=10 ** 9)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            t.train()
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    return {"frames": n, "frames_per_s": n / dt, "us_per_frame": 1e6 * dt / n, "device": str(t.device)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Pendulum-v0")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--propose", type=int, default=100)
    ap.add_argument("--uniform", type=int, default=100)
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--host-frames", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--graphs", type=int, default=1)
    ap.add_argument("--host-device", default=None)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--trace-frames", type=int, default=0)
    a = ap.parse_args()
    out = {"env": a.env, "batch": a.batch, "frames": a.frames, "engine": bench_engine(a)}
    if not a.no_baseline and not a.trace_frames:
        out["host"] = bench_host(a)
        out["engine_over_host"] = out["engine"]["frames_per_s"] / out["host"]["frames_per_s"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
