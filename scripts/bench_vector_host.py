#!/usr/bin/env python
"""Host-env vector engine measurements (profiles/vector_host_env.md); one process per variant:

  --mode tail      vec_host_tail alone: device events around back-to-back launches, per E
  --mode trace     the same launches with no timing of their own (a rocprofv3 --kernel-trace target)
  --mode act       acting only (forward, action copy, host step, staging copy, tail, n-step, tree)
  --mode train     VectorHostEngine, K learner steps beside / after the host step: SGD steps/s
  --mode gpuenv    VectorApexEngine (device envs) at the same E, for scale
  --mode hostloop  the host loop a user had before: trainers.apex_single train_DQN (CPU worker
                   processes, eager PyTorch learner on the GPU, Python PER)

Every mode prints one JSON line.  Host clocks end in a device synchronize."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TAIL_ENVS = (16, 64, 256, 4096)


def _cfg(a, **kw):
    from apex_amd.engine.vector import VectorEngineConfig

    return VectorEngineConfig(env_id=a.env, n_envs=a.envs, batch_size=a.batch, replay_capacity=a.capacity,
                              seed=a.seed, **kw)


def _timed_engine(a, overlap):
    """VectorHostEngine with the host's wait for the actions timed (the shard times vec.step)."""
    from apex_amd.engine.vector_host import VectorHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    vec = HostVectorEnv(a.env, a.envs, seed=a.seed, max_episode_length=50000)
    eng = VectorHostEngine(_cfg(a), vec, "cuda:0", learner_steps=a.k, host_overlap=overlap)
    ev, waits = eng.shard.event, [0.0]
    sync = ev.synchronize

    class Timed:
        def record(self, *x):
            return ev.record(*x)

        def synchronize(self):
            t0 = time.perf_counter()
            sync()
            waits[0] += time.perf_counter() - t0

    eng.shard.event = Timed()
    return eng, waits


def _tail_rig(E, obs=4):
    """A VecHostTail over buffers of its own (no engine): E envs, F = 4E ring rows."""
    import numpy as np
    import torch

    from apex_amd import ops

    h, dev, F = ops.hip(), "cuda:0", 4 * E
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    rng = np.random.RandomState(E)
    b = {"stage": torch.from_numpy(rng.uniform(-1, 1, size=E * (2 * obs + 3)).astype(np.float32)).to(dev),
         "ring": torch.zeros(F, obs, **f32), "step": torch.zeros(1, dtype=torch.int64, device=dev),
         "reward": torch.zeros(E, **f32), "done": torch.zeros(E, **f32), "new_frame": torch.zeros(E, **i32),
         "hist": torch.zeros(E, 4, **i32), "ep_log": torch.zeros(E, 4, **f32), "ep_ret": torch.zeros(E, **f32),
         "ep_len": torch.zeros(E, **f32)}
    tail = h.make_vec_host_tail(dict(E=E, obs=obs, F=F, **{k: v.data_ptr() for k, v in b.items()}))
    return h, tail, b


def mode_tail(a):
    import torch

    out = {}
    for E in TAIL_ENVS:
        h, tail, keep = _tail_rig(E)
        s = torch.cuda.current_stream().cuda_stream
        for _ in range(50):
            h.vec_host_tail(tail, False, s)
        torch.cuda.synchronize()
        reps = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                h.vec_host_tail(tail, False, s)
            e1.record()
            torch.cuda.synchronize()
            reps.append(1e3 * e0.elapsed_time(e1) / a.launches)
        out[str(E)] = {"us_min": round(min(reps), 2), "us_max": round(max(reps), 2)}
    return {"mode": "tail", "launches": a.launches, "us_per_launch": out}


def mode_trace(a):
    import torch

    n = {}
    for E in TAIL_ENVS:
        h, tail, keep = _tail_rig(E)
        s = torch.cuda.current_stream().cuda_stream
        for _ in range(a.launches):
            h.vec_host_tail(tail, False, s)
        torch.cuda.synchronize()
        n[str(E)] = a.launches
    return {"mode": "trace", "launches": n}


def mode_act(a):
    import torch

    eng, waits = _timed_engine(a, True)
    eng.fill(4 * a.envs)
    torch.cuda.synchronize()
    waits[0], eng.shard.host_seconds = 0.0, 0.0
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        eng.actor_step()
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"mode": "act", "E": a.envs, "iterations_per_s": round(n / dt, 1), "env_steps_per_s": round(n * a.envs / dt),
           "host_step_share": round(eng.shard.host_seconds / dt, 3), "action_wait_share": round(waits[0] / dt, 3)}
    eng.close()
    return out


def mode_train(a):
    import torch

    eng, waits = _timed_engine(a, not a.serial)
    eng.fill(a.fill)
    if a.graphs:
        eng.capture()
    for _ in range(50):
        eng.train_step()
    torch.cuda.synchronize()
    waits[0], eng.shard.host_seconds = 0.0, 0.0
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        eng.train_step()
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"mode": "train", "overlap": not a.serial, "E": a.envs, "K": eng.K, "batch": a.batch,
           "sgd_steps_per_s": round(n * eng.K / dt, 1), "iterations_per_s": round(n / dt, 1),
           "env_steps_per_s": round(n * a.envs / dt), "host_step_share": round(eng.shard.host_seconds / dt, 3),
           "action_wait_share": round(waits[0] / dt, 3), "loss": float(eng.learner.loss.item())}
    eng.close()
    return out


def mode_gpuenv(a):
    import torch

    from apex_amd.engine.vector import VectorApexEngine

    eng = VectorApexEngine(_cfg(a), "cuda:0")
    eng.fill(a.fill)
    if a.graphs:
        eng.capture()
    for _ in range(50):
        eng.train_step()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        for _ in range(100):
            eng.train_step()
        torch.cuda.synchronize()
        n += 100
    dt = time.perf_counter() - t0
    return {"mode": "gpuenv", "E": a.envs, "batch": a.batch, "sgd_steps_per_s": round(n / dt, 1),
            "env_steps_per_s": round(n * a.envs / dt)}


def mode_hostloop(a):
    import torch

    from apex_amd.trainers.apex_single import train_DQN
    from apex_amd.utils.tb import NullWriter

    with tempfile.TemporaryDirectory() as d:
        t = train_DQN(a.env, n_workers=a.envs, batch_size=a.batch, device="cuda", writer=NullWriter(),
                      buffer_size=a.capacity, max_step=a.hostloop_steps, save_dir=d, save_interval=10 ** 9)
        first, step = [None, 0], t.learn_step

        def learn_step():   # (the clock starts at the first SGD step: the workers' start-up is not timed)
            if first[0] is None:
                first[0], first[1] = time.perf_counter(), len(t.buffer)
            return step()

        t.learn_step = learn_step
        t.train()
        torch.cuda.synchronize()
        dt = time.perf_counter() - first[0]
        return {"mode": "hostloop", "workers": a.envs, "batch": a.batch, "sgd_steps": t.learn_idx,
                "sgd_steps_per_s": round(t.learn_idx / dt, 1),
                "transitions_per_s": round((len(t.buffer) - first[1]) / dt), "seconds": round(dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["tail", "trace", "act", "train", "gpuenv", "hostloop"])
    ap.add_argument("--env", default="CartPole-v0")
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--fill", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--serial", action="store_true")
    ap.add_argument("--graphs", type=int, default=1)
    ap.add_argument("--hostloop-steps", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    print(json.dumps({"tail": mode_tail, "trace": mode_trace, "act": mode_act, "train": mode_train,
                      "gpuenv": mode_gpuenv, "hostloop": mode_hostloop}[a.mode](a)), flush=True)


if __name__ == "__main__":
    main()
