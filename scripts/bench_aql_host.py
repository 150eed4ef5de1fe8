#!/usr/bin/env python
"""Host-env AQL engine measurements (profiles/aql_host_env.md); one process per variant:

  --mode tail      aql_host_tail alone: device events around back-to-back launches, per E
  --mode act       acting only (forward, action copy, host step, staging copy, tail): iterations/s
  --mode train     AQLHostEngine, K learner steps beside / after the host step: SGD steps/s
  --mode gpuenv    AQLEngine (device envs) at the same E and K, for scale
  --mode dis       the eager yardstick: trainers.aql train_AQL_dis (CPU workers, Python PER)

Every mode prints one JSON line.  Host clocks end in a device synchronize."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _cfg(a, **kw):
    from apex_amd.engine.aql import AQLEngineConfig

    return AQLEngineConfig(env_id=a.env, n_envs=a.envs, capacity=a.capacity, batch_size=a.batch, learner_steps=a.k,
                           seed=a.seed, **kw)


def _timed_engine(a, overlap):
    """AQLHostEngine with the host's wait for the actions and its env step timed apart."""
    import torch

    from apex_amd.engine.aql_host import AQLHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    class Timed(AQLHostEngine):
        t_wait = t_step = 0.0

        def act_finish(self):
            t0 = time.perf_counter()
            self.event.synchronize()
            t1 = time.perf_counter()
            self.vec.step(self._act_np)
            t2 = time.perf_counter()
            self.env_steps += self.E
            s = torch.cuda.current_stream().cuda_stream
            self.hip.memcpy_h2d_async(self.stage_dev.data_ptr(), self._stage_ptr, self._stage_bytes, s)
            self.hip.aql_host_tail(self._tail, s)
            Timed.t_wait += t1 - t0
            Timed.t_step += t2 - t1

    vec = HostVectorEnv(a.env, a.envs, seed=a.seed, max_episode_length=50000)
    return Timed(_cfg(a), vec, "cuda:0", host_overlap=overlap), Timed


def mode_tail(a):
    import torch

    from apex_amd.engine.aql_host import AQLHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    out = {}
    for E in (16, 64, 256):
        vec = HostVectorEnv(a.env, E, seed=a.seed)
        a.envs = E
        eng = AQLHostEngine(_cfg(a), vec, "cuda:0")
        s = torch.cuda.current_stream().cuda_stream
        for _ in range(50):
            eng.hip.aql_host_tail(eng._tail, s)
        torch.cuda.synchronize()
        reps = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                eng.hip.aql_host_tail(eng._tail, s)
            e1.record()
            torch.cuda.synchronize()
            reps.append(1e3 * e0.elapsed_time(e1) / a.launches)
        out[str(E)] = {"us_min": round(min(reps), 2), "us_max": round(max(reps), 2)}
        eng.close()
    return {"mode": "tail", "launches": a.launches, "us_per_launch": out}


def mode_act(a):
    import torch

    eng, T = _timed_engine(a, True)
    eng.fill(4 * a.envs)
    torch.cuda.synchronize()
    T.t_wait = T.t_step = 0.0
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        eng.actor_step()
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"mode": "act", "E": a.envs, "iterations_per_s": round(n / dt, 1), "env_steps_per_s": round(n * a.envs / dt),
            "host_step_share": round(T.t_step / dt, 3), "action_wait_share": round(T.t_wait / dt, 3)}


def mode_train(a):
    import torch

    eng, T = _timed_engine(a, not a.serial)
    eng.fill(a.fill)
    if a.graphs:
        eng.capture()
    for _ in range(50):
        eng.iteration()
    torch.cuda.synchronize()
    T.t_wait = T.t_step = 0.0
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        eng.iteration()
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"mode": "train", "overlap": not a.serial, "E": a.envs, "K": eng.K, "batch": a.batch,
            "sgd_steps_per_s": round(n * eng.K / dt, 1), "iterations_per_s": round(n / dt, 1),
            "env_steps_per_s": round(n * a.envs / dt), "host_step_share": round(T.t_step / dt, 3),
            "action_wait_share": round(T.t_wait / dt, 3), "episodes": len(eng.finished_episodes())}


def mode_gpuenv(a):
    import torch

    from apex_amd.engine.aql import AQLEngine

    eng = AQLEngine(_cfg(a), "cuda:0")
    eng.fill(a.fill)
    if a.graphs:
        eng.capture()
    for _ in range(50):
        eng.iteration()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        for _ in range(100):
            eng.iteration()
        torch.cuda.synchronize()
        n += 100
    dt = time.perf_counter() - t0
    return {"mode": "gpuenv", "E": a.envs, "K": eng.K, "batch": a.batch, "sgd_steps_per_s": round(n * eng.K / dt, 1),
            "iterations_per_s": round(n / dt, 1)}


def mode_dis(a):
    import torch

    from apex_amd.trainers.aql import train_AQL_dis
    from apex_amd.utils.tb import NullWriter

    with tempfile.TemporaryDirectory() as d:
        t = train_AQL_dis(a.env, max_step=a.dis_iters, n_workers=10, save_dir=d, writer=NullWriter(),
                          batch_size=a.batch, buffer_size=a.capacity)
        t0 = time.perf_counter()   # (the workers are up: their start is not timed)
        t.train()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"mode": "dis", "iterations": a.dis_iters, "sgd_steps_per_s": round(t.learn_idx / dt, 1),
                "env_steps_per_s": round(len(t.replay_buffer) / dt), "seconds": round(dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["tail", "act", "train", "gpuenv", "dis"])
    ap.add_argument("--env", default="Pendulum-v0")
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--fill", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--serial", action="store_true")
    ap.add_argument("--graphs", type=int, default=1)
    ap.add_argument("--dis-iters", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    print(json.dumps({"tail": mode_tail, "act": mode_act, "train": mode_train, "gpuenv": mode_gpuenv,
                      "dis": mode_dis}[a.mode](a)), flush=True)


if __name__ == "__main__":
    main()
