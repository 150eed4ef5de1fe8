#!/usr/bin/env python
"""Host-env engine (``engine/host_env.py``) measurements, one JSON line per mode.

``--mode host``     host only: ``AtariPreprocess.step`` (the parent's per-step pixel work in numpy)
                    against ``RawAtariVector.step`` (frames only), env steps/s at ``--envs``.
``--mode ingest``   ``--steps`` launches of ``host_env_ingest`` at ``--envs`` on seeded random pairs
                    (device events give the mean; run under ``rocprofv3 --kernel-trace --stats`` for
                    the kernel's own duration), and the bytes copied per step.
``--mode engine``   ``HostEnvEngine.iteration`` rate with ``--k`` learner steps per env step (0 =
                    acting only) over the synthetic emulator, after the learner graph is captured.
``--mode learner``  the same learner graph replayed alone (no acting), steps/s.
``--mode learn``    one learning run: ``--steps`` iterations, the actors' clipped return and unclipped
                    score over the run's last finished episodes against a random policy's
                    (``--k 0`` run of the same length, same seeds).

``--workers W`` (modes host, engine, learn) steps the emulators in ``W`` worker processes
(``ProcRawAtariVector``) and ``--ingest`` picks banked or whole ingest; 0 is the in-process vector.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _vec(a, raw=True):
    from apex_amd.envs.core import make
    from apex_amd.envs.preprocess import AtariPreprocess, PreprocessSpec
    from apex_amd.envs.raw_vector import RawAtariVector

    if raw and a.workers:
        from apex_amd.envs.proc_vector import ProcRawAtariVector

        return ProcRawAtariVector(a.env, a.envs, PreprocessSpec(), workers=a.workers, seed=a.seed)
    cls = RawAtariVector if raw else AtariPreprocess
    v = cls([make(a.env) for _ in range(a.envs)], PreprocessSpec())
    v.seed(a.seed)
    return v


def mode_host(a):
    import numpy as np

    out = {}
    for name, raw in (("atari_preprocess", False), ("raw_vector", True)):
        v = _vec(a, raw)
        rng = np.random.default_rng(0)
        n_act = v.action_space.n
        buf = v.staging if raw and a.workers else np.zeros((a.envs, 2) + tuple(v.envs[0].observation_space.shape),
                                                           np.uint8)
        v.reset(buf) if raw else v.reset()
        acts = [rng.integers(0, n_act, a.envs) for _ in range(a.warmup + a.steps)]
        for t in range(a.warmup + a.steps):
            if t == a.warmup:
                t0 = time.perf_counter()
            if raw:
                v.step(acts[t], buf)
            else:
                _, _, d, _ = v.step(acts[t])
                for i in np.flatnonzero(d):
                    v.reset_one(int(i))
        dt = time.perf_counter() - t0
        out[name] = {"env_steps_per_s": a.steps * a.envs / dt, "ms_per_env_step": 1e3 * dt / (a.steps * a.envs)}
        if hasattr(v, "close"):
            v.close()
    out["workers"] = a.workers
    out["raw_over_preprocess"] = out["raw_vector"]["env_steps_per_s"] / out["atari_preprocess"]["env_steps_per_s"]
    return out


def mode_ingest(a):
    import torch

    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.host_env import HostEnvShard

    dev = torch.device("cuda:0")
    rp = HBMReplay(max(4096, 8 * a.envs), n_envs=a.envs, device=dev)
    sh = HostEnvShard(rp, a.envs, 18, (a.height, a.width, 3))
    g = torch.Generator().manual_seed(a.seed)
    sh.raw_host.copy_(torch.randint(0, 256, sh.raw_host.shape, generator=g, dtype=torch.uint8))
    sh.raw_dev.copy_(sh.raw_host)
    for _ in range(a.warmup):
        sh._ingest(False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.steps):
        sh._ingest(False)
    e1.record()
    torch.cuda.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / a.steps
    # the H2D copy alone, from the pinned staging buffer
    e0.record()
    for _ in range(a.steps):
        sh.raw_dev.copy_(sh.raw_host, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    return {"envs": a.envs, "raw_hw": [a.height, a.width], "ingest_us_back_to_back": us,
            "h2d_us": 1e3 * e0.elapsed_time(e1) / a.steps, "bytes_h2d_per_step": sh.raw_bytes_per_step,
            "bytes_d2h_per_step": 4 * a.envs, "bytes_ring_per_step": 7056 * a.envs}


def _engine(a, k, vec=None):
    from apex_amd.engine.host_env import HostEnvConfig, HostEnvEngine
    from apex_amd.engine.learner import LearnerConfig

    cfg = HostEnvConfig(replay_capacity=a.capacity, threshold_size=a.threshold, learner_steps_per_actor_step=k,
                        seed=a.seed, target_update_interval=a.target_interval, ingest=a.ingest,
                        learner=LearnerConfig(batch_size=a.batch, forward="hip", lr=a.lr, seed=a.seed))
    return HostEnvEngine(cfg, vec if vec is not None else _vec(a), "cuda:0")


def mode_engine(a):
    eng = _engine(a, a.k)
    fill = -(-a.threshold // a.envs) + 1
    for _ in range(fill + a.warmup):
        eng.iteration()
    l0 = eng.learn_steps
    dt = eng.run(a.steps)
    res = {"envs": a.envs, "k": a.k, "batch": a.batch, "workers": a.workers, "ingest": eng.ingest,
           "iterations_per_s": a.steps / dt,
           "env_steps_per_s": a.steps * a.envs / dt, "frames_per_s": a.steps * eng.frames_per_actor_step / dt,
           "learner_steps_per_s": (eng.learn_steps - l0) / dt, "graph": eng._g_learn is not None}
    eng.close()
    return res


def mode_learner(a):
    import torch

    eng = _engine(a, 1)
    for _ in range(-(-a.threshold // a.envs) + 2):
        eng.iteration()
    assert eng._g_learn is not None
    for _ in range(a.warmup):
        eng._learner_step()
    torch.cuda.synchronize()
    n = a.steps * max(1, a.k)
    t0 = time.perf_counter()
    for _ in range(n):
        eng._learner_step()
    torch.cuda.synchronize()
    return {"batch": a.batch, "learner_steps_per_s_alone": n / (time.perf_counter() - t0)}


def mode_learn(a):
    out = {"envs": a.envs, "iterations": a.steps, "batch": a.batch, "lr": a.lr, "threshold": a.threshold,
           "workers": a.workers, "ingest": a.ingest,
           "target_interval": a.target_interval, "env": a.env}
    for name, k in (("random_policy", 0), ("learning", a.k)):
        eng = _engine(a, k)
        if k == 0:
            eng.actor.eps.fill_(1.0)  # uniform random actions
        t0 = time.perf_counter()
        half = []
        for i in range(a.steps):
            eng.iteration()
            if i == a.steps // 2:
                half = eng.stats()
        st = eng.stats()
        out[name] = {"k": k, "seconds": time.perf_counter() - t0, "learn_steps": eng.learn_steps,
                     "episodes": st["episodes"], "episode_reward_last": st.get("episode_reward"),
                     "episode_score_last": st.get("episode_score"), "episode_length_last": st.get("episode_length"),
                     "episode_reward_halfway": half.get("episode_reward"), "loss": st.get("loss")}
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["host", "ingest", "engine", "learner", "learn"], required=True)
    ap.add_argument("--env", default="SeaquestNoFrameskip-v4")
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--height", type=int, default=210)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--workers", type=int, default=0, help="emulator worker processes (0 = in process)")
    ap.add_argument("--ingest", choices=["auto", "whole", "banked"], default="auto")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--threshold", type=int, default=2048)
    ap.add_argument("--target-interval", type=int, default=2500)
    ap.add_argument("--lr", type=float, default=6.25e-5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--seed", type=int, default=1122)
    a = ap.parse_args()
    res = {"mode": a.mode, **globals()[f"mode_{a.mode}"](a)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
