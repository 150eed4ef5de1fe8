#!/usr/bin/env python
"""The tall mode of the wide MLP kernels (profiles/vector_tall.md), one process:

* kernel times, hip events around ``--launches`` back-to-back launches, median of ``--reps``: ``vect_act`` at
  E = 16 and 4096; ``vect_learn`` / ``vect_grad`` and their pair at obs 256 / 512 / 1024, A 18, B 64 / 512; at
  obs 128 the same through ``vecw_*`` and through ``vect_*`` (which takes any obs <= 1024), alternated inside
  every repetition, and ``vect_*`` at obs 129;
* the captured host-env engine loop at obs 1024 (64 synthetic envs, ``--learner-steps`` ``--k``): SGD steps/s,
  median of ``--reps`` windows of ``--seconds``;
* ``train_vector --host-envs --wide --tall`` itself on a synthetic env of Humanoid's 376 floats, ``--cli-steps``
  SGD steps.

``--vectb`` measures the bf16-operand tall kernels instead (profiles/vector_tall_bf16.md): ``vectb_*`` alternated
with ``vect_*`` inside every repetition at obs 128 / 256 / 512 / 1024, B 64 / 512, the two acts at E = 16 and
4096, and the captured loop at obs 1024 / B 64 for both.

``--ring`` measures ``vectb_*`` over the bf16 observation ring against the fp32 ring (profiles/vector_tall_bf16_ring.md),
alternated inside every repetition: the act at obs 1024, E = 16 and 4096; learn / grad / pair at obs 256 / 512 / 1024,
B 512; the captured loop at obs 1024 / B 64, its windows alternated between the two engines.

One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_vector_wide_bf16 import _us  # noqa: E402


def _engine(a, obs, B, tall, k=1, envs=64, tall_dtype="fp32", ring_dtype="fp32"):
    from bench_vector_host_eval import wide_env

    from apex_amd.engine.vector import VectorEngineConfig
    from apex_amd.engine.vector_host import VectorHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    vec = HostVectorEnv([lambda: wide_env(f"wide-{obs}x18")] * envs, seed=a.seed, max_obs=1024)
    cfg = VectorEngineConfig(env_id=f"wide-{obs}x18", batch_size=B, replay_capacity=16384, wide_net=True,
                             tall_obs=tall, tall_dtype=tall_dtype, ring_dtype=ring_dtype, seed=a.seed)
    return VectorHostEngine(cfg, vec, "cuda:0", learner_steps=k)


def kernels(a, obs, B, modes):
    """``modes``: the (name, tall[, tall_dtype[, ring_dtype]]) variants measured on this shape, alternated."""
    import torch

    engs = {n: _engine(a, obs, B, t, tall_dtype=(d + ["fp32"])[0], ring_dtype=(d + ["fp32"] * 2)[1])
            for n, t, *d in modes}
    f = {}
    for n, e in engs.items():
        e.fill(4 * B)
        L, s = e.learner, torch.cuda.current_stream().cuda_stream
        L.sample()
        f[n] = {"learn": lambda L=L: L._learn(L.L, s), "grad": lambda L=L: L._grad(L.G, s),
                "pair": L.forward_backward, "act64": e.shard.act}
    torch.cuda.synchronize()
    reps = {(n, k): [] for n in f for k in f[n]}
    for fn in (x for n in f for x in f[n].values()):
        _us(fn, 50)
    for _ in range(a.reps):
        for k in ("learn", "grad", "pair", "act64"):
            for n in f:
                reps[n, k].append(_us(f[n][k], a.launches))
    out = dict(what="kernels", obs=obs, A=18, B=B, launches=a.launches)
    for (n, k), v in reps.items():
        out[f"{k}_{n}_us"] = round(statistics.median(v), 2)
        out[f"{k}_{n}_spread"] = round((max(v) - min(v)) / statistics.median(v), 4)
    for e in engs.values():
        e.close()
    return out


def act(a, obs, E, tall_dtype="fp32", ring_dtypes=("fp32",)):
    """``ring_dtypes``: one shard per ring, alternated inside every repetition."""
    import numpy as np
    import torch

    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.vector_host import VectorHostShard
    from apex_amd.models.dqn import DuelingDQN

    class Rows:   # the HostVectorEnv protocol as far as a shard that only acts needs it
        continuous, n_actions, max_episode_steps = False, 18, None

        def __init__(self):
            self.obs_dim, self.staging = obs, np.zeros(E * (2 * obs + 3), np.float32)

        def __len__(self):
            return E

        def reset(self):
            self.staging[E * obs:2 * E * obs] = np.random.default_rng(a.seed).standard_normal(E * obs)

    shards = {}
    for rd in ring_dtypes:
        rp = HBMReplay(max(4096, 4 * E), n_envs=E, n_step=3, device="cuda:0", frame_bytes=(2 if rd == "bf16" else 4) * obs)
        sh = VectorHostShard(rp, Rows(), seed=a.seed, wide=True, tall=True, tall_dtype=tall_dtype, ring_dtype=rd)
        sh.set_policy(DuelingDQN.from_shapes((obs,), 18).to("cuda:0"))
        _us(sh.act, 50)
        shards[rd] = sh
    v = {rd: [] for rd in shards}
    for _ in range(a.reps):
        for rd, sh in shards.items():
            v[rd].append(_us(sh.act, a.launches))
    for sh in shards.values():
        sh.close()
    name = "vectb_act" if tall_dtype == "bf16" else "vect_act"
    out = dict(what="act", obs=obs, A=18, E=E)
    for rd, t in v.items():
        tag = name + ("" if len(v) == 1 else "_ring_" + rd)
        out[tag + "_us"] = round(statistics.median(t), 2)
        out["spread" if len(v) == 1 else tag + "_spread"] = round((max(t) - min(t)) / statistics.median(t), 4)
    return out


def loop(a, obs, B, tall_dtype="fp32"):
    import torch

    e = _engine(a, obs, B, True, a.k, tall_dtype=tall_dtype)
    e.fill(4 * B)
    e.capture()
    for _ in range(50):
        e.train_step()
    torch.cuda.synchronize()
    rate = []
    for _ in range(a.reps):
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < a.seconds:
            e.train_step()
            n += 1
        torch.cuda.synchronize()
        rate.append(n * e.K / (time.perf_counter() - t0))
    e.close()
    return dict(what="loop", tall_dtype=tall_dtype, obs=obs, A=18, B=B, K=a.k, envs=64,
                sgd_steps_per_s=round(statistics.median(rate)),
                spread=round((max(rate) - min(rate)) / statistics.median(rate), 4))


def ring_loop(a, obs, B):
    """``loop`` for the fp32 and the bf16 ring in one process, the timed windows alternated."""
    import torch

    engs = {rd: _engine(a, obs, B, True, a.k, tall_dtype="bf16", ring_dtype=rd) for rd in ("fp32", "bf16")}
    for e in engs.values():
        e.fill(4 * B)
        e.capture()
        for _ in range(50):
            e.train_step()
    torch.cuda.synchronize()
    rate = {rd: [] for rd in engs}
    for _ in range(a.reps):
        for rd, e in engs.items():
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < a.seconds:
                e.train_step()
                n += 1
            torch.cuda.synchronize()
            rate[rd].append(n * e.K / (time.perf_counter() - t0))
    out = dict(what="ring_loop", obs=obs, A=18, B=B, K=a.k, envs=64)
    for rd, e in engs.items():
        out[f"sgd_steps_per_s_ring_{rd}"] = round(statistics.median(rate[rd]))
        out[f"spread_ring_{rd}"] = round((max(rate[rd]) - min(rate[rd])) / statistics.median(rate[rd]), 4)
        out[f"replay_obs_bytes_ring_{rd}"] = e.replay.frame_bytes
        e.close()
    return out


def cli(a):
    import tempfile

    from bench_vector_host_eval import wide_env

    from apex_amd import train_vector
    from apex_amd.envs.core import register

    register("wide-376x18", lambda: wide_env("wide-376x18"))
    with tempfile.TemporaryDirectory() as d:
        args = train_vector.parser().parse_args(
            ["--host-envs", "--wide", "--tall", "--env", "wide-376x18", "--envs", "16", "--max-step",
             str(a.cli_steps), "--save-dir", d, "--log-interval", str(a.cli_steps)])
        t0 = time.perf_counter()
        last = train_vector.train(args)
    return dict(what="cli", argv="--host-envs --wide --tall --env wide-376x18 --envs 16", steps=a.cli_steps,
                seconds=round(time.perf_counter() - t0, 2), last={k: v for k, v in (last or {}).items()
                                                                  if isinstance(v, (int, float))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--cli-steps", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--vectb", action="store_true", help="vectb_* against vect_* (profiles/vector_tall_bf16.md)")
    ap.add_argument("--ring", action="store_true",
                    help="vectb_* over a bf16 ring against the fp32 ring (profiles/vector_tall_bf16_ring.md)")
    a = ap.parse_args()
    if a.ring:
        for E in (16, 4096):
            print(json.dumps(act(a, 1024, E, "bf16", ("fp32", "bf16"))), flush=True)
        for obs in (256, 512, 1024):
            modes = (("ring_fp32", True, "bf16", "fp32"), ("ring_bf16", True, "bf16", "bf16"))
            print(json.dumps(kernels(a, obs, 512, modes)), flush=True)
        print(json.dumps(ring_loop(a, 1024, 64)), flush=True)
        return
    if a.vectb:
        for E in (16, 4096):
            for dt in ("fp32", "bf16"):
                print(json.dumps(act(a, 1024, E, dt)), flush=True)
        for B in (64, 512):
            for obs in (128, 256, 512, 1024):
                print(json.dumps(kernels(a, obs, B, (("vect", True), ("vectb", True, "bf16")))), flush=True)
        for dt in ("fp32", "bf16"):
            print(json.dumps(loop(a, 1024, 64, dt)), flush=True)
        return
    for E in (16, 4096):
        print(json.dumps(act(a, 1024, E)), flush=True)
    for B in (64, 512):
        print(json.dumps(kernels(a, 128, B, (("vecw", False), ("vect", True)))), flush=True)
        for obs in (129, 256, 512, 1024):
            print(json.dumps(kernels(a, obs, B, (("vect", True),))), flush=True)
    print(json.dumps(loop(a, 1024, 64)), flush=True)
    print(json.dumps(cli(a)), flush=True)


if __name__ == "__main__":
    main()
