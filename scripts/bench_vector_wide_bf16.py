#!/usr/bin/env python
"""fp32 against bf16-operand wide MLP kernels (profiles/vector_wide_bf16.md), one process, the two
variants alternated inside every repetition:

* per kernel and as the learner's pair: hip events around ``--launches`` back-to-back launches, median of
  ``--reps``, at CartPole-v0 shapes (256 device envs) for B = 64 / 256 / 1024 and at obs 128 / A 18 / B 512
  (64 synthetic host envs);
* the captured host-env engine loop at ``--learner-steps`` ``--k``: SGD steps/s, median of ``--reps`` windows
  of ``--seconds``.

One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DTYPES = ("fp32", "bf16")


def _us(fn, launches):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def _engine(a, shape, dtype, k=1):
    from apex_amd.engine.vector import VectorApexEngine, VectorEngineConfig

    cfg = VectorEngineConfig(env_id="CartPole-v0", n_envs=256, batch_size=shape["B"], replay_capacity=65536,
                             wide_net=True, wide_dtype=dtype, seed=a.seed)
    if shape["env"] == "CartPole-v0" and k == 1:
        return VectorApexEngine(cfg, "cuda:0")
    import dataclasses

    from bench_vector_host_eval import wide_env

    from apex_amd.engine.vector_host import VectorHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    if shape["env"] == "CartPole-v0":
        vec = HostVectorEnv("CartPole-v0", 16, seed=a.seed)
    else:
        vec = HostVectorEnv([lambda: wide_env(shape["env"])] * 64, seed=a.seed, max_obs=128)
    return VectorHostEngine(dataclasses.replace(cfg, env_id=shape["env"]), vec, "cuda:0", learner_steps=k)


def kernels(a, shape):
    import torch

    engs = {d: _engine(a, shape, d) for d in DTYPES}
    for e in engs.values():
        e.fill(4 * shape["B"])
        e.learner.sample()
    torch.cuda.synchronize()

    def fns(e):
        L, s = e.learner, torch.cuda.current_stream().cuda_stream
        return {"learn": lambda: L._learn(L.L, s), "grad": lambda: L._grad(L.G, s), "pair": L.forward_backward,
                "act": e.shard.act}

    f = {d: fns(e) for d, e in engs.items()}
    reps = {(d, n): [] for d in DTYPES for n in f[d]}
    for fn in (x for d in DTYPES for x in f[d].values()):
        _us(fn, 50)
    for _ in range(a.reps):
        for n in f["fp32"]:
            for d in DTYPES:   # the variants alternate
                reps[d, n].append(_us(f[d][n], a.launches))
    out = dict(shape, what="kernels", launches=a.launches)
    for (d, n), v in reps.items():
        out[f"{n}_{d}_us"] = round(statistics.median(v), 2)
        out[f"{n}_{d}_spread"] = round((max(v) - min(v)) / statistics.median(v), 4)
    for e in engs.values():
        getattr(e, "close", lambda: None)()
    return out


def loop(a, shape):
    import torch

    engs = {d: _engine(a, shape, d, a.k) for d in DTYPES}
    for e in engs.values():
        e.fill(4 * shape["B"])
        e.capture()
        for _ in range(50):
            e.train_step()
    torch.cuda.synchronize()
    rate = {d: [] for d in DTYPES}
    for _ in range(a.reps):
        for d, e in engs.items():
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < a.seconds:
                e.train_step()
                n += 1
            torch.cuda.synchronize()
            rate[d].append(n * e.K / (time.perf_counter() - t0))
    out = dict(shape, what="loop", K=a.k, envs=len(engs["fp32"].vec))
    for d, v in rate.items():
        out[f"sgd_steps_per_s_{d}"] = round(statistics.median(v))
    for e in engs.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    cart = [dict(env="CartPole-v0", obs=4, A=2, B=B) for B in (64, 256, 1024)]
    big = dict(env="wide-128x18", obs=128, A=18, B=512)
    for shape in cart + [big]:
        print(json.dumps(kernels(a, shape)), flush=True)
    for shape in (cart[0], big):
        print(json.dumps(loop(a, shape)), flush=True)


if __name__ == "__main__":
    main()
