"""Cost of ``noisy_heads`` on one MI355X (profiles/vector_noisy.md).

``python scripts/bench_vector_noisy.py``: the captured learner step with and without ``noisy_heads``, alternated
inside every repetition of one process, at CartPole B = 64 (narrow), obs 128 / A 18 / B 512 (wide bf16) and
obs 1024 / A 18 / B 512 (tall bf16); ``vecn_compose`` (two nets) and ``vecn_grad`` alone, back to back; the captured
host-env loop at ``learner_steps=4``.  ``--trace``: a short run of the noisy learner step alone, for
``rocprofv3 --kernel-trace --stats -- python scripts/bench_vector_noisy.py --trace``."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apex_amd.engine.vector import VectorApexEngine, VectorEngineConfig  # noqa: E402
from apex_amd.engine.vector_host import VectorHostEngine  # noqa: E402
from apex_amd.envs.core import Env  # noqa: E402
from apex_amd.envs.host_vector import HostVectorEnv  # noqa: E402
from apex_amd.envs import spaces  # noqa: E402


class NoiseEnv(Env):
    """Seeded Gaussian observations, episodes of 50 steps: a host env that costs next to nothing."""

    def __init__(self, obs, A):
        super().__init__()
        big = np.full(obs, np.finfo(np.float32).max, dtype=np.float32)
        self.observation_space, self.action_space = spaces.Box(-big, big, dtype=np.float32), spaces.Discrete(A)
        self.obs, self.t = obs, 0

    def reset(self):
        self.t = 0
        return self.np_random.standard_normal(self.obs).astype(np.float32)

    def step(self, a):
        self.t += 1
        return self.np_random.standard_normal(self.obs).astype(np.float32), float(a == 0), self.t >= 50, {}


SHAPES = {"narrow CartPole B 64": None,
          "wide bf16 obs 128 A 18 B 512": (128, 18, dict(wide_net=True, wide_dtype="bf16")),
          "tall bf16 obs 1024 A 18 B 512": (1024, 18, dict(wide_net=True, tall_obs=True, tall_dtype="bf16"))}


def engine(shape, noisy, learner_steps=1, B=512):
    if SHAPES[shape] is None:
        eng = VectorApexEngine(VectorEngineConfig(env_id="CartPole-v0", n_envs=64, batch_size=64,
                                                  replay_capacity=65536, noisy_heads=noisy), "cuda")
    else:
        obs, A, kw = SHAPES[shape]
        vec = HostVectorEnv([lambda: NoiseEnv(obs, A)] * 64, seed=0, max_obs=1024 if kw.get("tall_obs") else 128)
        eng = VectorHostEngine(VectorEngineConfig(env_id="noise", batch_size=B, replay_capacity=65536,
                                                  noisy_heads=noisy, **kw), vec, "cuda", learner_steps=learner_steps)
    eng.fill()
    eng.capture(warmup_iters=3)
    return eng


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n   # us per call


def report(name, rows):
    """rows: {label: [us per repetition]}"""
    out = []
    for k, v in rows.items():
        out.append(f"{k} {statistics.median(v):.2f} us (spread {(max(v) - min(v)) / statistics.median(v) * 100:.1f} %)")
    print(name + ": " + "; ".join(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.trace:
        for shape in SHAPES:
            eng = engine(shape, True)
            for _ in range(200):
                eng.learner.step()   # eager: the trace names every launch
            torch.cuda.synchronize()
            getattr(eng, "close", lambda: None)()
        return
    for shape in SHAPES:
        engs = {"plain": engine(shape, False), "noisy": engine(shape, True)}
        rows = {k: [] for k in engs}
        for _ in range(a.reps):
            for k, e in engs.items():
                rows[k].append(events(e._g_learn.replay, 2000))
        report("learner step, " + shape, rows)
        L = engs["noisy"].learner
        s = torch.cuda.current_stream().cuda_stream
        k = {"vecn_compose (2 nets)": lambda: L.hip.vecn_compose(L._c_step, s),
             "vecn_grad": lambda: L.hip.vecn_grad(L.NG, s)}
        rows = {n: [events(f, 2000) for _ in range(a.reps)] for n, f in k.items()}
        report("back-to-back launches, " + shape, rows)
        for e in engs.values():
            getattr(e, "close", lambda: None)()
    shape = "wide bf16 obs 128 A 18 B 512"
    engs = {"plain": engine(shape, False, 4, B=64), "noisy": engine(shape, True, 4, B=64)}
    rows = {k: [] for k in engs}
    for _ in range(a.reps):
        for k, e in engs.items():
            torch.cuda.synchronize()
            t0, n0 = time.perf_counter(), e.learn_steps
            while time.perf_counter() - t0 < 2.0:
                e.train_step()
            torch.cuda.synchronize()
            rows[k].append((e.learn_steps - n0) / (time.perf_counter() - t0))
    print("host-env loop, obs 128 / A 18 / B 64 / 64 envs / learner_steps 4 (SGD steps/s): " + "; ".join(
        f"{k} {statistics.median(v):.0f} (spread {(max(v) - min(v)) / statistics.median(v) * 100:.0f} %)"
        for k, v in rows.items()), flush=True)
    for e in engs.values():
        e.close()


if __name__ == "__main__":
    main()
