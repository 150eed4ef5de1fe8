"""Cost of the categorical (C51) heads on one MI355X (profiles/vector_dist.md).

``python scripts/bench_vector_dist.py``: ``vecw_learn + vecw_grad`` against ``vecd_learn + vecd_grad`` and ``vecw_act``
against ``vecd_act`` (``dist_atoms=51``), back-to-back launches alternated inside every repetition of one process, at
CartPole B = 64 and at obs 128 / A 8 / B 512; then the captured host-env loop at ``learner_steps=4``, plain against
categorical.  ``--trace``: a short eager run of both families, for
``rocprofv3 --kernel-trace --stats -- python scripts/bench_vector_dist.py --trace``."""
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


SHAPES = {"CartPole B 64": None, "obs 128 A 8 B 512": (128, 8, 512)}


def engine(shape, atoms, learner_steps=1):
    kw = dict(replay_capacity=65536, wide_net=True, dist_atoms=atoms, v_min=0.0, v_max=100.0)
    if SHAPES[shape] is None:
        eng = VectorApexEngine(VectorEngineConfig(env_id="CartPole-v0", n_envs=64, batch_size=64, **kw), "cuda")
    else:
        obs, A, B = SHAPES[shape]
        vec = HostVectorEnv([lambda: NoiseEnv(obs, A)] * 64, seed=0, max_obs=128)
        eng = VectorHostEngine(VectorEngineConfig(env_id="noise", batch_size=B, **kw), vec, "cuda",
                               learner_steps=learner_steps)
    eng.fill()
    for _ in range(3):
        eng.train_step()
    return eng


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n   # us per call


def launches(eng):
    return {"learn + grad": eng.learner.forward_backward, "act": eng.shard.act}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for shape in SHAPES:
        engs = {"vecw": engine(shape, 0), "vecd": engine(shape, 51)}
        for e in engs.values():
            e.learner.sample()
        for what in ("learn + grad", "act"):
            fns = {k: launches(e)[what] for k, e in engs.items()}
            if a.trace:
                for f in fns.values():
                    for _ in range(200):
                        f()
                torch.cuda.synchronize()
                continue
            rows = {k: [] for k in fns}
            for _ in range(a.reps):
                for k, f in fns.items():
                    rows[k].append(events(f, 2000))
            med = {k: statistics.median(v) for k, v in rows.items()}
            print(f"{what}, {shape}: " + "; ".join(
                f"{k} {med[k]:.2f} us (spread {(max(v) - min(v)) / med[k] * 100:.1f} %)" for k, v in rows.items())
                + f"; vecd / vecw {med['vecd'] / med['vecw']:.2f}", flush=True)
        for e in engs.values():
            getattr(e, "close", lambda: None)()
    if a.trace:
        return
    shape = "obs 128 A 8 B 512"
    engs = {"plain": engine(shape, 0, 4), "atoms 51": engine(shape, 51, 4)}
    for e in engs.values():
        e.capture(warmup_iters=3)
    rows = {k: [] for k in engs}
    for _ in range(a.reps):
        for k, e in engs.items():
            torch.cuda.synchronize()
            t0, n0 = time.perf_counter(), e.learn_steps
            while time.perf_counter() - t0 < 2.0:
                e.train_step()
            torch.cuda.synchronize()
            rows[k].append((e.learn_steps - n0) / (time.perf_counter() - t0))
    print("captured host-env loop, obs 128 / A 8 / B 512 / 64 envs / learner_steps 4 (SGD steps/s): " + "; ".join(
        f"{k} {statistics.median(v):.0f} (spread {(max(v) - min(v)) / statistics.median(v) * 100:.0f} %)"
        for k, v in rows.items()), flush=True)
    for e in engs.values():
        e.close()


if __name__ == "__main__":
    main()
