#!/usr/bin/env python
"""Host-env evaluator (``engine/host_eval.py``) measurements, one JSON line per mode.

``--mode step``   one evaluator step (ingest + act + actions D2H, host step excluded) of
                  ``kernel="fused"`` (2 launches) against ``kernel="step"`` (7 launches) at
                  ``--eval-envs``: device time from events on the evaluator's side stream over
                  ``--steps`` back-to-back steps, and the host's enqueue time per step.  ``--repeat``
                  alternated repetitions give the spread.
``--mode train``  ``HostEnvEngine.iteration`` rate (``--envs`` emulators in ``--workers`` processes,
                  ``--k`` learner steps per env step -- the README's ``train_host`` line) with an
                  asynchronous evaluator of ``--eval-envs`` emulators in ``--eval-workers`` processes
                  pumped every iteration (``--eval-envs 0``: none, the engine alone).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def mode_step(a):
    import torch

    from apex_amd.engine.host_eval import HostEvaluator
    from apex_amd.envs.core import make
    from apex_amd.envs.preprocess import PreprocessSpec
    from apex_amd.envs.raw_vector import RawAtariVector
    from apex_amd.models.dqn import DuelingDQN

    dev = torch.device("cuda:0")
    vec = RawAtariVector([make(a.env) for _ in range(a.eval_envs)], PreprocessSpec())
    vec.seed(a.seed)
    torch.manual_seed(a.seed)
    model = DuelingDQN.from_shapes((4, 84, 84), vec.n_actions)
    evs = {k: HostEvaluator(model, vec, dev, kernel=k, seed=a.seed) for k in ("fused", "step")}
    for ev in evs.values():
        ev.run(2)   # reset + first steps: every kernel's first launch is behind us
    out = {"eval_envs": a.eval_envs, "steps": a.steps, "launches_per_step": {"fused": 2, "step": 7},
           "device_us": {"fused": [], "step": []}, "enqueue_us": {"fused": [], "step": []}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.repeat):
        for k, ev in evs.items():
            with torch.cuda.stream(ev.stream):
                for _ in range(a.warmup):
                    ev.ship(False)
                    ev.act()
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    ev.ship(False)
                    ev.act()
                t1 = time.perf_counter()
                e1.record()
            torch.cuda.synchronize()
            out["device_us"][k].append(round(1e3 * e0.elapsed_time(e1) / a.steps, 2))
            out["enqueue_us"][k].append(round(1e6 * (t1 - t0) / a.steps, 2))
    return out


def mode_train(a):
    import torch

    from apex_amd.engine.host_env import HostEnvConfig, HostEnvEngine
    from apex_amd.engine.host_eval import HostEnvEvaluation, HostEvaluator, eval_seed
    from apex_amd.engine.learner import LearnerConfig
    from apex_amd.envs.preprocess import PreprocessSpec
    from apex_amd.envs.proc_vector import ProcRawAtariVector

    vec = ProcRawAtariVector(a.env, a.envs, PreprocessSpec(), workers=a.workers, seed=a.seed)
    cfg = HostEnvConfig(replay_capacity=a.capacity, threshold_size=a.threshold, learner_steps_per_actor_step=a.k,
                        seed=a.seed, learner=LearnerConfig(batch_size=a.batch, forward="hip", seed=a.seed))
    eng = HostEnvEngine(cfg, vec, "cuda:0")
    evaluation = None
    try:
        if a.eval_envs:
            pool = ProcRawAtariVector(a.env, a.eval_envs, PreprocessSpec(), workers=a.eval_workers,
                                      seed=eval_seed(a.seed), max_episode_steps=50000)
            evaluation = HostEnvEvaluation(HostEvaluator(eng.actor_model, pool, "cuda:0", kernel=a.eval_kernel,
                                                         seed=eval_seed(a.seed)), pool)

        def iterate(n):
            for _ in range(n):
                eng.iteration()
                if evaluation is not None:
                    if eng.learn_steps % a.eval_interval < a.k:
                        evaluation.refresh(eng.actor_flat, eng.actor_net)
                    evaluation.pump(eng.learn_steps)

        iterate(-(-a.threshold // a.envs) + 1 + a.warmup)
        torch.cuda.synchronize()
        l0, s0 = eng.learn_steps, evaluation.ev.ledger.steps if evaluation else 0
        t0 = time.perf_counter()
        iterate(a.steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res = {"envs": a.envs, "workers": a.workers, "k": a.k, "batch": a.batch, "eval_envs": a.eval_envs,
               "eval_workers": a.eval_workers if a.eval_envs else 0, "eval_kernel": a.eval_kernel,
               "iterations_per_s": round(a.steps / dt, 1), "learner_steps_per_s": round((eng.learn_steps - l0) / dt, 1),
               "evaluator_steps_per_s": round((evaluation.ev.ledger.steps - s0) / dt, 1) if evaluation else 0.0,
               "refreshes": evaluation.ev.weights.refreshes if evaluation else 0, "graph": eng._g_learn is not None}
        return res
    finally:
        if evaluation is not None:
            evaluation.close()
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "train"], required=True)
    ap.add_argument("--env", default="SeaquestNoFrameskip-v4")
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--eval-envs", type=int, default=8)
    ap.add_argument("--eval-workers", type=int, default=2)
    ap.add_argument("--eval-kernel", choices=["fused", "step"], default="fused")
    ap.add_argument("--eval-interval", type=int, default=100)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--threshold", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1122)
    a = ap.parse_args()
    res = {"mode": a.mode, **globals()[f"mode_{a.mode}"](a)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
