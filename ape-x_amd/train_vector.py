"""GPU Ape-X training CLI for vector-observation envs:
``python -m apex_amd.train_vector --env CartPole-v0 --envs 256 --max-step N --save-dir D``.

The MI355X counterpart of the reference's single-node ``ApeX.py`` (MountainCar-v0) and
``DQN.py`` (CartPole) trainers: one :class:`~apex_amd.engine.vector.VectorApexEngine` keeps
E vectorised GPU envs, the HBM prioritized replay and the fused MLP dueling-DQN learner on
one GPU.  One *step* = one learner SGD step + ``--actor-steps`` steps of all E envs.

Reference cadences and artefacts kept: learning starts once the replay holds more than one
batch, weights are published to the actors every 32 learner steps, the target network is
synced every 2500, and ``model{t}.pth`` (the reference ``state_dict``) is written every
``--save-interval`` (5000) steps and at the last one.  One JSON line is printed per
``--log-interval`` steps (loss, grad norms, SGD and env steps per second, the actors' mean
episode return) and, every ``--eval-interval`` steps, the greedy return of
``--eval-episodes`` evaluation episodes.  ``--eval-mode``: ``step`` evaluates with the stepwise
``evaluate()``; ``rollout`` with the one-launch ``rollout_evaluate()``; ``async`` launches the
rollout on a weight snapshot beside training (:class:`VectorEvaluator`), syncs only the training
stream at a log line, and reports a finished evaluation in the next record as
``greedy_mean_return`` with ``greedy_step``, the step of its snapshot.

``--host-envs`` trains on gym-API envs stepped on the CPU instead
(:class:`~apex_amd.engine.vector_host.VectorHostEngine`): ``--env`` is then any ``envs.make`` id
with a flat observation (<= 8 floats) and a discrete action space (<= 7 actions), one *step* of
the loop is one step of all E host envs + ``--learner-steps`` SGD steps, overlapped unless
``--host-serial``, and ``--eval-mode`` must be ``step`` (the host evaluator).  Same log tags,
checkpoints and JSON log.  ``step`` mode there is the blocking ``VectorHostEngine.evaluate`` (a
device synchronize, then whole episodes on a CPU copy of the net inside the training loop).
``--eval-envs N`` (with ``--eval-workers W``, ``--eval-kernel``) evaluates beside training instead:
N (at most 64) greedy evaluator envs in W worker processes (:mod:`apex_amd.engine.vector_host_eval`),
their weights refreshed whenever ``learn_steps`` crosses a multiple of ``--eval-interval``, the
evaluator pumped once per iteration.  ``evaluate`` is then not called and no ``greedy_mean_return``
is written; each record carries ``evaluator_episodes`` (episodes finished since the last record),
``evaluator_mean_return`` (their mean, None without one) and ``evaluator_steps`` instead.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

from .engine.vector import VECTOR_ENVS, VectorApexEngine, VectorEngineConfig, VectorEvaluator


EVAL_MODES = ("step", "rollout", "async")


class _Parser(argparse.ArgumentParser):
    """The rules between flags are parser errors (exit status 2), as a bad choice is."""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if a.host_envs:
            if a.eval_mode != "step":
                self.error("--host-envs evaluates on the host: --eval-mode must be 'step'")
            if a.learner_steps < 1:
                self.error("--learner-steps must be >= 1")
            if a.eval_envs:
                if not 0 < a.eval_envs <= 64:
                    self.error(f"--eval-envs {a.eval_envs}: the host-env evaluator runs 1..64 envs (0 = off)")
                if a.eval_interval < 1:
                    self.error("--eval-envs refreshes the evaluator's weights every --eval-interval learner steps: "
                               "it must be >= 1")
                if a.eval_workers is None:
                    a.eval_workers = min(2, a.eval_envs)
                if not 1 <= a.eval_workers <= a.eval_envs:
                    self.error(f"--eval-workers {a.eval_workers} must be in 1..--eval-envs ({a.eval_envs})")
            elif a.eval_workers is not None:
                self.error("--eval-workers is the worker count of --eval-envs")
        else:
            if a.env not in VECTOR_ENVS:
                self.error(f"argument --env: invalid choice: {a.env!r} (choose from "
                           f"{', '.join(map(repr, sorted(VECTOR_ENVS)))}; any envs.make id with --host-envs)")
            if a.learner_steps != 1 or a.host_serial:
                self.error("--learner-steps and --host-serial belong to --host-envs")
            if a.eval_envs or a.eval_workers is not None:
                self.error("--eval-envs and --eval-workers evaluate on host envs beside --host-envs training (the "
                           "GPU envs have --eval-mode rollout / async)")
        return a


def parser() -> argparse.ArgumentParser:
    d = VectorEngineConfig()
    p = _Parser(description="Ape-X DQN on vector-observation envs (GPU-resident engine)")
    p.add_argument("--env", default=d.env_id,
                   help=f"one of {sorted(VECTOR_ENVS)}; with --host-envs any envs.make id")
    p.add_argument("--host-envs", action="store_true",
                   help="step gym-API envs on the CPU (flat observation <= 8, discrete actions <= 7)")
    p.add_argument("--learner-steps", type=int, default=1, help="(--host-envs) SGD steps per env step")
    p.add_argument("--host-serial", action="store_true",
                   help="(--host-envs) learner steps, then the acting step: no overlap with the host's env step")
    p.add_argument("--max-episode-length", type=int, default=50000,
                   help="(--host-envs) reset an env after this many steps of one episode (done stays 0)")
    p.add_argument("--envs", type=int, default=d.n_envs, help="GPU envs (the reference's actor processes)")
    p.add_argument("--max-step", type=int, default=100_000, help="learner SGD steps")
    p.add_argument("--batch-size", type=int, default=d.batch_size)
    p.add_argument("--n-step", type=int, default=d.n_step)
    p.add_argument("--gamma", type=float, default=d.gamma)
    p.add_argument("--lr", type=float, default=d.lr)
    p.add_argument("--capacity", type=int, default=d.replay_capacity)
    p.add_argument("--actor-steps", type=int, default=d.actor_steps_per_learner_step,
                   help="steps of all envs per learner step")
    p.add_argument("--nstep-mode", default=d.nstep_mode, choices=["reference", "textbook"])
    p.add_argument("--target-update-interval", type=int, default=d.target_update_interval)
    p.add_argument("--publish-interval", type=int, default=d.publish_param_interval)
    p.add_argument("--save-interval", type=int, default=5000)
    p.add_argument("--save-dir", default=".")
    p.add_argument("--log-interval", type=int, default=1000, help="steps between metric reads (host syncs)")
    p.add_argument("--eval-interval", type=int, default=0, help="steps between greedy evaluations (0 = off)")
    p.add_argument("--eval-episodes", type=int, default=10)
    p.add_argument("--eval-mode", default="step", choices=EVAL_MODES,
                   help="step: the stepwise evaluator; rollout: one vec_rollout launch; async: the rollout on a "
                        "weight snapshot beside training, reported by the next log line")
    p.add_argument("--eval-envs", type=int, default=0,
                   help="(--host-envs) this many (at most 64) greedy evaluator envs in worker processes beside "
                        "training (engine.vector_host_eval); their weights are refreshed every --eval-interval "
                        "learner steps and the blocking evaluate is not called (0 = off)")
    p.add_argument("--eval-workers", type=int, default=None,
                   help="(--eval-envs) worker processes, 1..--eval-envs (default min(2, --eval-envs))")
    p.add_argument("--eval-kernel", default="fused", choices=["fused", "step"],
                   help="(--eval-envs) the evaluator's act: one vec_host_eval_act launch or the stepwise kernels")
    p.add_argument("--json-log", default=None, help="append one JSON record per log interval to this file")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--no-graphs", action="store_true")
    return p


def model_path(save_dir: str, t: int) -> str:
    return os.path.join(save_dir, f"model{t}.pth")


def config_from_args(a) -> VectorEngineConfig:
    return VectorEngineConfig(env_id=a.env, n_envs=a.envs, batch_size=a.batch_size, n_step=a.n_step, gamma=a.gamma,
                              lr=a.lr, replay_capacity=a.capacity, actor_steps_per_learner_step=a.actor_steps,
                              nstep_mode=a.nstep_mode, target_update_interval=a.target_update_interval,
                              publish_param_interval=a.publish_interval, seed=a.seed).validate(not a.host_envs)


def _crossed(t: int, prev: int, interval: int) -> bool:
    """A multiple of ``interval`` in (prev, t] (``t % interval == 0`` when t = prev + 1)."""
    return t // interval > prev // interval


def make_engine(a, cfg: VectorEngineConfig):
    if not a.host_envs:
        return VectorApexEngine(cfg, a.device)
    from .engine.vector_host import VectorHostEngine
    from .envs.host_vector import HostVectorEnv

    vec = HostVectorEnv(a.env, a.envs, seed=a.seed, max_episode_length=a.max_episode_length)
    return VectorHostEngine(cfg, vec, a.device, learner_steps=a.learner_steps, host_overlap=not a.host_serial)


def make_host_evaluation(a, eng):
    """``--eval-envs``: the worker pool and the non-blocking evaluator over it."""
    from .engine.vector_host_eval import VectorHostEvaluation, VectorHostEvaluator, make_pool

    pool = make_pool(a.env, a.eval_envs, a.eval_workers, seed=a.seed, max_episode_length=a.max_episode_length)
    try:
        return VectorHostEvaluation(VectorHostEvaluator(eng, pool, kernel=a.eval_kernel, seed=a.seed), pool)
    except BaseException:
        pool.close()
        raise


def train(a) -> dict:
    cfg = config_from_args(a)
    if not torch.cuda.is_available():
        raise RuntimeError("train_vector needs a GPU (the host-side trainer is apex_amd.trainers.apex_single)")
    eng = make_engine(a, cfg)
    hev = None
    try:
        eng.fill()
        asyn = VectorEvaluator(eng, a.eval_episodes) if a.eval_mode == "async" and a.eval_interval > 0 else None
        if not a.no_graphs:
            eng.capture()
        if a.host_envs and a.eval_envs:
            hev = make_host_evaluation(a, eng)
        return _loop(a, cfg, eng, asyn, hev)
    finally:
        if hev is not None:
            hev.close()
        if a.host_envs:
            eng.close()


def _loop(a, cfg: VectorEngineConfig, eng, asyn=None, hev=None) -> dict:
    """The training loop after fill and capture.  ``asyn`` (``--eval-mode async``): the
    :class:`VectorEvaluator`.  ``hev`` (``--eval-envs``): a
    :class:`~apex_amd.engine.vector_host_eval.VectorHostEvaluation`; it is refreshed at the
    evaluation cadence, pumped once per iteration, and its finished episodes ride in the log
    records.  The blocking ``evaluate`` is then not called."""
    mode = a.eval_mode
    jl = open(a.json_log, "a") if a.json_log else None
    last = {}
    t_win, s_win, a_win = time.perf_counter(), eng.learn_steps, eng.actor_steps
    ep_seen = torch.zeros(cfg.n_envs, device=eng.device)
    try:
        while eng.learn_steps < a.max_step:
            prev = eng.learn_steps
            eng.train_step()
            t = eng.learn_steps   # (prev + 1; prev + --learner-steps on host envs)
            final = t >= a.max_step
            if hev is not None:
                if _crossed(t, prev, a.eval_interval):
                    hev.refresh()   # (conflates while the target set is still read)
                hev.pump(t)
            if _crossed(t, prev, a.save_interval) or final:
                eng.save(model_path(a.save_dir, t))
            ev = hev is None and a.eval_interval > 0 and (_crossed(t, prev, a.eval_interval) or final)
            if ev and asyn is not None:
                # snapshot + side-stream rollout; no log line and no sync of its own.  The last step's
                # evaluation must run: wait out (and drop, they are superseded) earlier ones
                launched = asyn.launch(tag=t)
                while final and not launched:
                    asyn.wait()
                    launched = asyn.launch(tag=t)
                ev = False
            if not (_crossed(t, prev, a.log_interval) or final or ev):
                continue
            if asyn is not None:
                torch.cuda.current_stream(eng.device).synchronize()  # the side stream keeps running
            else:
                torch.cuda.synchronize(eng.device)
            dt = max(time.perf_counter() - t_win, 1e-9)
            st = eng.learner.stats()
            ret, _, cnt = eng.shard.episode_stats()
            fresh = cnt > ep_seen  # envs that finished an episode in this window
            ep_seen = cnt.clone()
            last = {"step": t, "loss": st["loss"], "grad_norm": st["grad_norm"], "grad_norm_l2": st["grad_norm_l2"],
                    "lr": st["lr"], "sgd_steps_per_s": round((t - s_win) / dt, 1),
                    "env_steps_per_s": round((eng.actor_steps - a_win) * cfg.n_envs / dt, 1),
                    "episodes": int(cnt.sum().item()),
                    "actor_mean_return": float(ret[fresh].mean().item()) if bool(fresh.any()) else None}
            if ev:
                g = eng.rollout_evaluate(a.eval_episodes) if mode == "rollout" else eng.evaluate(a.eval_episodes)
                last["greedy_mean_return"] = sum(g) / len(g)
            if hev is not None:
                done_eps = hev.poll()
                last["evaluator_episodes"] = len(done_eps)
                last["evaluator_mean_return"] = sum(e[0] for e in done_eps) / len(done_eps) if done_eps else None
                last["evaluator_steps"] = hev.ev.ledger.steps
            if asyn is not None:
                # the newest evaluation that has landed (after the last step: the final one)
                if (res := asyn.latest(block=final)) is not None:
                    last["greedy_mean_return"] = sum(res["returns"]) / len(res["returns"])
                    last["greedy_step"] = res["tag"]
            print(json.dumps(last), flush=True)
            if jl:
                jl.write(json.dumps(last) + "\n")
                jl.flush()
            t_win, s_win, a_win = time.perf_counter(), eng.learn_steps, eng.actor_steps
    finally:
        if jl:
            jl.close()
    return last


def main(argv=None) -> int:
    train(parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
