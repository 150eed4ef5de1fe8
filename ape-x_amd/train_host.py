"""Ape-X on HOST Atari environments under the fused GPU learner:
``python -m apex_amd.train_host --env SeaquestNoFrameskip-v4 --envs 16 [arguments.py flags]``.

The reference's ``actor.py --env <id>`` case on one GPU: ``--envs`` emulators built by
``envs.core.make`` (the synthetic ALE-surface emulator of this package, or real ALE wherever gym
registers the id) are stepped on the host with the reference's start / repeat / life / FIRE
semantics (``envs.raw_vector.RawAtariVector``); their raw frames are preprocessed on the GPU
into the HBM frame ring, and the replay, n-step batcher and fused learner are the flagship
engine's (``engine.host_env.HostEnvEngine``).  ``apex_amd.train`` remains the CLI of the
GPU-resident envs.

``--workers W`` steps the emulators in ``W`` worker processes (``envs.proc_vector.ProcRawAtariVector``:
shared-memory staging that the GPU copies out of in place, per-worker ingest with ``--ingest
banked``); the default 0 is the in-process vector.  Both compute the same run, bit for bit.

Flags: the reference's (``--env``, ``--episode_life``, ``--clip_rewards``, ``--replay_buffer_size``,
``--threshold_size``, ``--batch_size``, intervals, ...) plus ``--envs``, ``--learner-steps`` (learner
steps enqueued per env step), ``--workers``, ``--worker-timeout`` (seconds a worker may stay silent),
``--ingest {auto,whole,banked}``, ``--max-step`` (learner steps, 0 = forever), ``--save-path``,
``--resume`` (model + ``.train.pt`` sidecar, as ``apex_amd.train``: the replay is filled afresh),
``--state-dir`` / ``--save-state-interval`` / ``--resume-state`` (below) and ``--log-dir``.  Logged every
``--bps_interval`` learner steps: ``learner/loss``, ``learner/grad_norm``, ``learner/BPS``,
``actor/episode_reward`` (clipped return), ``actor/episode_length``, ``actor/episode_score``
(unclipped game score), ``actor/frames_per_sec`` and ``replay/size``.

``--state-dir D`` writes a full-state checkpoint -- the replay with its frame ring and priority tree,
the learner, the acting weights and the counters -- as the directory ``D`` at the end of the run and
every ``--save-state-interval`` learner steps (``utils/engine_state.py``).  ``--resume-state D`` is a
replay-preserving resume: it restores all of that and starts the emulators afresh (host emulators
cannot be restored, and the at most n * E transitions inside the n-step windows open at save time
are lost), so training continues on the saved replay instead of refilling it.

``--eval-envs N`` (default 0 = off) adds the reference's evaluator (``eval.py``): ``N`` further
emulators played greedily (epsilon 0, rewards unclipped, episodes capped at ``--max_episode_length``
agent steps) with the published actor weights, refreshed every ``--eval-interval`` learner steps
(``engine.host_eval``).  ``--eval-mode async`` (default) steps them in ``--eval-workers`` worker
processes of their own and pumps the evaluator once per training iteration without ever waiting for
it; ``--eval-mode step`` steps in-process emulators for ``--eval-steps`` blocking evaluator steps per
interval (deterministic; tests and A/Bs).  ``--eval-kernel {fused,step}`` picks the one-launch act or
the stepwise yardstick.  Evaluator env ``j`` is seeded ``seed + 1,000,003 + j``.  When episodes
finished since the last log line: ``evaluator/episode_reward`` (game score), ``evaluator/episode_length``,
``evaluator/episodes``, ``evaluator/capped_episodes`` and ``evaluator/steps``.
"""
from __future__ import annotations

import os
import sys
import time

from .config import args_to_config, build_parser, preset


def parser():
    p = build_parser(preset("origin"), description="Ape-X DQN on MI355X over host gym-API Atari envs")
    p.add_argument("--envs", type=int, default=16, help="host emulators stepped per actor step")
    p.add_argument("--learner-steps", type=int, default=1, help="learner steps enqueued per env step (k >= 0)")
    p.add_argument("--workers", type=int, default=0,
                   help="emulator worker processes (0 = step the envs in this process)")
    p.add_argument("--worker-timeout", type=float, default=60.0,
                   help="seconds a worker may take for one step before the run is aborted")
    p.add_argument("--ingest", choices=["auto", "whole", "banked"], default="auto",
                   help="with --workers: ingest each worker's envs as they finish (banked) or all at once (whole)")
    p.add_argument("--eval-envs", type=int, default=0, help="greedy evaluator emulators (0 = no evaluator; at most 64)")
    p.add_argument("--eval-workers", type=int, default=1, help="evaluator worker processes (--eval-mode async)")
    p.add_argument("--eval-interval", type=int, default=100, help="learner steps between evaluator weight refreshes")
    p.add_argument("--eval-mode", choices=["async", "step"], default="async",
                   help="async: worker pool pumped every iteration; step: in-process, blocking, deterministic")
    p.add_argument("--eval-steps", type=int, default=64, help="evaluator steps per interval (--eval-mode step)")
    p.add_argument("--eval-kernel", choices=["fused", "step"], default="fused",
                   help="fused: one-launch act (host_eval_act); step: the stepwise forward")
    p.add_argument("--save-path", default="model.pth")
    p.add_argument("--resume", default=None, help="model.pth (+ .train.pt sidecar) to resume from")
    from .train import add_state_flags

    add_state_flags(p)
    p.add_argument("--log-dir", default=None, help="event-file directory (default runs/<time>-<env>-host)")
    p.add_argument("--no-tb", action="store_true")
    return p


def main(argv=None) -> int:
    import torch   # (not at module level: a worker process re-imports the main module, and stays torch-free)

    args = parser().parse_args(argv)
    if args.workers < 0:
        raise SystemExit("--workers must be >= 0")
    if not 0 <= args.eval_envs <= 64:
        raise SystemExit("--eval-envs must be in [0, 64]")
    if args.eval_envs and (args.eval_interval < 1 or args.eval_steps < 1 or
                           not 1 <= args.eval_workers <= args.eval_envs):
        raise SystemExit("--eval-interval / --eval-steps must be >= 1 and --eval-workers in [1, --eval-envs]")
    from .train import check_state_flags

    check_state_flags(args, int(os.environ.get("WORLD_SIZE", "1")))
    cfg = args_to_config(args)
    if not torch.cuda.is_available():
        raise SystemExit("apex_amd.train_host runs the GPU engine; use apex_amd.roles.* on CPU")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)

    from .envs.core import make
    from .envs.preprocess import PreprocessSpec
    from .envs.raw_vector import RawAtariVector

    spec = PreprocessSpec.from_args(cfg.env)
    if args.workers:
        from .envs.proc_vector import ProcRawAtariVector

        vec = ProcRawAtariVector(cfg.env.env, args.envs, spec, workers=args.workers, seed=cfg.seed,
                                 timeout=args.worker_timeout)
    else:
        vec = RawAtariVector([make(cfg.env.env) for _ in range(args.envs)], spec)
        vec.seed(cfg.seed)
    try:
        return _train(args, cfg, vec, spec, device)
    finally:   # every exit path, exceptions included: stop the workers, unlink their shared block
        close = getattr(vec, "close", None)
        if close is not None:
            close()


def _train(args, cfg, vec, spec, device) -> int:
    import torch

    from .engine.host_env import HostEnvConfig, HostEnvEngine
    from .engine.learner import LearnerConfig
    from .train import load_engine, save_engine

    L, R = cfg.learner, cfg.replay
    lc = LearnerConfig(batch_size=R.batch_size, n_step=cfg.n_steps, gamma=cfg.gamma, lr=L.lr, rms_alpha=L.rms_alpha,
                       rms_eps=L.rms_eps, centered=L.centered, max_norm=L.max_norm, lr_gamma=L.lr_gamma,
                       lr_step_size=L.lr_step_size, beta=R.beta, optimizer=L.optimizer, forward=cfg.kernel.forward,
                       dtype=cfg.kernel.dtype, seed=cfg.seed)
    ecfg = HostEnvConfig(replay_capacity=R.replay_buffer_size, alpha=R.alpha, threshold_size=R.threshold_size,
                         learner_steps_per_actor_step=args.learner_steps,
                         publish_param_interval=L.publish_param_interval,
                         target_update_interval=L.target_update_interval, nstep_mode=cfg.actor.nstep_mode,
                         eps_base=cfg.actor.eps_base, eps_alpha=cfg.actor.eps_alpha,
                         clip_rewards=bool(cfg.env.clip_rewards), action_repeat=spec.skip,
                         use_graphs=cfg.kernel.use_graphs, exact_mass=R.exact_mass, seed=cfg.seed,
                         ingest=args.ingest if args.workers else "auto", learner=lc)
    eng = HostEnvEngine(ecfg, vec, device)
    evaluation = None
    try:
        evaluation = _make_evaluation(args, cfg, spec, eng, device)
        return _loop(args, cfg, eng, device, evaluation)
    finally:
        if evaluation is not None:
            evaluation.close()   # side stream drained, staging unregistered, evaluator pool closed
        eng.close()   # unregisters the shared staging block, then closes the pool that owns it


def _make_evaluation(args, cfg, spec, eng, device):
    """The evaluator of ``--eval-envs`` emulators (None when off): a :class:`HostEnvEvaluation` over
    its own worker pool (async) or a :class:`HostEvaluator` over in-process emulators (step)."""
    if not args.eval_envs:
        return None
    from .engine.host_eval import HostEnvEvaluation, HostEvaluator, eval_seed

    cap, sd = int(cfg.env.max_episode_length), eval_seed(cfg.seed)
    if args.eval_mode == "step":
        from .envs.core import make
        from .envs.raw_vector import RawAtariVector

        vec = RawAtariVector([make(cfg.env.env) for _ in range(args.eval_envs)], spec, max_episode_steps=cap)
        vec.seed(sd)
        return HostEvaluator(eng.actor_model, vec, device, kernel=args.eval_kernel, seed=sd)
    from .envs.proc_vector import ProcRawAtariVector

    pool = ProcRawAtariVector(cfg.env.env, args.eval_envs, spec, workers=args.eval_workers, seed=sd,
                              timeout=args.worker_timeout, max_episode_steps=cap)
    try:
        return HostEnvEvaluation(HostEvaluator(eng.actor_model, pool, device, kernel=args.eval_kernel, seed=sd), pool)
    except BaseException:
        pool.close()
        raise


def _loop(args, cfg, eng, device, evaluation=None) -> int:
    import torch

    from .train import load_engine, resume_state, save_engine

    L, vec = cfg.learner, eng.vec
    counters = {}
    if args.resume:
        counters = load_engine(eng.learner, args.resume)
        eng.publish_params()
    start = int(counters.get("learn_steps", 0))
    eng.learn_steps = start
    if args.resume_state:
        start = resume_state(eng, args.resume_state)
    where = f" in {args.workers} worker processes ({eng.ingest} ingest)" if args.workers else ""
    print(f"{cfg.env.env}: {len(vec)} host envs{where}, {vec.n_actions} actions, raw {vec.raw_shape}; "
          f"training from step {start}", flush=True)

    writer = None
    if not args.no_tb:
        from .utils.tb import SummaryWriter

        writer = SummaryWriter(args.log_dir, comment=f"-{cfg.env.env}-host")
    max_step = int(L.max_step)
    bps_every = max(1, L.bps_interval)
    t_last, step_last, act_last, next_log = time.perf_counter(), start, eng.actor_steps, start + bps_every
    next_state = (start // args.save_state_interval + 1) * args.save_state_interval if args.save_state_interval else None
    next_save = (start // L.save_interval + 1) * L.save_interval if L.save_interval else None
    next_refresh = start + args.eval_interval
    ev_core = getattr(evaluation, "ev", evaluation)   # the HostEvaluator (its ledger holds the totals)
    if evaluation is not None:
        print(f"evaluator: {args.eval_envs} greedy host envs, {args.eval_mode} mode, {args.eval_kernel} act kernel",
              flush=True)
    state_saved_at = None
    while not max_step or eng.learn_steps < max_step:
        eng.iteration()
        step = eng.learn_steps
        if evaluation is not None:
            ev_core.learn_step = step
            # (a refused refresh -- the target set is still read -- is simply tried again next iteration)
            if step >= next_refresh and evaluation.refresh(eng.actor_flat, eng.actor_net):
                next_refresh = step + args.eval_interval
                if args.eval_mode == "step":
                    evaluation.run(args.eval_steps)
            if args.eval_mode == "async":
                evaluation.pump()
        if step >= next_log:
            next_log = step + bps_every
            st = eng.stats()  # (synchronises)
            now = time.perf_counter()
            dt = now - t_last
            line = {"learner/loss": st["loss"], "learner/grad_norm": st["grad_norm"],
                    "learner/grad_norm_l2": st["grad_norm_l2"], "learner/BPS": (step - step_last) / dt,
                    "actor/frames_per_sec": (eng.actor_steps - act_last) * eng.frames_per_actor_step / dt}
            if "episode_reward" in st:
                line["actor/episode_reward"] = st["episode_reward"]
                line["actor/episode_length"] = st["episode_length"]
                line["actor/episode_score"] = st["episode_score"]
            line["replay/size"] = float(st["replay_size"])
            done_eps = evaluation.poll() if evaluation is not None else []
            if done_eps:
                n = float(len(done_eps))
                line["evaluator/episode_reward"] = sum(e[0] for e in done_eps) / n
                line["evaluator/episode_length"] = sum(e[1] for e in done_eps) / n
                line["evaluator/episodes"] = float(ev_core.ledger.episodes)
                line["evaluator/capped_episodes"] = float(ev_core.ledger.capped)
                line["evaluator/steps"] = float(ev_core.ledger.steps)
            t_last, step_last, act_last = now, step, eng.actor_steps
            print(f"Step: {step} " + " ".join(f"{k}={v:.4g}" for k, v in line.items()), flush=True)
            if writer is not None:
                for k, v in line.items():
                    writer.add_scalar(k, v, step)
        if next_save is not None and step >= next_save:
            next_save = (step // L.save_interval + 1) * L.save_interval
            print("Saving Model..", flush=True)
            save_engine(eng.learner, args.save_path, {"learn_steps": step, "actor_steps": eng.actor_steps})
        if next_state is not None and step >= next_state:
            next_state = (step // args.save_state_interval + 1) * args.save_state_interval
            eng.save_state(args.state_dir)
            state_saved_at = step
    torch.cuda.synchronize(device)
    save_engine(eng.learner, args.save_path, {"learn_steps": eng.learn_steps, "actor_steps": eng.actor_steps})
    if args.state_dir and state_saved_at != eng.learn_steps:
        eng.save_state(args.state_dir)
    if writer is not None:
        writer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
