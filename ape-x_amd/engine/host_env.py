"""The fused Ape-X engine over HOST environments: gym-API Atari emulators stepped on the CPU
under the HBM replay, the on-device n-step batcher and the fused learner of
:mod:`apex_amd.engine.apex`.

``ActorShard`` hard-wires the GPU sprite game.  :class:`HostEnvShard` is the same shard with a
different front end: a raw vector env (:mod:`apex_amd.envs.raw_vector` protocol) hands over the
two unpooled RGB frames of every env's observation, one H2D copy moves them, and one kernel
(``host_env_ingest``, ops/csrc/host_env_kernels.hip) does the pixel work of the host pipeline --
max-pool, grey, fp64 area resize, round, transpose -- straight into the frame ring at the slot
``vec_env_step`` would have written, with the same reward / done / new_frame / ep_log outputs.
The actor forward with its eps-greedy epilogue, ``nstep_emit``, ``write_batch`` and the
learner graph are shared with the GPU-env engine, unchanged.

:class:`HostEnvEngine` overlaps the two sides on ONE stream: per iteration it enqueues the
actor forward, copies the actions out, enqueues ``k`` learner steps, and only then steps the
emulators on the host -- the GPU trains while the CPU emulates.

Emulator worker processes live behind the vector-env protocol
(:class:`apex_amd.envs.proc_vector.ProcRawAtariVector`); what this module adds for them is the
device side of a pool.  A vector env that exposes ``staging`` (its shared ``[N, 2, H, W, 3]``
block) is read in place: the shard registers the block with HIP and copies out of it with
``memcpy_h2d_async`` on the engine's stream, so no host memcpy moves the pairs into a second
pinned buffer.  A vector env that exposes ``banks`` and ``step_async`` / ``wait_bank`` is ingested
bank by bank (``HostEnvConfig.ingest``): each worker's env range gets its own H2D copies and one
ranged ``host_env_ingest_range`` launch as soon as that worker is done, while the other workers
are still emulating.  A range launch writes exactly what the whole launch writes for its envs, so
the banked, the whole and the in-process paths fill the ring and the replay identically.

Greedy evaluation on further host emulators beside training (the reference's ``eval.py``) is
:mod:`apex_amd.engine.host_eval`; it shares :class:`Ingest` and touches nothing here.

Out of scope here: double-banked env groups (stepping one half of the envs while the other
half's forward runs) and the multi-GPU topologies (``parallel/``, ``engine/central.py``).
"""
from __future__ import annotations

import copy
import time
import weakref
from dataclasses import dataclass, field

import numpy as np
import torch

from .. import ops
from ..envs.preprocess import area_weights
from ..models.dqn import DuelingDQN
from ..utils.checkpoint import save_model
from .graphs import capture_graph, warm_up
from .hbm_replay import HBMReplay
from .learner import DQNLearner, LearnerConfig
from .shard import ActorPolicy, NStepShard

OUT = 84          # the warp's output side (kHostEnvOut)
TAP_WIDTH = 8     # weights per output index in the tap tables (kHostEnvTaps)
INGEST_MODES = ("auto", "whole", "banked")


def has_banks(vec) -> bool:
    """Does ``vec`` offer the banked form (``banks``, ``step_async``, ``wait_bank``)?"""
    return all(hasattr(vec, a) for a in ("banks", "step_async", "wait_bank"))


def _unregister(hip, ptr: int, keep) -> None:
    """Finalizer of a registered staging block (``keep`` holds the mapping until here)."""
    try:
        hip.host_unregister(ptr)
    except RuntimeError:
        pass


# ---------------------------------------------------------------------------- tap tables
def tap_tables(n_in: int, n_out: int = OUT, width: int = TAP_WIDTH):
    """``area_weights(n_out, n_in)`` in compact form: (first [n_out] int32, count [n_out] int32,
    weight [n_out, width] float64) -- output ``o`` reads inputs ``first[o] .. first[o] + count[o] - 1``.
    The weights are the dense matrix's own values, so the dense rebuild is exact."""
    if n_in < n_out:
        raise ValueError(f"the warp only shrinks: {n_in} input pixels < {n_out} output pixels")
    w = area_weights(n_out, n_in)
    nz = w > 0
    first = nz.argmax(1)
    last = n_in - 1 - nz[:, ::-1].argmax(1)
    count = last - first + 1
    if int(count.max()) > width:
        raise ValueError(f"{int(count.max())} taps per output pixel ({n_in} -> {n_out}) exceed the table width {width}")
    weight = np.zeros((n_out, width), dtype=np.float64)
    for o in range(n_out):
        weight[o, :count[o]] = w[o, first[o]:first[o] + count[o]]
    return first.astype(np.int32), count.astype(np.int32), weight


def dense_from_taps(first, count, weight, n_in: int) -> np.ndarray:
    """The dense [n_out, n_in] matrix a tap table stands for."""
    w = np.zeros((len(first), n_in), dtype=np.float64)
    for o in range(len(first)):
        w[o, first[o]:first[o] + count[o]] = weight[o, :count[o]]
    return w


class Ingest:
    """Device tap tables + params of ``host_env_ingest`` for one (H, W, ring) geometry, and the
    launch.  Construction raises ``ValueError`` for H or W below 84 or an over-wide tap count."""

    def __init__(self, E: int, H: int, W: int, frame_bytes: int, frame_capacity: int, clip_rewards: bool, device):
        tabs = [tap_tables(H), tap_tables(W)]  # (raises before the device is touched)
        self.hip = ops.hip()
        assert self.hip.HOST_ENV_TAPS == TAP_WIDTH
        self._keep = []
        self.taps = []
        for first, count, weight in tabs:
            t = [torch.from_numpy(a).to(device) for a in (first, count, weight)]
            self._keep.append(t)
            self.taps.append(self.hip.make_host_env_taps(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                                         int(count.max())))
        self.params = self.hip.HostEnvParams(E, frame_bytes, frame_capacity, int(clip_rewards), H, W)

    def __call__(self, raw, reward_in, done_in, frames, step_counter, reset: bool, reward, done, new_frame, hist, acc,
                 ep_log) -> None:
        self.hip.host_env_ingest(raw.data_ptr(), reward_in.data_ptr(), done_in.data_ptr(), self.taps[0], self.taps[1],
                                 frames.data_ptr(), self.params, step_counter.data_ptr(), bool(reset),
                                 reward.data_ptr(), done.data_ptr(), new_frame.data_ptr(), hist.data_ptr(),
                                 acc.data_ptr(), ep_log.data_ptr(), torch.cuda.current_stream().cuda_stream)

    def range(self, e0: int, n: int, raw, reward_in, done_in, frames, step_counter, reset: bool, reward, done,
              new_frame, hist, acc, ep_log) -> None:
        """The same launch over envs ``[e0, e0 + n)``; every tensor is the whole shard's."""
        self.hip.host_env_ingest_range(raw.data_ptr(), reward_in.data_ptr(), done_in.data_ptr(), self.taps[0],
                                       self.taps[1], frames.data_ptr(), self.params, step_counter.data_ptr(),
                                       bool(reset), reward.data_ptr(), done.data_ptr(), new_frame.data_ptr(),
                                       hist.data_ptr(), acc.data_ptr(), ep_log.data_ptr(), int(e0), int(n),
                                       torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------- shard
class HostEnvShard(NStepShard):
    """``ActorShard``'s interface (the :class:`NStepShard` state, ``act_args()``, ``select()``,
    ``observe()``, ``episode_stats()``) over a host vector env.  ``ep_log`` column 3 is the
    episode's unclipped score."""

    def __init__(self, replay, n_envs: int, n_actions: int, raw_shape, n_step: int = 3, gamma: float = 0.99,
                 eps_base: float = 0.4, eps_alpha: float = 7.0, actor_offset: int = 0, total_actors: int | None = None,
                 seed: int = 0, mode: str = "reference", clip_rewards: bool = True, staging=None,
                 ingest: str = "auto"):
        if ingest not in INGEST_MODES:
            raise ValueError(f"ingest must be one of {INGEST_MODES}, got {ingest!r}")
        self.ingest_mode = ingest
        E = int(n_envs)
        H, W, C = (int(x) for x in raw_shape)
        if C != 3:
            raise ValueError("raw emulator frames must be RGB [H, W, 3]")
        dev = replay.device
        # (first: bad geometry raises before the shard allocates anything on the device)
        self.ingest = Ingest(E, H, W, replay.frame_bytes, replay.frame_capacity, clip_rewards, dev)
        super().__init__(replay, E, n_actions, n_step, gamma, eps_base, eps_alpha, actor_offset, total_actors, seed,
                         mode)
        f32 = dict(dtype=torch.float32, device=dev)
        self.acc = torch.zeros(E, 4, **f32)      # running (return, raw return, length, -) per env
        self.obs = torch.zeros(E, 4, 84, 84, dtype=torch.uint8, device=dev)
        # host staging (pinned: the copies below are truly asynchronous) and the device twins
        self._registered = None
        if staging is None:
            self.raw_host = torch.zeros(E, 2, H, W, 3, dtype=torch.uint8).pin_memory()
            self.raw_np = self.raw_host.numpy()
        else:
            # the vector env's own shared block, registered with HIP and read in place
            if tuple(staging.shape) != (E, 2, H, W, 3) or staging.dtype != np.uint8 or not staging.flags.c_contiguous:
                raise ValueError(f"staging must be a contiguous uint8 {(E, 2, H, W, 3)} array")
            self.raw_host = None
            self.raw_np = staging
            self.raw_ptr = int(staging.ctypes.data)
            self.hip.host_register(self.raw_ptr, int(staging.nbytes))
            self._registered = weakref.finalize(self, _unregister, self.hip, self.raw_ptr, staging)
        self.pair_bytes = 2 * H * W * 3
        self.raw_dev = torch.zeros(E, 2, H, W, 3, dtype=torch.uint8, device=dev)
        self.reward_host = torch.zeros(E, dtype=torch.float32).pin_memory()
        self.done_host = torch.zeros(E, dtype=torch.float32).pin_memory()
        self.actions_host = torch.zeros(E, dtype=torch.int32).pin_memory()
        self.reward_in = torch.zeros(E, **f32)
        self.done_in = torch.zeros(E, **f32)
        self.event = torch.cuda.Event()
        self.raw_bytes_per_step = self.raw_dev.numel() + 8 * E

    def _ingest(self, reset: bool) -> None:
        self.ingest(self.raw_dev, self.reward_in, self.done_in, self.replay.frames, self.step_counter, reset,
                    self.reward, self.done, self.new_frame, self.st["hist"], self.acc, self.ep_log)

    def _banked(self, vec) -> bool:
        """Ingest bank by bank?  ``auto`` says yes whenever ``vec`` offers banks."""
        if self.ingest_mode == "whole" or self._registered is None:
            return False
        return has_banks(vec)

    def _ship(self, e0: int, e1: int, reset: bool) -> None:
        """Envs ``[e0, e1)`` of the registered staging block: their H2D copies (pairs; reward and
        done slices on a step) and one ingest launch over the range, on the current stream."""
        s = torch.cuda.current_stream().cuda_stream
        off = e0 * self.pair_bytes
        self.hip.memcpy_h2d_async(self.raw_dev.data_ptr() + off, self.raw_ptr + off, (e1 - e0) * self.pair_bytes, s)
        if not reset:
            self.reward_in[e0:e1].copy_(self.reward_host[e0:e1], non_blocking=True)
            self.done_in[e0:e1].copy_(self.done_host[e0:e1], non_blocking=True)
        if e0 == 0 and e1 == self.E:
            self._ingest(reset)
        else:
            self.ingest.range(e0, e1 - e0, self.raw_dev, self.reward_in, self.done_in, self.replay.frames,
                              self.step_counter, reset, self.reward, self.done, self.new_frame, self.st["hist"],
                              self.acc, self.ep_log)

    def reset(self, vec) -> None:
        """Start every env; the start frames fill the stacks (``vec_env_reset``'s outputs).  The
        copy out of the pinned buffer is ordered like a step's (see :meth:`finish`).  With a
        registered staging block the pairs take a step's path: per bank, or as one range."""
        vec.reset(self.raw_np)
        if self._registered is None:
            self.raw_dev.copy_(self.raw_host, non_blocking=True)
            self._ingest(True)
            return
        for e0, e1 in (vec.banks if self._banked(vec) else [(0, self.E)]):
            self._ship(e0, e1, True)

    def observe(self) -> torch.Tensor:
        """Current stacked observations u8 [E,4,84,84] (gathered from the frame ring)."""
        self.replay.gather_frames(self.st["hist"], self.obs)
        return self.obs

    def begin(self) -> None:
        """After the forward picked ``self.actions``: start their copy to the host and mark the
        point the host has to wait for."""
        self.actions_host.copy_(self.actions, non_blocking=True)
        self.event.record()

    def finish(self, vec) -> None:
        """Wait for the actions, step the host envs, ship the pairs and run the device half of
        the actor step (ingest, n-step emit, tree write; the write advances ``step_counter``).

        One staging buffer is enough: iteration t's H2D copies are enqueued BEFORE iteration
        t+1's forward on the same stream, and the host waits for the event recorded after that
        forward before it writes the pinned buffers again -- when the wait returns, every copy
        that read them has completed.  (The same holds for the pinned reward / done / actions
        buffers, and for the copy :meth:`reset` starts.)

        The invariant keeps holding with worker processes and a registered shared staging block:
        the workers are told to step (``step_async``) only after the host has waited for the event
        recorded after the next forward, and by then every copy that read the staging block has
        completed.  Within a step, a bank's copy reads only that bank's env range, which its
        worker has finished writing; it may run while the other workers still write their own,
        disjoint ranges.  Banked ingest: for each bank, in completion order, its H2D copies and
        one ranged ingest launch; ``nstep_emit`` and ``write_batch`` follow once all banks are in."""
        self.event.synchronize()
        if self._registered is None:
            r, d = vec.step(self.actions_host.numpy(), self.raw_np)
            self.reward_host.numpy()[:] = r
            self.done_host.numpy()[:] = d
            self.raw_dev.copy_(self.raw_host, non_blocking=True)
            self.reward_in.copy_(self.reward_host, non_blocking=True)
            self.done_in.copy_(self.done_host, non_blocking=True)
            self._ingest(False)
        elif self._banked(vec):
            vec.step_async(self.actions_host.numpy())
            rh, dh = self.reward_host.numpy(), self.done_host.numpy()
            for _ in vec.banks:
                b, r, d = vec.wait_bank()
                e0, e1 = vec.banks[b]
                rh[e0:e1] = r
                dh[e0:e1] = d
                self._ship(e0, e1, False)
        else:
            r, d = vec.step(self.actions_host.numpy(), self.raw_np)   # (out is the staging block: no copy)
            self.reward_host.numpy()[:] = r
            self.done_host.numpy()[:] = d
            self._ship(0, self.E, False)
        self._emit(self.nstep, self.slot, self.prio, False)
        self.replay.write_batch(pre=(self.slot, self.prio, self.replay.filled), bump=self.step_counter)

    def close(self) -> None:
        """Let go of a registered staging block: wait for the copies that read it, unregister
        it, drop the view.  Call before the vector env unlinks the block; idempotent."""
        if self._registered is not None and self._registered.alive:
            torch.cuda.synchronize(self.device)
            self._registered()
        self.raw_np = None

    def step_host(self, vec) -> None:
        """Both halves back to back (``self.actions`` already chosen)."""
        self.begin()
        self.finish(vec)

    def episode_scores(self) -> torch.Tensor:
        """Last episode's unclipped score per env (``ep_log`` column 3)."""
        return self.ep_log[:, 3]


# ---------------------------------------------------------------------------- engine
@dataclass
class HostEnvConfig:
    """The ``EngineConfig`` fields that apply to host envs; ``n_envs`` / ``n_actions`` come from
    the vector env."""
    replay_capacity: int = 2_000_000
    alpha: float = 0.6
    threshold_size: int = 50_000
    learner_steps_per_actor_step: int = 1     # k >= 0 learner steps enqueued per iteration
    publish_param_interval: int = 25
    target_update_interval: int = 2500
    nstep_mode: str = "reference"
    eps_base: float = 0.4
    eps_alpha: float = 7.0
    actor_offset: int = 0
    total_actors: int | None = None
    clip_rewards: bool = True
    action_repeat: int = 4                    # emulator frames per env step (frames/s accounting only)
    use_graphs: bool = True
    warmup_learner_steps: int = 3             # eager learner steps before the graph is captured
    exact_mass: bool = False
    seed: int = 1122
    # how a vector env with worker banks is ingested: "banked" = per-bank copies + ranged launches in
    # completion order, "whole" = wait for every bank, then one copy and one launch, "auto" = banked
    # when the vector env offers banks.  The in-process vector (no banks) is not affected.
    ingest: str = "auto"
    learner: LearnerConfig = field(default_factory=LearnerConfig)


class HostEnvEngine:
    def __init__(self, cfg: HostEnvConfig, vec, device: str | torch.device = "cuda", model=None):
        k = cfg.learner_steps_per_actor_step
        if not isinstance(k, int) or isinstance(k, bool) or k < 0:
            raise ValueError("learner_steps_per_actor_step must be an int >= 0")
        if cfg.ingest not in INGEST_MODES:
            raise ValueError(f"ingest must be one of {INGEST_MODES}, got {cfg.ingest!r}")
        staging = getattr(vec, "staging", None)
        if cfg.ingest == "banked" and (staging is None or not has_banks(vec)):
            raise ValueError("ingest='banked' needs a vector env with staging, banks, step_async and wait_bank")
        self.cfg = cfg
        self.vec = vec
        self.device = torch.device(device)
        lc = cfg.learner
        E, A = len(vec), int(vec.n_actions)
        self.E, self.A = E, A
        torch.manual_seed(cfg.seed)
        self.replay = HBMReplay(cfg.replay_capacity, E, lc.n_step, cfg.alpha, self.device, exact_mass=cfg.exact_mass,
                                seed=cfg.seed)
        self.actor = HostEnvShard(self.replay, E, A, vec.raw_shape, lc.n_step, lc.gamma, cfg.eps_base, cfg.eps_alpha,
                                  cfg.actor_offset, cfg.total_actors, cfg.seed, cfg.nstep_mode, cfg.clip_rewards,
                                  staging=staging, ingest=cfg.ingest)
        self.ingest = "banked" if self.actor._banked(vec) else "whole"   # what "auto" resolved to
        model = model if model is not None else DuelingDQN.from_shapes((4, 84, 84), A)
        self.learner = DQNLearner(model, self.replay, lc)
        p = self.policy = ActorPolicy(copy.deepcopy(self.learner.model), E, A, self.device, lc.forward, lc.dtype,
                                      self.actor.q)
        self.actor_model, self.actor_flat, self.hip_net = p.model, p.flat, p.hip_net
        self.actor_net, self.actor_ws = p.net, p.ws   # (None without the HIP forward)
        self.publish_params()
        self.learn_steps = 0
        self.actor_steps = 0
        self._g_learn = None
        self._learning = False
        self.actor.reset(vec)

    # ------------------------------------------------------------------ bodies
    def publish_params(self) -> None:
        """Learner -> actor weights (``ApexEngine.publish_params``)."""
        self.policy.publish_from(self.learner)

    def _forward(self) -> None:
        q = self.policy.forward(self.replay, self.actor)
        if q is not None:  # (the HIP forward's heads kernel picked the actions itself)
            self.actor.select(q)

    def _learn_body(self) -> None:
        self.learner.forward_phase()
        self.learner.optimize()

    def _learner_step(self) -> None:
        if self._g_learn is not None:
            self._g_learn.replay()
        else:
            self._learn_body()
        self.learn_steps += 1
        if self.learn_steps % self.cfg.publish_param_interval == 0:
            self.publish_params()
        if self.learn_steps % self.cfg.target_update_interval == 0:
            self.learner.sync_target()

    def capture(self) -> None:
        """Warm up with ``warmup_learner_steps`` eager learner steps on a side stream (real
        steps, counted, cadences kept), then capture one learner step as a hipGraph.  The
        replay must hold transitions.  Called by :meth:`iteration` when learning starts; with
        ``use_graphs=False`` the same warm-up steps run and nothing is captured, so both
        modes execute the same sequence of steps."""
        if self._learning:
            return
        self._learning = True
        warm_up(self.device, self._learner_step, self.cfg.warmup_learner_steps)
        if not self.cfg.use_graphs:
            return
        torch.cuda.synchronize(self.device)
        # (capture records, it does not run: the step counters are untouched)
        self._g_learn = capture_graph(self._learn_body)

    def held(self) -> int:
        """Transitions in the replay, from the host's own count (no device read)."""
        return min(self.actor_steps * self.E, self.replay.capacity)

    def iteration(self) -> None:
        """Actor forward + action copy-out | k learner steps | host env step + device ingest.
        The learner steps are already queued when the host starts emulating; the host's only
        wait is for the event recorded right after the forward."""
        self._forward()
        self.actor.begin()
        k = self.cfg.learner_steps_per_actor_step
        if k and self.held() >= max(self.cfg.threshold_size, 1):
            if not self._learning:
                self.capture()
            for _ in range(k):
                self._learner_step()
        self.actor.finish(self.vec)
        self.actor_steps += 1

    def run(self, n_iterations: int) -> float:
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        for _ in range(n_iterations):
            self.iteration()
        torch.cuda.synchronize(self.device)
        return time.perf_counter() - t0

    # ------------------------------------------------------------------ reporting
    @property
    def frames_per_actor_step(self) -> int:
        return self.E * int(self.cfg.action_repeat)

    def stats(self) -> dict:
        """Host view of the learner's last step and the finished episodes (forces a sync)."""
        out = {"learn_steps": self.learn_steps, "actor_steps": self.actor_steps, "replay_size": len(self.replay)}
        if self.learn_steps:
            out.update(self.learner.stats())
        log = self.actor.ep_log.cpu()
        fin = log[:, 2] > 0
        out["episodes"] = int(log[:, 2].sum().item())
        if bool(fin.any()):
            out["episode_reward"] = float(log[fin, 0].mean())
            out["episode_length"] = float(log[fin, 1].mean())
            out["episode_score"] = float(log[fin, 3].mean())
        return out

    def state_dict(self):
        return self.learner.state_dict()

    def save(self, path: str) -> str:
        """``torch.save(state_dict)`` with the reference keys (utils/checkpoint.py)."""
        return save_model(self.learner.model, path)

    # ------------------------------------------------------------------ full-state checkpoints
    def state_tensors(self) -> dict[str, torch.Tensor]:
        """What a replay-preserving resume restores: the replay, the learner, the acting weights
        and the shard's step counter (it places the next frame and slot).  The emulators are host
        objects: env state, open n-step windows and the episode accumulators are not saved."""
        parts = {"replay": self.replay, "learner": self.learner, "policy": self.policy}
        out = {f"{c}.{k}": t for c, obj in parts.items() for k, t in obj.state_tensors().items()}
        out["actor.step_counter"] = self.actor.step_counter
        return out

    def state_geometry(self) -> dict:
        rp, lc = self.replay, self.cfg.learner
        return {"engine": "host_env", "capacity": rp.capacity, "frame_capacity": rp.frame_capacity,
                "frame_bytes": rp.frame_bytes, "E": self.E, "A": self.A, "n_step": self.actor.n,
                "batch": lc.batch_size, "params": self.learner.P, "forward": lc.forward, "dtype": lc.dtype}

    def host_state(self) -> dict:
        return {"learn_steps": self.learn_steps, "actor_steps": self.actor_steps, "actor_seed": self.actor.seed,
                "replay_seed": self.replay.seed, **self.learner.host_state()}

    def save_state(self, path: str, chunk_bytes: int = 64 << 20) -> dict:
        """Checkpoint the replay (live rows only), the learner, the acting weights and the
        counters as the directory ``path`` (utils/engine_state.py), between two iterations.
        Blocking.  The transitions still inside the open n-step windows (at most n * E rows) are
        not part of it: a resumed run starts its windows afresh."""
        from ..utils.engine_state import save_engine_state

        torch.cuda.synchronize(self.device)
        rows = {f"replay.{k}": n for k, n in self.replay.live_rows(self.actor.frames_written()).items()}
        tensors = {k: (t, rows[k]) if k in rows else t for k, t in self.state_tensors().items()}
        return save_engine_state(path, tensors, self.host_state(), self.state_geometry(), chunk_bytes)

    def load_state(self, path: str, chunk_bytes: int = 64 << 20) -> dict:
        """Replay-preserving resume: restore what :meth:`save_state` wrote into this engine (built
        with the same geometry over fresh envs), then start the envs afresh.  Not bit for bit --
        the emulators cannot be restored, and the rows inside the n-step windows that were open
        at save time (at most n * E) are lost.

        The frame ring and the slots advance in lockstep (a step with counter ``c`` writes frames
        ``(c + 1) * E + e`` and slots ``c * E + e``; a reset writes frames ``c * E + e``), so a
        reset at the restored counter would land on the newest frames, which the newest
        transitions reference.  One dead step is spent first: its E slots get priority 0 through
        the ordinary tree write (which advances ``filled`` and the step counter, as after a step
        whose windows emitted nothing), the n-step windows are cleared, and the reset then
        writes the frames that step would have written."""
        from ..utils.engine_state import check_covers, load_engine_state

        torch.cuda.synchronize(self.device)
        check_covers(path, {f"replay.{k}": n
                            for k, n in self.replay.live_rows(self.actor.frames_written()).items()})
        host = load_engine_state(path, self.state_tensors(), self.state_geometry(), chunk_bytes)
        keys = (self.actor.seed, self.replay.seed)
        self.learn_steps, self.actor_steps = int(host["learn_steps"]), int(host["actor_steps"])
        self.actor.load_host_state({"seed": host["actor_seed"]})
        self.replay.seed = int(host["replay_seed"])
        self.learner.load_host_state(host)
        self.learner.refresh_packed()
        self.learner.refresh_target_packed()
        self.policy.refresh_packed()
        a, rp = self.actor, self.replay
        step = int(a.step_counter.item())
        a.slot.copy_(((step * self.E + torch.arange(self.E, device=self.device)) % rp.capacity).to(torch.int32))
        a.prio.zero_()
        rp.write_batch(pre=(a.slot, a.prio, rp.filled), bump=a.step_counter)   # the dead step
        self.actor_steps += 1
        for t in a.st.values():
            t.zero_()
        a.acc.zero_()
        a.reset(self.vec)
        torch.cuda.synchronize(self.device)
        if self._g_learn is not None and keys != (a.seed, rp.seed):   # the draw key is a launch argument
            self._g_learn = capture_graph(self._learn_body)
            torch.cuda.synchronize(self.device)
        return host

    def close(self) -> None:
        """Finish the queued work, release the staging block and close a vector env that has a
        ``close`` (a worker pool: its processes stop, its shared block is unlinked).  Idempotent."""
        self.actor.close()
        close = getattr(self.vec, "close", None)
        if close is not None:
            close()
