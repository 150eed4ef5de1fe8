"""The GPU vector-observation Ape-X engine over HOST environments: gym-API envs stepped on the
CPU under the HBM replay, the acting forward and the fused MLP learner of
:mod:`apex_amd.engine.vector`.

:class:`~apex_amd.engine.vector.VectorApexEngine` hard-wires three env kinds into
``vec_classic_step``; the reference's ``ApeX.py`` takes any ``gym.make(env_id)`` with a flat
observation and a discrete action space.  :class:`VectorHostEngine` is the same engine with a
different env half of the acting step: a :class:`~apex_amd.envs.host_vector.HostVectorEnv` (or
any object of its protocol) steps the envs, one H2D copy moves its staging block, and one kernel
(``vec_host_tail``, ops/csrc/vector_host_kernels.hip) leaves the observation ring row, ``reward``,
``done``, ``new_frame`` and the episode log exactly where ``vec_classic_step`` would have.  The
n-step batcher, the tree write, ``vec_act`` (same seeds, same counter), the replay, the learner,
the cadences and the checkpoints are shared.

One acting step: ``vec_act`` -> the actions D2H into a pinned buffer + an event | the host waits
for the event and steps the envs | one ``memcpy_h2d_async`` of the staging block (out of its
pinned twin) -> ``vec_host_tail`` -> ``nstep_emit`` -> ``per_write_leaves``: 4 kernel
launches, 2 copies, 1 host wait.

``done`` is the env's own flag.  A length-cap reset (``ended`` set, ``done`` clear: the episode
reached ``max_episode_length`` without the env ending it) stores ``done = 0``, so the n-step
window runs on across the reset, as the reference's recorder does (batchrecorder.py:54-76: it
stores the env's flag and resets on ``done or episode_length >= max_episode_length``).  The
episode log counts such an episode all the same.

Iteration order.  ``host_overlap=False``: the K learner steps with their publish and target
cadences, then the acting step -- ``VectorApexEngine.train_step``'s order.
``host_overlap=True`` (default): ``act_begin`` (the acting forward and the action copy are
enqueued), then the K learner steps (the captured learner graph after
:meth:`VectorHostEngine.capture`), and only then ``act_finish``: the host waits for the actions
and steps the envs while the GPU trains; the staging copy, the tail, the batcher and the tree
write follow.  Everything is on ONE stream.  Two consequences:

* In both orders **the learner steps of iteration i sample the rows written through acting step
  i - 1**: the step acted in iteration i reaches the replay after that iteration's SGD steps.
* Overlapped, the action of step i is chosen before the publish of iteration i's learner steps:
  at a publish boundary the acting weights lag by one env step against the serial order.

One staging block and one action buffer are enough.  The host writes the staging block again
only after it has waited for the event recorded after the NEXT acting forward, which the same
stream runs after the copy that read the block.  The host reads the action buffer inside
``vec.step`` and enqueues the next action copy only after that call has returned.

Greedy evaluation is the host one: :meth:`VectorHostEngine.evaluate` (blocking: a CPU copy of the
online net on a separate env), or beside training :mod:`apex_amd.engine.vector_host_eval`
(evaluator envs in worker processes, ``vec_host_eval_act`` on a side stream, two weight sets, a
pump that never waits; ``train_vector --host-envs --eval-envs N``).  ``rollout_evaluate`` and
:class:`~apex_amd.engine.vector.VectorEvaluator` play device envs and are refused.  Out of scope:
worker processes for the TRAINING envs and the central topology.

Shapes: observations to 8 floats and 7 actions (``kVecMaxObs`` / ``kVecMaxA``) by default; with
``VectorEngineConfig.wide_net`` the acting forward and the learner are the MFMA kernels of
``ops/csrc/vector_wide_kernels.hip`` and the limits are 128 / 32 (``kVecWideMaxObs`` /
``kVecWideMaxA``); ``wide_dtype="bf16"`` takes them from ``ops/csrc/vector_wide_bf16_kernels.hip``
(``vecwb_*``: bf16 matrix-core operands, fp32 accumulation and master weights); ``tall_obs`` (with
``wide_net``, fp32) raises the observation limit to 1024 (``kVecTallMaxObs``) on the streamed kernels of
``ops/csrc/vector_tall_kernels.hip`` (``vect_*``), ``tall_dtype="bf16"`` takes those with bf16 operands
(``ops/csrc/vector_tall_bf16_kernels.hip``, ``vectb_*``), and ``ring_dtype="bf16"`` (with those) stores the
observation ring as bf16: ``vec_host_tail`` writes ``to_bf16`` of each staged row (nearest even, the rounding the
``vectb_*`` kernels apply to an fp32 row at every read), the replay holds ``2 * obs_dim`` bytes per observation, the
three kernels load the operand bits without converting, and every result is bit-equal to the fp32 ring's.  The
staging block, the evaluators and :meth:`VectorHostShard.observe` stay fp32.  The side-stream
evaluator follows the engine: over a wide engine its act is ``vecw_host_eval_act`` / ``vecwb_host_eval_act``
(:mod:`apex_amd.engine.vector_host_eval`, through the API; ``train_vector
--wide --eval-envs`` is still refused, the CLI's switch-over is a follow-up, so on the command line a
wide engine evaluates with the blocking :meth:`VectorHostEngine.evaluate`).
"""
from __future__ import annotations

import dataclasses
import time

import numpy as np
import torch

from .. import ops
from ..models.dqn import DuelingDQN
from .graphs import capture_graph
from .hbm_replay import HBMReplay
from .host_env import PinnedMirror
from .shard import NStepShard
from .vector import (DIST_MAX_ACTIONS, MLPDQNLearner, VectorEngineConfig, ring_bytes, save_state_dict, vec_net,
                     wide_kernel)

MAX_OBS = 8       # kVecMaxObs: the MLP kernels' widest observation
MAX_ACTIONS = 7   # kVecMaxA: their widest action set
WIDE_MAX_OBS = 128      # kVecWideMaxObs: the wide (MFMA) kernels' widest observation
WIDE_MAX_ACTIONS = 32   # kVecWideMaxA: their widest action set
TALL_MAX_OBS = 1024     # kVecTallMaxObs: the tall (streamed) mode of the wide kernels


def host_env_spec(vec, wide: bool = False, tall: bool = False) -> tuple[int, int, int | None]:
    """``(obs_dim, n_actions, max_episode_steps)`` of a vector env the MLP kernels can play
    (``max_episode_steps``: its registered TimeLimit, None if it has none); ``wide``: the limits
    of the wide kernels (``VectorEngineConfig.wide_net``); ``tall`` (with ``wide``): their tall mode's
    observation limit (``tall_obs``).  No GPU needed."""
    if tall and not wide:
        raise ValueError("tall is a mode of the wide kernels: pass wide=True")
    if getattr(vec, "continuous", False):
        raise ValueError("the vector Ape-X engine takes a discrete action space; a continuous (Box) one is AQL's "
                         "(engine/aql_host.py)")
    obs, n_actions = int(vec.obs_dim), int(vec.n_actions)
    max_obs, max_a, tag = (WIDE_MAX_OBS, WIDE_MAX_ACTIONS, "kVecWideMax") if wide else (MAX_OBS, MAX_ACTIONS, "kVecMax")
    if tall:
        max_obs = TALL_MAX_OBS
    if not 1 <= obs <= max_obs:
        raise ValueError(f"observation dim {obs} is outside the MLP kernels' limit of {max_obs} "
                         f"({'kVecTallMax' if tall else tag}Obs)")
    if not 1 <= n_actions <= max_a:
        raise ValueError(f"{n_actions} actions are outside the MLP kernels' limit of {max_a} ({tag}A)")
    lim = getattr(vec, "max_episode_steps", None)
    return obs, n_actions, None if lim is None else int(lim)


class VectorHostShard(NStepShard):
    """E host envs (a ``HostVectorEnv`` or an object of its protocol) over an ``HBMReplay`` whose
    frames are observations: the surface of :class:`~apex_amd.engine.vector.VectorActorShard`
    (``set_policy``, ``reset``, ``observe``, ``act``, ``episode_stats``) with the acting step in
    two halves, :meth:`act_begin` and :meth:`act_finish` (module docstring)."""

    def __init__(self, replay: HBMReplay, vec, n_step: int = 3, gamma: float = 0.99, eps_base: float = 0.4,
                 eps_alpha: float = 7.0, actor_offset: int = 0, total_actors: int | None = None, seed: int = 0,
                 mode: str = "reference", wide: bool = False, wide_dtype: str = "fp32", tall: bool = False,
                 tall_dtype: str = "fp32", ring_dtype: str = "fp32", dist: bool = False):
        self.vec = vec
        if dist and not wide:
            raise ValueError("the categorical act (vecd_act) is a mode of the wide kernels: pass wide=True")
        self.wide = bool(wide)   # act with vecw_act; the tail takes the wide observation limit
        self.tall = bool(tall)   # (wide) act with vect_act; the tail takes the tall observation limit
        self.obs_dim, n_actions, self.max_episode_steps = host_env_spec(vec, self.wide, self.tall)
        E = len(vec)
        if not 1 <= E <= 4096:
            raise ValueError("VectorHostShard: 1 <= envs <= 4096 (the actor step's one-launch tree write)")
        width = ring_bytes(ring_dtype)
        self.ring_bf16 = width == 2   # vec_host_tail rounds the row once; vectb_act reads the bits
        if self.ring_bf16 and not (self.wide and self.tall and tall_dtype == "bf16"):
            raise ValueError("ring_dtype='bf16' is a layout of the tall bf16 kernels: pass wide, tall and "
                             "tall_dtype='bf16'")
        if replay.frame_bytes != width * self.obs_dim:
            raise ValueError(f"replay frame_bytes must be {width} * obs_dim = {width * self.obs_dim}")
        super().__init__(replay, E, n_actions, n_step, gamma, eps_base, eps_alpha, actor_offset, total_actors, seed,
                         mode)
        # (vecwb_act for bf16, vect_act for tall, vecd_act for categorical heads)
        self._wide_act = (wide_kernel(self.hip, "act", wide_dtype, self.tall, tall_dtype, ring_dtype, dist=dist)
                          if self.wide else None)
        h, dev = self.hip, self.device
        self.ring = replay.frames.view(torch.bfloat16 if self.ring_bf16 else torch.float32)  # [F, obs_dim]
        self.ep_ret = torch.zeros(E, dtype=torch.float32, device=dev)
        self.ep_len = torch.zeros(E, dtype=torch.float32, device=dev)
        # the staging block, shipped through its pinned twin, and its device copy
        st = vec.staging
        n = E * (2 * self.obs_dim + 3)
        if not isinstance(st, np.ndarray) or st.dtype != np.float32 or st.shape != (n,) or not st.flags.c_contiguous:
            raise ValueError(f"staging must be a contiguous float32 array of {n} elements")
        self._staging = st
        self._stage_bytes = int(st.nbytes)
        self._mirror = PinnedMirror(st)
        self.stage_dev = torch.zeros(n, dtype=torch.float32, device=dev)
        self.act_host = torch.zeros(E, dtype=torch.int32).pin_memory()
        self._act_np = self.act_host.numpy()
        self.event = torch.cuda.Event()
        self._tail = h.make_vec_host_tail(dict(
            E=E, obs=self.obs_dim, F=replay.frame_capacity, stage=self.stage_dev.data_ptr(),
            ring=self.ring.data_ptr(), step=self.step_counter.data_ptr(), reward=self.reward.data_ptr(),
            done=self.done.data_ptr(), new_frame=self.new_frame.data_ptr(), hist=self.st["hist"].data_ptr(),
            ep_log=self.ep_log.data_ptr(), ep_ret=self.ep_ret.data_ptr(), ep_len=self.ep_len.data_ptr(),
            wide=self.wide, tall=self.tall, ring_bf16=self.ring_bf16))
        self._act = None
        self.env_steps = 0    # host env steps taken (all envs)
        self.host_seconds = 0.0   # wall time inside vec.step
        self.reset()

    def _enqueued(self) -> None:
        """Called after every enqueue of an acting step (the engine hooks its own in)."""

    def set_policy(self, model: DuelingDQN) -> None:
        """Act with ``model`` (its parameter storage is read in place by every later step)."""
        if model.input_shape != (self.obs_dim,) or model.num_actions != self.A:
            raise ValueError("policy shape does not match the env")
        self._policy = model
        make = self.hip.make_vecw_act if self.wide else self.hip.make_vec_act
        kw = dict(ring_bf16=True) if self.ring_bf16 else {}
        self._act = make(vec_net(self.hip, model), self.ring.data_ptr(), self.st["hist"].data_ptr(), self.E,
                         self.eps.data_ptr(), self.act_seed, self.step_counter.data_ptr(), self.q.data_ptr(),
                         self.actions.data_ptr(), **kw)

    def reset(self) -> None:
        """Start every host env; their first observations into the ring (the reset form of
        ``vec_host_tail``: ``vec_classic_reset``'s contract).  A blocking copy."""
        self.vec.reset()
        self.stage_dev.copy_(torch.from_numpy(self._staging))
        self.hip.vec_host_tail(self._tail, True, self._stream())

    def observe(self) -> torch.Tensor:
        """Current observations f32 [E, obs_dim] (a gather from the ring; allocates; over a bf16 ring the
        stored, rounded values as floats)."""
        return self.ring[self.st["hist"][:, 3].long()].float()

    def act(self) -> None:
        """Q of the current observations into ``self.q`` and the epsilon-greedy actions."""
        if self._act is None:
            raise RuntimeError("set_policy() first: acting needs the HIP forward's weights")
        (self._wide_act or self.hip.vec_act)(self._act, self._stream())

    def act_begin(self) -> None:
        """The acting forward, the actions on their way to the host, the event the host waits for."""
        self.act()
        self._enqueued()
        self.act_host.copy_(self.actions, non_blocking=True)
        self.event.record()
        self._enqueued()

    def act_finish(self) -> None:
        """Wait for the actions, step the host envs, ship the staging block, then the tail, the
        n-step batcher (it bumps the step counter) and the tree write."""
        h, s = self.hip, self._stream()
        self.event.synchronize()
        t0 = time.perf_counter()
        self.vec.step(self._act_np)
        self.host_seconds += time.perf_counter() - t0
        self.env_steps += self.E
        h.memcpy_h2d_async(self.stage_dev.data_ptr(), self._mirror.stage(), self._stage_bytes, s)
        self._enqueued()
        h.vec_host_tail(self._tail, False, s)
        self._enqueued()
        self._emit(self.nstep, self.slot, self.prio, True)
        self._enqueued()
        self.replay.write_priorities(self.slot, self.prio, dedup=False, bumps=((self.replay.filled, self.E),))
        self._enqueued()

    def act_and_step(self) -> None:
        self.act_begin()
        self.act_finish()

    def close(self) -> None:
        """Finish the queued work, release the staging block, close the vector env.  Idempotent."""
        if self._mirror.alive:
            torch.cuda.synchronize(self.device)
            self._mirror.release()
        close = getattr(self.vec, "close", None)
        if close is not None:
            close()


class VectorHostEngine:
    """Actors on host envs + observation-ring replay + MLP learner on one GPU (see the module
    docstring).  ``cfg.env_id`` is only a label and ``cfg.n_envs`` is ignored: shapes and the env
    count come from ``vec``.  ``learner_steps``: SGD steps per env step (host envs are the slow
    side).  ``eval_env``: the constructor of :meth:`evaluate`'s env (default:
    ``envs.make(cfg.env_id)``)."""

    def __init__(self, cfg: VectorEngineConfig, vec, device: str | torch.device = "cuda", learner_steps: int = 1,
                 host_overlap: bool = True, eval_env=None):
        if int(learner_steps) < 1:
            raise ValueError("learner_steps >= 1")
        if cfg.actor_steps_per_learner_step != 1:
            raise ValueError("a host-env engine takes one env step per iteration: set learner_steps, not "
                             "actor_steps_per_learner_step")
        self.obs_dim, self.A, self.limit = host_env_spec(vec, cfg.wide_net, cfg.tall_obs)
        self.cfg = cfg = dataclasses.replace(cfg, n_envs=len(vec)).validate(device_env=False)
        self.vec = vec
        self.K = int(learner_steps)
        self.host_overlap = bool(host_overlap)
        self.eval_env = eval_env
        self.device = dev = torch.device(device)
        self.hip = ops.hip()
        torch.manual_seed(cfg.seed)
        # (dist_atoms: categorical heads on the learner's model, the acting copy and evaluate()'s CPU copy)
        self._dist = dict(atoms=cfg.dist_atoms, v_min=cfg.v_min, v_max=cfg.v_max) if cfg.dist_atoms else {}
        if self._dist and self.A > DIST_MAX_ACTIONS:
            raise ValueError(f"dist_atoms takes up to {DIST_MAX_ACTIONS} actions, the env has {self.A}")
        model = DuelingDQN.from_shapes((self.obs_dim,), self.A, noisy=cfg.noisy_heads, **self._dist)
        self.replay = HBMReplay(cfg.replay_capacity, cfg.n_envs, cfg.n_step, cfg.alpha, dev,
                                frame_bytes=ring_bytes(cfg.ring_dtype) * self.obs_dim, seed=cfg.seed + 17)
        self.learner = MLPDQNLearner(model, self.replay, cfg)
        self.actor_model = DuelingDQN.from_shapes((self.obs_dim,), self.A, **self._dist).to(dev)
        self.actor_flat = self.actor_model.flatten_parameters()
        self.shard = VectorHostShard(self.replay, vec, cfg.n_step, cfg.gamma, cfg.eps_base, cfg.eps_alpha,
                                     seed=cfg.seed * 0x2545F491 + 0xAC7, mode=cfg.nstep_mode, wide=cfg.wide_net,
                                     wide_dtype=cfg.wide_dtype, tall=cfg.tall_obs, tall_dtype=cfg.tall_dtype,
                                     ring_dtype=cfg.ring_dtype, dist=bool(cfg.dist_atoms))
        self.shard._enqueued = lambda: self._enqueued()
        self.shard.set_policy(self.actor_model)
        self.publish_params()
        self.learn_steps = 0
        self.actor_steps = 0
        self._g_learn = None

    env_steps = property(lambda self: self.shard.env_steps)

    # ------------------------------------------------------------------ phases
    def _enqueued(self) -> None:
        """Called after every enqueue of an iteration (a test synchronizes here)."""

    def publish_params(self) -> None:
        self.learner.publish_to(self.actor_flat)   # (noisy_heads: composed with the acting copy's own noise)
        self._enqueued()

    def actor_step(self) -> None:
        self.shard.act_and_step()
        self.actor_steps += 1

    def learner_step(self) -> None:
        """One SGD step (the captured graph after :meth:`capture`) and its cadences."""
        if self._g_learn is not None:
            self._g_learn.replay()
        else:
            self.learner.step()
        self._enqueued()
        self.learn_steps += 1
        if self.learn_steps % self.cfg.publish_param_interval == 0:
            self.publish_params()
        if self.learn_steps % self.cfg.target_update_interval == 0:
            self.learner.sync_target()
            self._enqueued()

    def fill(self, min_transitions: int | None = None) -> None:
        """Act until the replay holds more than ``threshold_size`` slots (ApeX.py: learning
        starts once ``len(buffer) > batch_size``)."""
        thr = self.cfg.threshold_size if self.cfg.threshold_size is not None else self.cfg.batch_size
        need = (thr if min_transitions is None else int(min_transitions)) + 1
        # n-step rows trail the env steps: the first n steps of an env emit nothing
        steps = -(-need // self.cfg.n_envs) + self.cfg.n_step
        for _ in range(steps):
            self.actor_step()

    def train_step(self) -> None:
        """One iteration: one step of all host envs and ``learner_steps`` SGD steps, in the order
        ``host_overlap`` selects (module docstring)."""
        if self.host_overlap:
            self.shard.act_begin()
            for _ in range(self.K):
                self.learner_step()
            self.shard.act_finish()
        else:
            for _ in range(self.K):
                self.learner_step()
            self.shard.act_and_step()
        self.actor_steps += 1

    def capture(self, warmup_iters: int = 3) -> None:
        """``warmup_iters`` real, counted iterations (every learner kernel's first launch happens
        outside a capture), then the learner step as a hipGraph, replayed K times an iteration with
        the cadence checks between.  The acting step waits for the host: it stays eager."""
        for _ in range(warmup_iters):
            self.train_step()
        torch.cuda.synchronize(self.device)
        self._g_learn = capture_graph(self.learner.step)
        torch.cuda.synchronize(self.device)

    def save(self, path: str) -> str:
        """Reference-format ``state_dict`` of the online network."""
        return save_state_dict(self.learner.model, path)

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, episodes: int = 10, seed: int = 12345) -> list[float]:
        """Greedy (epsilon = 0) returns of ``episodes`` episodes on a separate host env from the
        same constructor, played by a CPU copy of the online net; an episode without an end of its
        own stops at the env's TimeLimit or the vector env's length cap."""
        from .. import envs

        env = self.eval_env() if self.eval_env is not None else envs.make(self.cfg.env_id)
        env.seed(int(seed))
        torch.cuda.synchronize(self.device)
        m = DuelingDQN.from_shapes((self.obs_dim,), self.A, noisy=self.cfg.noisy_heads, **self._dist)   # (eval: mu)
        m.load_state_dict({k: v.detach().cpu() for k, v in self.learner.model.state_dict().items()})
        m.eval()
        limit = int(getattr(env, "_max_episode_steps", None) or self.limit
                    or getattr(self.vec, "max_episode_length", None) or 10_000)
        out = []
        with torch.no_grad():
            for _ in range(int(episodes)):
                s, er = env.reset(), 0.0
                for _ in range(limit):
                    q = m(torch.as_tensor(np.asarray(s, dtype=np.float32).reshape(1, -1)))
                    s, r, d, _ = env.step(int(q.argmax(1).item()))
                    er += float(r)
                    if d:
                        break
                out.append(er)
        env.close()
        return out

    def rollout_evaluate(self, *a, **k):
        raise RuntimeError("rollout_evaluate plays vec_rollout's device envs; a host-env engine evaluates on the "
                           "host: VectorHostEngine.evaluate")

    def close(self) -> None:
        """Finish the queued work, release the staging block, close the vector env.  Idempotent."""
        self.shard.close()
