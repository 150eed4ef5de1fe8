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
for the event and steps the envs | one ``memcpy_h2d_async`` of the staging block (registered with
HIP, read in place) -> ``vec_host_tail`` -> ``nstep_emit`` -> ``per_write_leaves``: 4 kernel
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
worker processes for the TRAINING envs, wider nets than ``kVecMaxObs`` / ``kVecMaxA``, the central
topology.
"""
from __future__ import annotations

import dataclasses
import time
import weakref

import numpy as np
import torch

from .. import ops
from ..models.dqn import DuelingDQN
from .graphs import capture_graph
from .hbm_replay import HBMReplay
from .host_env import _unregister
from .shard import NStepShard
from .vector import MLPDQNLearner, VectorEngineConfig, save_state_dict, vec_net

MAX_OBS = 8       # kVecMaxObs: the MLP kernels' widest observation
MAX_ACTIONS = 7   # kVecMaxA: their widest action set


def host_env_spec(vec) -> tuple[int, int, int | None]:
    """``(obs_dim, n_actions, max_episode_steps)`` of a vector env the MLP kernels can play
    (``max_episode_steps``: its registered TimeLimit, None if it has none).  No GPU needed."""
    if getattr(vec, "continuous", False):
        raise ValueError("the vector Ape-X engine takes a discrete action space; a continuous (Box) one is AQL's "
                         "(engine/aql_host.py)")
    obs, n_actions = int(vec.obs_dim), int(vec.n_actions)
    if not 1 <= obs <= MAX_OBS:
        raise ValueError(f"observation dim {obs} is outside the MLP kernels' limit of {MAX_OBS} (kVecMaxObs)")
    if not 1 <= n_actions <= MAX_ACTIONS:
        raise ValueError(f"{n_actions} actions are outside the MLP kernels' limit of {MAX_ACTIONS} (kVecMaxA)")
    lim = getattr(vec, "max_episode_steps", None)
    return obs, n_actions, None if lim is None else int(lim)


class VectorHostShard(NStepShard):
    """E host envs (a ``HostVectorEnv`` or an object of its protocol) over an ``HBMReplay`` whose
    frames are observations: the surface of :class:`~apex_amd.engine.vector.VectorActorShard`
    (``set_policy``, ``reset``, ``observe``, ``act``, ``episode_stats``) with the acting step in
    two halves, :meth:`act_begin` and :meth:`act_finish` (module docstring)."""

    def __init__(self, replay: HBMReplay, vec, n_step: int = 3, gamma: float = 0.99, eps_base: float = 0.4,
                 eps_alpha: float = 7.0, actor_offset: int = 0, total_actors: int | None = None, seed: int = 0,
                 mode: str = "reference"):
        self.vec = vec
        self.obs_dim, n_actions, self.max_episode_steps = host_env_spec(vec)
        E = len(vec)
        if not 1 <= E <= 4096:
            raise ValueError("VectorHostShard: 1 <= envs <= 4096 (the actor step's one-launch tree write)")
        if replay.frame_bytes != 4 * self.obs_dim:
            raise ValueError(f"replay frame_bytes must be 4 * obs_dim = {4 * self.obs_dim}")
        super().__init__(replay, E, n_actions, n_step, gamma, eps_base, eps_alpha, actor_offset, total_actors, seed,
                         mode)
        h, dev = self.hip, self.device
        self.ring = replay.frames.view(torch.float32)  # [F, obs_dim]
        self.ep_ret = torch.zeros(E, dtype=torch.float32, device=dev)
        self.ep_len = torch.zeros(E, dtype=torch.float32, device=dev)
        # the staging block, registered with HIP and read in place, and its device copy
        st = vec.staging
        n = E * (2 * self.obs_dim + 3)
        if not isinstance(st, np.ndarray) or st.dtype != np.float32 or st.shape != (n,) or not st.flags.c_contiguous:
            raise ValueError(f"staging must be a contiguous float32 array of {n} elements")
        self._staging = st
        self._stage_ptr, self._stage_bytes = int(st.ctypes.data), int(st.nbytes)
        h.host_register(self._stage_ptr, self._stage_bytes)
        self._registered = weakref.finalize(self, _unregister, h, self._stage_ptr, st)
        self.stage_dev = torch.zeros(n, dtype=torch.float32, device=dev)
        self.act_host = torch.zeros(E, dtype=torch.int32).pin_memory()
        self._act_np = self.act_host.numpy()
        self.event = torch.cuda.Event()
        self._tail = h.make_vec_host_tail(dict(
            E=E, obs=self.obs_dim, F=replay.frame_capacity, stage=self.stage_dev.data_ptr(),
            ring=self.ring.data_ptr(), step=self.step_counter.data_ptr(), reward=self.reward.data_ptr(),
            done=self.done.data_ptr(), new_frame=self.new_frame.data_ptr(), hist=self.st["hist"].data_ptr(),
            ep_log=self.ep_log.data_ptr(), ep_ret=self.ep_ret.data_ptr(), ep_len=self.ep_len.data_ptr()))
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
        self._act = self.hip.make_vec_act(vec_net(self.hip, model), self.ring.data_ptr(), self.st["hist"].data_ptr(),
                                          self.E, self.eps.data_ptr(), self.act_seed,
                                          self.step_counter.data_ptr(), self.q.data_ptr(), self.actions.data_ptr())

    def reset(self) -> None:
        """Start every host env; their first observations into the ring (the reset form of
        ``vec_host_tail``: ``vec_classic_reset``'s contract).  A blocking copy."""
        self.vec.reset()
        self.stage_dev.copy_(torch.from_numpy(self._staging))
        self.hip.vec_host_tail(self._tail, True, self._stream())

    def observe(self) -> torch.Tensor:
        """Current observations f32 [E, obs_dim] (a gather from the ring; allocates)."""
        return self.ring[self.st["hist"][:, 3].long()]

    def act(self) -> None:
        """Q of the current observations into ``self.q`` and the epsilon-greedy actions."""
        if self._act is None:
            raise RuntimeError("set_policy() first: acting needs the HIP forward's weights")
        self.hip.vec_act(self._act, self._stream())

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
        h.memcpy_h2d_async(self.stage_dev.data_ptr(), self._stage_ptr, self._stage_bytes, s)
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
        if self._registered.alive:
            torch.cuda.synchronize(self.device)
            self._registered()
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
        self.obs_dim, self.A, self.limit = host_env_spec(vec)
        self.cfg = cfg = dataclasses.replace(cfg, n_envs=len(vec)).validate(device_env=False)
        self.vec = vec
        self.K = int(learner_steps)
        self.host_overlap = bool(host_overlap)
        self.eval_env = eval_env
        self.device = dev = torch.device(device)
        self.hip = ops.hip()
        torch.manual_seed(cfg.seed)
        model = DuelingDQN.from_shapes((self.obs_dim,), self.A)
        self.replay = HBMReplay(cfg.replay_capacity, cfg.n_envs, cfg.n_step, cfg.alpha, dev,
                                frame_bytes=4 * self.obs_dim, seed=cfg.seed + 17)
        self.learner = MLPDQNLearner(model, self.replay, cfg)
        self.actor_model = DuelingDQN.from_shapes((self.obs_dim,), self.A).to(dev)
        self.actor_flat = self.actor_model.flatten_parameters()
        self.shard = VectorHostShard(self.replay, vec, cfg.n_step, cfg.gamma, cfg.eps_base, cfg.eps_alpha,
                                     seed=cfg.seed * 0x2545F491 + 0xAC7, mode=cfg.nstep_mode)
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
        self.learner.copy_params_to(self.actor_flat)
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
        m = DuelingDQN.from_shapes((self.obs_dim,), self.A)
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
