"""The GPU AQL engine over HOST environments: gym-API envs stepped on the CPU under the HBM
replay, the acting forward and the fused learner of :mod:`apex_amd.engine.aql`.

:class:`~apex_amd.engine.aql.AQLEngine` hard-wires three device envs into its kernels; the
reference takes any ``gym.make(env_id)`` (AQL_dis.py:145).  :class:`AQLHostEngine` is the same
engine with a different acting tail: a :class:`~apex_amd.envs.host_vector.HostVectorEnv` (or any
object of its protocol) steps the envs, one H2D copy moves its staging block, and one kernel
(``aql_host_tail``, ops/csrc/aql_host_kernels.hip) writes the replay rows, the episode log and
the tree exactly where ``aql_act_tail`` would have.  Models, replay, learner, candidate proposal,
candidate critic, selection (same seeds, same counter), checkpoints and cadences are shared
(:class:`~apex_amd.engine.aql.AQLEngineCore`).

One acting step: ``aql_propose`` -> ``aql_act_q`` -> ``aql_select`` -> the actions D2H into a
pinned buffer + an event | the host waits for the event and steps the envs | one
``memcpy_h2d_async`` of the staging block (registered with HIP, read in place) ->
``aql_host_tail``: 4 kernel launches, 2 copies, 1 host wait.

Iteration order.  ``host_overlap=False``: the acting step, then the K learner steps -- the
GPU-env engine's order.  ``host_overlap=True`` (default): the acting forward and the action
copy are enqueued, then the K learner steps (the captured learner graph after
:meth:`AQLHostEngine.capture`), and only then does the host wait for the actions and step the
envs, while the GPU trains; the staging copy and the tail follow.  Everything is on ONE stream.
**The learner of iteration i therefore samples the transitions through iteration i - 1**: the
step acted in iteration i reaches the ring after that iteration's SGD steps (one acting step of
lag, as ``AQLEngineConfig.overlap`` has on the device envs).

One staging block is enough: the host writes it again only after it has waited for the event
recorded after the NEXT acting forward, which the same stream runs after the copy that read it.

Greedy evaluation: :meth:`AQLHostEngine.evaluate` is the blocking host one
(``train_aql.greedy_eval`` on a separate env of the same id);
:class:`~apex_amd.engine.aql_host_eval.AQLHostEvaluator` plays evaluator envs of its own in worker
processes beside training (``train_aql --eval-envs``: a side stream, two weight sets, a pump that
never waits).  ``rollout_evaluate`` and :class:`~apex_amd.engine.aql.AQLEvaluator` play device
envs and are refused.  Out of scope: worker processes for the TRAINING envs, the central
(``--gpus N``) topology over host envs, double-banked env groups.
"""
from __future__ import annotations

import weakref

import numpy as np
import torch

from ..envs import spaces
from .aql import AQLEngineConfig, AQLEngineCore
from .host_env import _unregister


class _Spaces:
    """The two spaces the AQL model is built from, out of a vector env's attributes."""

    def __init__(self, vec):
        big = np.full(int(vec.obs_dim), np.finfo(np.float32).max, dtype=np.float32)
        self.observation_space = spaces.Box(-big, big, dtype=np.float32)
        if vec.continuous:
            self.action_space = spaces.Box(np.asarray(vec.low, dtype=np.float32).reshape(-1),
                                           np.asarray(vec.high, dtype=np.float32).reshape(-1), dtype=np.float32)
        else:
            self.action_space = spaces.Discrete(int(vec.n_actions))


class AQLHostEngine(AQLEngineCore):
    """Actors on host envs + replay + learner of AQL_dis on one GPU (see module docstring).
    ``cfg.n_envs`` is ignored: the vector env says how many envs there are."""

    def __init__(self, cfg: AQLEngineConfig, vec, device: str | torch.device = "cuda", host_overlap: bool = True):
        if cfg.overlap:
            raise ValueError("AQLEngineConfig.overlap is the device envs' acting stream; host envs overlap with "
                             "host_overlap")
        E = len(vec)
        if E > 1024:
            raise ValueError("AQLHostEngine: at most 1024 envs (aql_host_tail's one tree workgroup)")
        self.vec = vec
        self.host_overlap = bool(host_overlap)
        self.host_env = _Spaces(vec)
        self._init_core(cfg, device, E)
        h, dev, r = self.hip, self.device, self.replay
        if int(vec.obs_dim) != self.obs or int(vec.action_dim) != self.adim:
            raise ValueError("the vector env's obs_dim / action_dim differ from the model's")
        self.learner.set_publish(self.actor_flat, self.actor_eps)
        # the staging block, registered with HIP and read in place, and its device copy
        st = vec.staging
        n = E * (2 * self.obs + 3)
        if not isinstance(st, np.ndarray) or st.dtype != np.float32 or st.shape != (n,) or not st.flags.c_contiguous:
            raise ValueError(f"staging must be a contiguous float32 array of {n} elements")
        self._stage_ptr, self._stage_bytes = int(st.ctypes.data), int(st.nbytes)
        h.host_register(self._stage_ptr, self._stage_bytes)
        self._registered = weakref.finalize(self, _unregister, h, self._stage_ptr, st)
        self.stage_dev = torch.zeros(n, dtype=torch.float32, device=dev)
        self.act_host = torch.zeros(E, self.adim, dtype=torch.float32).pin_memory()
        self._act_np = self.act_host.numpy()
        self.event = torch.cuda.Event()
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self._iter_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._tail = h.make_aql_host_tail(self.ins, r.tree, dict(
            E=E, obs=self.obs, adim=self.adim, T=self.T, stage=self.stage_dev.data_ptr(),
            obs_buf=self.obs_buf.data_ptr(), amu=self.amu.data_ptr(), act_idx=self.act_idx.data_ptr(),
            ep_len=self.ep_len.data_ptr(), ep_ret=self.ep_ret.data_ptr(), ep_count=self.ep_count.data_ptr(),
            ep_log=self.ep_log.data_ptr(), log_cap=self.log_cap, alpha=float(r.alpha), max_prio=r.max_prio.data_ptr(),
            filled=r.filled.data_ptr(), counter=self.actor_ctr.data_ptr(), ticket=self._ticket.data_ptr(),
            beta_out=self.learner.beta.data_ptr(), iter=self._iter_dev.data_ptr(), beta0=float(cfg.beta_start),
            beta_omb=1.0 - cfg.beta_start, beta_max_step=float(cfg.max_step), beta_workers=float(cfg.n_workers)))
        self._init_acting()
        self.eval_limit = int(getattr(vec, "max_episode_steps", None) or 10_000)
        self.env_steps = 0    # host env steps taken (all envs)
        vec.reset()
        o = E * self.obs
        self.obs_buf.copy_(torch.from_numpy(st[o:2 * o].reshape(E, self.obs)))   # reset_obs (a blocking copy)

    # ------------------------------------------------------------------ counters
    def _set_iterations(self, v: int) -> None:
        """As :class:`AQLEngineCore`'s; overlapped, the tail of iteration i writes the PER beta
        of iteration i + 1 (that learner runs before its own tail), so the device counter leads
        by one and the next learner's beta is written here."""
        AQLEngineCore.iterations.fset(self, v)
        if self.host_overlap and getattr(self, "_tail", None) is not None:
            self._iter_dev.fill_(self._iterations + 1)
            self.learner.beta.fill_(self._beta())

    iterations = property(AQLEngineCore.iterations.fget, _set_iterations)

    # ------------------------------------------------------------------ phases
    def _enqueued(self) -> None:
        """Called after every enqueue of an iteration (a test synchronizes here)."""

    def act_begin(self) -> None:
        """The acting forward (AQLEngine._act: same seeds and counter), the actions on their way
        to the host, the event the host waits for."""
        self._act(self.hip, self._s(), self.E)
        self._enqueued()
        self.act_host.copy_(self.env_act, non_blocking=True)
        self.event.record()
        self._enqueued()

    def act_finish(self) -> None:
        """Wait for the actions, step the host envs, ship the staging block, run the tail."""
        h, s = self.hip, self._s()
        self.event.synchronize()
        self.vec.step(self._act_np)
        self.env_steps += self.E
        h.memcpy_h2d_async(self.stage_dev.data_ptr(), self._stage_ptr, self._stage_bytes, s)
        self._enqueued()
        h.aql_host_tail(self._tail, s)
        self._enqueued()

    def actor_step(self) -> None:
        self.act_begin()
        self.act_finish()

    def _learn(self) -> bool:
        if self._g_learn is not None:
            self._g_learn.replay()
            pub = self._pub_in_graph
        else:
            pub = self.learn_steps(publish=True)
        self._enqueued()
        return pub

    def fill(self, threshold: int | None = None) -> None:
        """Act until the replay holds more than ``threshold`` transitions (AQL_dis.py:120)."""
        thr = threshold if threshold is not None else (self.cfg.threshold or self.cfg.batch_size + 1)
        for _ in range(max(1, -(-int(thr) // self.E))):
            self.actor_step()
        self.iterations = self._iterations  # (resyncs the tail's device iteration counter)
        self.publish()

    def capture(self) -> None:
        """The K learner steps as one hipGraph (the acting step waits for the host: it stays
        eager)."""
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):  # warm the launch paths outside capture
            torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._pub_in_graph = self.learn_steps(publish=True)
        self._g_learn = g
        torch.cuda.synchronize(self.device)

    def iteration(self) -> None:
        """One step of all host envs and K learner steps, in the order ``host_overlap`` selects
        (module docstring); then the publish if the last step did not, and the target cadence."""
        self.act_begin()
        if self.host_overlap:
            pub = self._learn()
            self.act_finish()
        else:
            self.act_finish()
            pub = self._learn()
        if not pub:
            self.publish()
        self._after_learn()

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, episodes: int = 10, seed: int = 12345) -> list[float]:
        """Greedy returns on a separate host env of ``cfg.env_id`` (``train_aql.greedy_eval``: a
        CPU copy of the online net in eval mode, eps 0)."""
        from ..train_aql import greedy_eval

        return greedy_eval(self, int(episodes), seed=int(seed))

    def rollout_evaluate(self, *a, **k):
        raise RuntimeError("rollout_evaluate plays aql_rollout's device envs; a host-env engine evaluates on the "
                           "host: AQLHostEngine.evaluate")

    def close(self) -> None:
        """Finish the queued work, release the staging block, close the vector env.  Idempotent."""
        if self._registered.alive:
            torch.cuda.synchronize(self.device)
            self._registered()
        close = getattr(self.vec, "close", None)
        if close is not None:
            close()
