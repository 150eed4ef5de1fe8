"""Greedy evaluator for the GPU engine (reference: origin_repo/eval.py:49-96).

The reference evaluator is one extra process: the latest published parameters, an
epsilon = 0 policy, ``clip_rewards`` forced off (episode returns in game points), the
same wrappers otherwise (episodic life on by default, ``max_episode_length`` 50000),
and ``evaluator/episode_reward`` / ``evaluator/episode_length`` logged per episode.

Here it is ``n_envs`` extra GPU envs with their own small frame ring (the training
replay's ring is never touched), their own copy of the network in the engine's
precision, and the same kernels as the actor shard: forward with the heads kernel's
action epilogue fed an all-zero epsilon (greedy), ``vec_env_step`` with reward
clipping off, and ``frame_hist_step`` advancing the observation stacks.  ``load`` copies
the latest published weights (the engine's actor weights, as the reference evaluator
takes the learner's PUB stream); ``run(k)`` advances every env ``k`` steps on the
caller's stream (a side stream in ``train.py``); ``poll()`` returns the episodes
finished since the last poll (a host read of the [E, 4] episode log).

``rollout(k)`` is ``run(k)`` in one launch (``atari_rollout``, fp32 HIP forward only): one
workgroup per env runs forward -> action -> env step -> render ``k`` times and leaves every
buffer as ``run(k)`` does, so the two may alternate.  It also fills ``ep_ring`` (the last
``RING`` episodes per env; ``poll_ring()``), since a long chunk ends several episodes per env.
:class:`AtariEvaluator` runs rollouts of a weight snapshot on a side stream beside training.
"""
from __future__ import annotations

import torch

from .. import ops
from ..models.dqn import DuelingDQN
from .actor_shard import ENV_STATE_STRIDE
from .evaluation import SideStreamEvaluation
from .graphs import capture_graph
from .hbm_replay import FRAME_BYTES


class GPUEvaluator:
    RING = 16           # episodes per env kept by ``ep_ring``
    MAX_ROLLOUT = 10000  # steps per ``atari_rollout`` launch

    def __init__(self, src_model: DuelingDQN, n_envs: int = 8, n_actions: int = 18, forward: str = "hip",
                 dtype: str = "fp32", device="cuda", seed: int = 0, episode_life: bool = True,
                 max_episode_steps: int = 50000, action_repeat: int = 4, epsilon: float = 0.0):
        self.hip = ops.hip()
        self.device = torch.device(device)
        self.E, self.A = int(n_envs), int(n_actions)
        self.seed = int(seed)
        E, dev = self.E, self.device
        self.model = DuelingDQN.from_shapes((4, 84, 84), self.A).to(dev)
        self.model.load_state_dict(src_model.state_dict())
        self.flat = self.model.flatten_parameters()
        for p in self.model.parameters():
            p.requires_grad_(False)
        self.forward_mode, self.dtype = forward, dtype
        if forward == "hip":
            from ..models.fused import make_hip_net, make_workspace

            self.net = make_hip_net(self.model, dtype)
            self.ws = make_workspace(E, self.A, dev, dtype)
        # frames live (2 x 4) steps in the ring: the stack needs the last 4
        self.F = E * 8
        self.frames = torch.zeros(self.F, FRAME_BYTES, dtype=torch.uint8, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.env_state = torch.zeros(E, ENV_STATE_STRIDE, **f32)
        self.new_frame = torch.zeros(E, **i32)
        self.hist = torch.zeros(E, 4, **i32)
        self.ep_log = torch.zeros(E, 4, **f32)
        self.reward = torch.zeros(E, **f32)
        self.done = torch.zeros(E, **f32)
        self.actions = torch.zeros(E, **i32)
        # greedy (reference: model.act(state, 0.)); epsilon 1 = the uniform-random baseline
        self.eps = torch.full((E,), float(epsilon), **f32)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.obs = torch.zeros(E, 4, 84, 84, dtype=torch.uint8, device=dev)
        self.params = self.hip.VecEnvParams(E, self.A, FRAME_BYTES, self.F, action_repeat, 0, int(episode_life),
                                            int(max_episode_steps))
        self.hip.vec_env_reset(self.env_state.data_ptr(), self.seed, self.frames.data_ptr(), self.params,
                               self.counter.data_ptr(), self.new_frame.data_ptr(), self.hist.data_ptr(),
                               self.ep_log.data_ptr(), self._stream())
        self._seen = torch.zeros(E)
        self.episodes = 0
        self.steps = 0
        self.max_episode_steps = int(max_episode_steps)
        self._graph, self._graph_steps = None, 0
        # (return, length) of the last RING episodes per env: written by ``rollout`` only
        self.ep_ring = torch.zeros(E, self.RING, 2, **f32)
        self._ring_seen = torch.zeros(E)

    @staticmethod
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream

    def load(self, flat: torch.Tensor, net=None) -> None:
        """Take the latest published weights (flat fp32 buffer of the same architecture;
        ``net``: the source's HIP net, whose packed copies are copied instead of re-derived)."""
        self.hip.copy_f32(self.flat.data_ptr(), flat.data_ptr(), self.flat.numel(), self._stream())
        if self.forward_mode == "hip":
            if net is not None and type(net) is type(self.net):
                self.net.copy_packed_from(net)
            else:
                self.net.repack()

    def step(self) -> None:
        """One greedy step of every evaluator env."""
        h, s = self.hip, self._stream()
        if self.forward_mode == "hip":
            self.net(self.frames, self.ws, self.hist,
                     act=(self.eps.data_ptr(), self.seed ^ 0xE7A1, self.counter.data_ptr(), self.actions.data_ptr()))
        else:
            from .learner import forward_q

            self.hip.gather_frames(self.frames.data_ptr(), FRAME_BYTES, self.hist.data_ptr(), self.E, 4,
                                   self.obs.data_ptr(), s)
            with torch.no_grad():
                q = forward_q(self.model, self.obs, self.dtype == "bf16")
            self.hip.select_actions(q.contiguous().data_ptr(), self.E, self.A, self.eps.data_ptr(), self.seed ^ 0xE7A1,
                                    self.counter.data_ptr(), self.actions.data_ptr(), s)
        h.vec_env_step(self.env_state.data_ptr(), self.actions.data_ptr(), self.seed, self.counter.data_ptr(),
                       self.frames.data_ptr(), self.params, self.reward.data_ptr(), self.done.data_ptr(),
                       self.new_frame.data_ptr(), self.ep_log.data_ptr(), s)
        h.frame_hist_step(self.hist.data_ptr(), self.new_frame.data_ptr(), self.done.data_ptr(), self.E,
                          self.counter.data_ptr(), s)
        self.steps += 1

    def run(self, n_steps: int) -> None:
        """``n_steps`` greedy steps of every env: whole replays of the captured chunk graph
        (:meth:`capture`) while they fit, eager steps for the rest."""
        if self._graph is not None:
            for _ in range(n_steps // self._graph_steps):
                self._graph.replay()
                self.steps += self._graph_steps
            n_steps %= self._graph_steps
        for _ in range(n_steps):
            self.step()

    def _rollout_args(self) -> dict:
        m, f, net = self.model, self.model.features, self.net
        t = {"w1": f[0].weight, "b1": f[0].bias, "w2p": net.w2p, "b2": f[2].bias, "w3p": net.w3p, "b3": f[4].bias,
             "wfc1p": net.wfc1p, "ba1": m.advantage[0].bias, "bv1": m.value[0].bias, "wa2": m.advantage[2].weight,
             "ba2": m.advantage[2].bias, "wv2": m.value[2].weight, "bv2": m.value[2].bias, "eps": self.eps,
             "counter": self.counter, "env_state": self.env_state, "hist": self.hist, "frames": self.frames,
             "new_frame": self.new_frame, "ep_log": self.ep_log, "reward": self.reward, "done": self.done,
             "actions": self.actions, "ep_ring": self.ep_ring}
        d = {k: v.data_ptr() for k, v in t.items()}
        d.update(env_seed=self.seed, act_seed=self.seed ^ 0xE7A1, ring_R=self.RING)
        return d

    def rollout(self, n_steps: int, trace: dict | None = None) -> None:
        """``run(n_steps)`` as one ``atari_rollout`` launch per at most 10,000 steps on the current
        stream, each followed by the stream-ordered counter advance.  ``trace``: ``q`` f32
        [E, T, A], ``act`` i32 [E, T], ``rew`` / ``done`` f32 [E, T] for the first T steps."""
        if self.forward_mode != "hip" or self.dtype != "fp32":
            raise ValueError(f"rollout needs the fp32 HIP forward (forward='{self.forward_mode}', "
                             f"dtype='{self.dtype}')")
        n_steps = int(n_steps)
        if n_steps < 1:
            raise ValueError("rollout: n_steps >= 1")
        args = self._rollout_args()
        if trace is not None:
            q, act = trace["q"], trace["act"]
            assert q.dtype == torch.float32 and act.dtype == torch.int32 and q.is_contiguous()
            assert q.shape[0] >= self.E and q.shape[2] == self.A and tuple(act.shape) == tuple(q.shape[:2])
            args.update(trace_q=q.data_ptr(), trace_act=act.data_ptr(), trace_rew=trace["rew"].data_ptr(),
                        trace_done=trace["done"].data_ptr(), trace_T=int(q.shape[1]))
        left = n_steps
        while left > 0:
            k = min(left, self.MAX_ROLLOUT)
            args["n_steps"] = k
            self.hip.atari_rollout(self.hip.make_atari_rollout(self.params, args), self._stream())
            self.counter.add_(k)
            left -= k
            for key in ("trace_q", "trace_act", "trace_rew", "trace_done", "trace_T"):
                args.pop(key, None)  # the trace covers the first launch's first steps
        self.steps += n_steps

    def capture(self, steps: int = 100) -> None:
        """Capture ``steps`` greedy steps as one hipGraph on the current stream (the
        evaluator's ~8 launches per step are host-bound when eager: a budget that finishes
        capped episodes is thousands of steps per log window)."""
        self.step()  # (a real step: every kernel's first launch happens outside the capture)
        torch.cuda.synchronize(self.device)
        g = capture_graph(lambda: [self.step() for _ in range(steps)])
        self.steps -= steps  # the captured steps did not run
        self._graph, self._graph_steps = g, int(steps)

    def running(self) -> tuple[torch.Tensor, torch.Tensor]:
        """(return so far, steps so far) of every env's episode in progress (one host read):
        the explicit marker for episodes still running at a log line."""
        st = self.env_state[:, 25:27].cpu()  # S_EPRET, S_EPLEN (actor_kernels.hip)
        return st[:, 0], st[:, 1]

    def poll(self) -> list[tuple[float, float]]:
        """(episode_reward, episode_length) of the episodes finished since the last poll
        (the last one per env if an env finished several: the log keeps one per env)."""
        log = self.ep_log.cpu()
        out = []
        for e in range(self.E):
            if log[e, 2] > self._seen[e]:
                out.append((float(log[e, 0]), float(log[e, 1])))
        self.episodes += int((log[:, 2] - self._seen).clamp_min(0).sum())
        self._seen = log[:, 2].clone()
        return out

    @staticmethod
    def ring_episodes(ring: torch.Tensor, counts: torch.Tensor, seen: torch.Tensor) -> list[tuple[float, float]]:
        """The episodes ``seen[e] .. counts[e] - 1`` of every env still in its ring (the newest
        ``R``), oldest first: episode i of env e is ring slot ``i % R``."""
        R = ring.shape[1]
        out = []
        for e in range(ring.shape[0]):
            c, s0 = int(counts[e]), int(seen[e])
            for i in range(max(s0, c - R), c):
                out.append((float(ring[e, i % R, 0]), float(ring[e, i % R, 1])))
        return out

    def poll_ring(self) -> list[tuple[float, float]]:
        """Every episode finished since the last ``poll_ring`` (up to ``RING`` per env, oldest
        first) from ``ep_ring``: episodes that ``rollout`` ended (stepwise steps do not fill it)."""
        ring, counts = self.ep_ring.cpu(), self.ep_log[:, 2].cpu()
        out = self.ring_episodes(ring, counts, self._ring_seen)
        self._ring_seen = counts.clone()
        self.episodes = int(counts.sum())
        return out

    # ---- the device side of AtariEvaluator
    def snapshot(self, src_flat: torch.Tensor, src_net) -> None:
        """Device copies of the source weights on the current stream: the flat parameters and
        the forward arena."""
        self.hip.copy_f32(self.flat.data_ptr(), src_flat.data_ptr(), self.flat.numel(), self._stream())
        self.net.copy_packed_from(src_net)

    def host_results(self) -> dict:
        E = self.E
        return {"ring": torch.zeros(E, self.RING, 2).pin_memory(), "counts": torch.zeros(E).pin_memory(),
                "running": torch.zeros(E, 2).pin_memory()}

    def copy_results(self, host: dict) -> None:
        host["ring"].copy_(self.ep_ring, non_blocking=True)
        host["counts"].copy_(self.ep_log[:, 2], non_blocking=True)
        host["running"].copy_(self.env_state[:, 25:27], non_blocking=True)  # S_EPRET, S_EPLEN


class AtariEvaluator(SideStreamEvaluation):
    """Greedy evaluation beside training (:class:`SideStreamEvaluation`).  ``launch()`` snapshots
    the source weights into the evaluator's own copies and plays ``n_steps`` greedy steps with
    ``GPUEvaluator.rollout`` on the side stream; a result holds the episodes finished since the
    previous one and the running (return, length) of every env."""

    def __init__(self, evaluator, stream=None, event=None, stream_ctx=None):
        super().__init__(evaluator.device, stream, event, stream_ctx)
        self.ev = evaluator
        self.host = evaluator.host_results()
        self._seen = torch.zeros_like(self.host["counts"])

    def launch(self, src_flat, src_net, n_steps: int, tag=None) -> bool:
        """Start one evaluation chunk of the source weights as they are at this point of the
        current stream.  ``False`` (and nothing done) while the previous one has not landed."""
        def play():
            self.ev.rollout(n_steps)
            self.ev.copy_results(self.host)

        return self._launch(tag, lambda: self.ev.snapshot(src_flat, src_net), play)

    def _result(self) -> dict:
        h = self.host
        counts = h["counts"].clone()
        eps = GPUEvaluator.ring_episodes(h["ring"], counts, self._seen)
        self._seen = counts
        return {"episodes": eps, "total_episodes": int(counts.sum()),
                "running_return": h["running"][:, 0].tolist(), "running_length": h["running"][:, 1].tolist()}
