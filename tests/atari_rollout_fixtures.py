"""Models, seeds and the host fp64 rollout shared by the Atari rollout tests (host self-checks
and GPU tests).

The free-running GPU comparisons (one-launch rollout against the stepwise evaluator) are only
meaningful while both fp32 networks pick the same greedy action, so the fixture pins two
(actions, model seed) cases whose fp64 top-2 Q gap stays above ``GAP`` x max|Q| at every step of
the host rollout: 2.5x the 4e-4 x max|Q| two kernels may disagree by when each is within the
project's Q bound (rtol 1e-4, atol 1e-4 x max|Q|, tests/test_gpu_f32_net.py).  ``gap_ok`` is
asserted by the host test and re-asserted (never skipped) by every GPU test that relies on it.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from apex_amd.models.dqn import DuelingDQN

from . import actor_oracle as ao

CASES = {"a18": (18, 2), "a6": (6, 0)}   # name -> (actions, model seed)
ENV_SEED, E, STEPS = 5, 8, 24
EPISODE_LIFE, MAX_EPISODE_STEPS = 1, 7   # three time-limit dones (+ reset draws) per env in 24 steps
GAP = 1e-3
Q_RTOL = Q_ATOL = 1e-4                   # the project's Q bound (atol x max|Q|)
ACT_XOR = 0xE7A1                         # the evaluator's action-draw seed = seed ^ ACT_XOR


def make_model(A: int, ms: int) -> DuelingDQN:
    """Built on the CPU (move it afterwards): default init, every bias U(-0.1, 0.1)."""
    torch.manual_seed(ms)
    m = DuelingDQN.from_shapes((4, 84, 84), A)
    with torch.no_grad():
        for mod in list(m.features) + list(m.advantage) + list(m.value):
            if getattr(mod, "bias", None) is not None:
                mod.bias.uniform_(-0.1, 0.1)
    return m


def constant_argmax_model(A: int, favour: int, ms: int = 0) -> DuelingDQN:
    """Q argmax = ``favour`` for every observation (tests/test_gpu_evaluator.py)."""
    m = make_model(A, ms)
    with torch.no_grad():
        m.advantage[2].bias.zero_()
        m.advantage[2].bias[favour] = 1e4
    return m


class HostEvaluator:
    """The stepwise evaluator on the host: VecEnvOracle envs, the 8 E-slot frame ring, the
    FrameStack ids, select_actions_ref.  ``q_fn(obs u8 [E,4,84,84]) -> Q [E, A]`` (numpy)."""

    def __init__(self, A, E, seed, episode_life=EPISODE_LIFE, max_episode_steps=MAX_EPISODE_STEPS, eps=0.0,
                 counter=0):
        self.A, self.E, self.seed, self.F = A, E, int(seed), 8 * E
        self.env = ao.VecEnvOracle(E, A, self.F, action_repeat=4, clip_rewards=0, episode_life=episode_life,
                                   max_episode_steps=max_episode_steps)
        self.counter = int(counter)
        self.state = np.stack([self.env.reset(e, self.seed, self.counter * 16 + 1) for e in range(E)])
        self.frames = np.zeros((self.F, 84, 84), np.uint8)
        self.hist = np.zeros((E, 4), np.int64)
        self.ep_log = np.zeros((E, 4), np.float32)
        self.eps = np.full(E, eps, np.float32)
        for e in range(E):
            slot = self.env.frame_slot(self.counter, e, reset=True)
            self.frames[slot] = self.env.render(self.state[e])
            self.hist[e] = slot
        self.reward = np.zeros(E, np.float32)
        self.done = np.zeros(E, np.float32)
        self.actions = np.zeros(E, np.int32)

    def obs(self) -> np.ndarray:
        return self.frames[self.hist]  # [E, 4, 84, 84]

    def step(self, q_fn=None, actions=None):
        q = None
        if actions is None:
            q = np.asarray(q_fn(self.obs()))
            actions = ao.select_actions_ref(q.astype(np.float32), self.eps, self.seed ^ ACT_XOR, self.counter)
        self.actions = np.asarray(actions, np.int32)
        for e in range(self.E):
            out = self.env.step(self.state[e], int(actions[e]), e, self.seed, self.counter, self.ep_log[e])
            slot = self.env.frame_slot(self.counter, e)
            self.state[e], self.ep_log[e] = out.state, out.ep_log
            self.reward[e], self.done[e] = out.reward, out.done
            self.frames[slot] = out.frame
            self.hist[e] = slot if out.done else np.append(self.hist[e, 1:], slot)
        self.counter += 1
        return q


def q64_fn(model64: DuelingDQN):
    def f(obs):
        with torch.no_grad():
            return model64(torch.from_numpy(np.ascontiguousarray(obs)).double()).numpy()
    return f


@functools.lru_cache(maxsize=None)
def host_rollout(case: str, n_envs: int = E, steps: int = STEPS, env_seed: int = ENV_SEED):
    """The fp64 greedy rollout of a fixture case: per step Q [steps, E, A] (fp64), actions,
    rewards, dones, and the relative top-2 gap of every (step, env).  Cached; do not modify."""
    A, ms = CASES[case]
    m64 = make_model(A, ms).double()
    ev = HostEvaluator(A, n_envs, env_seed)
    f = q64_fn(m64)
    qs, acts, rews, dones = [], [], [], []
    for _ in range(steps):
        qs.append(ev.step(f))
        acts.append(ev.actions.copy())
        rews.append(ev.reward.copy())
        dones.append(ev.done.copy())
    q = np.stack(qs)
    top = np.sort(q, axis=2)
    # max|Q| over the step's batch of envs: the scale of the Q bound's atol for one stepwise forward
    gap = (top[:, :, -1] - top[:, :, -2]) / np.abs(q).max(axis=(1, 2))[:, None]
    out = {"q": q, "actions": np.stack(acts), "rewards": np.stack(rews), "dones": np.stack(dones), "gap": gap,
           "state": ev.state.copy(), "ep_log": ev.ep_log.copy()}
    for v in out.values():
        v.setflags(write=False)
    return out


def gap_ok(case: str, n_envs: int = E, steps: int = STEPS) -> tuple[bool, float]:
    """(every step's fp64 top-2 gap >= GAP x max|Q|, the smallest gap) for the envs and steps used."""
    g = float(host_rollout(case, n_envs, steps)["gap"].min())
    return g >= GAP, g
