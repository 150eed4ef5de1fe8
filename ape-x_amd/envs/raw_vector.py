"""Raw vector front end for host Atari emulators: :class:`AtariPreprocess` without the pixels.

:class:`RawAtariVector` steps N raw emulators through the same start / repeat / life-ledger /
FIRE-start stages as :class:`apex_amd.envs.preprocess.AtariPreprocess` (the very same stage
helpers), but does no max-pool, grey conversion, resize or stacking.  For every env it hands
back the two unpooled emulator frames whose element-wise max is the observation; the GPU
engine (:mod:`apex_amd.engine.host_env`) copies the pairs to the device, where one kernel does
the pixel work and writes the 84x84 plane into the frame ring.

Differences from ``AtariPreprocess``:

* ``reset(out)`` / ``step(actions, out)`` fill a caller-supplied ``[N, 2, H, W, 3]`` uint8 array
  (the engine passes pinned memory).  With the reference pool the pair is the pool's two
  persistent slots; a single-frame observation (the no-op start's last frame) is written twice.
* It auto-resets: when env ``i`` reports an agent-level done the next episode is started at
  once, exactly as ``reset_one(i)`` would, and the pair written for that step is the start
  observation's -- the convention of the GPU env, whose done step renders the reset frame.
* ``step`` returns ``(reward [N] float64, done [N] bool)``; the reward is the raw, unclipped
  sum over the repeat window (clipping is the consumer's business).
* ``max_episode_steps > 0`` caps an agent-level episode (the reference evaluator's
  ``max_episode_length``): the agent step at which an env's episode reaches that many agent steps
  reports done and the env is started again through the same path as any other done -- with
  ``episode_life`` a game that is not over takes the soft start, as the reference's ``env.reset()``
  through ``EpisodicLifeEnv`` does.  The default 0 is no cap.

The vector-env protocol the engine relies on.  :class:`apex_amd.envs.proc_vector.ProcRawAtariVector`
provides the same five members over worker processes (one ``RawAtariVector`` per worker), plus a
shared ``staging`` block and a banked ``step_async`` / ``wait_bank`` form the engine uses when it
finds them:

``__len__()``              number of envs
``raw_shape``              ``(H, W, 3)`` of one emulator frame
``n_actions``              size of the discrete action set
``reset(out)``             start every env, fill ``out``
``step(actions, out)``     one agent step of every env, fill ``out``, return ``(reward, done)``
"""
from __future__ import annotations

import numpy as np

from .preprocess import (LifeLedger, PreprocessSpec, RepeatPool, fire_start, has_fire, life_start, lives_of, meaning,
                         noop_start)


class PairPool(RepeatPool):
    """:class:`RepeatPool` that returns the pair ``[2, H, W, 3]`` instead of its max: the two
    persistent slots (reference pool) or the last two frames of this window (the only frame
    twice when the window ends after one step)."""

    def run(self, step_fn, action):
        total, prev, last, done, info = 0.0, None, None, False, {}
        for i in range(self.repeat):
            frame, r, done, info = step_fn(action)
            if self.reference:
                if self._slots is None:
                    f = np.asarray(frame)
                    self._slots = np.zeros((2,) + f.shape, dtype=f.dtype)
                if i == self.repeat - 2:
                    self._slots[0] = frame
                if i == self.repeat - 1:
                    self._slots[1] = frame
            prev, last = last, frame
            total += r
            if done:
                break
        if self.reference:
            return self._slots.copy(), total, done, info  # (a later window must not change this one's pair)
        return np.stack([last if prev is None else prev, last]), total, done, info


class RawAtariVector:
    def __init__(self, raw_envs, spec: PreprocessSpec = PreprocessSpec(), max_episode_steps: int = 0):
        self.envs = list(raw_envs)
        self.spec = spec
        if int(max_episode_steps) < 0:
            raise ValueError("max_episode_steps must be >= 0 (0 = no cap)")
        self.max_episode_steps = int(max_episode_steps)
        self.episode_steps = [0] * len(self.envs)   # agent steps of each env's episode in progress
        self.fixed_noops: list[int | None] = [None] * len(self.envs)
        e0 = self.envs[0]
        if meaning(e0, 0) != "NOOP":
            raise ValueError("action 0 must be NOOP")
        fire = has_fire(e0) if spec.fire_reset is None else spec.fire_reset
        if fire and (meaning(e0, 1) != "FIRE" or len(e0.unwrapped.get_action_meanings()) < 3):
            raise ValueError("the FIRE start needs FIRE at action 1 and at least 3 actions")
        self.fire = fire
        self.pools = [PairPool(spec.skip, spec.reference_pool) for _ in self.envs]
        self.ledgers = [LifeLedger() for _ in self.envs]
        shape = tuple(e0.observation_space.shape)
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError(f"raw emulator frames must be [H, W, 3], got {shape}")
        self.raw_shape = shape
        self.action_space = e0.action_space
        self.n_actions = int(e0.action_space.n)

    def __len__(self) -> int:
        return len(self.envs)

    # -- the stages of AtariPreprocess, on pairs
    def _repeat(self, i, a):
        return self.pools[i].run(self.envs[i].step, a)

    def _agent_step(self, i, a):
        pair, r, done, info = self._repeat(i, a)
        if self.spec.episode_life:
            done = self.ledgers[i].observe(done, lives_of(self.envs[i]))
        return pair, r, done, info

    def _hard_start(self, i):
        return noop_start(self.envs[i], self.spec.noop_max, self.fixed_noops[i])

    def _start(self, i):
        if self.spec.episode_life:
            return life_start(self.ledgers[i], lambda: self._hard_start(i), lambda a: self._repeat(i, a),
                              lambda: lives_of(self.envs[i]))
        return self._hard_start(i)

    def _start_into(self, i, out) -> None:
        obs = fire_start(lambda: self._start(i), lambda a: self._agent_step(i, a)) if self.fire else self._start(i)
        out[i] = np.asarray(obs)  # a pair, or one frame [H, W, 3] broadcast into both halves

    def _check(self, out) -> None:
        want = (len(self.envs), 2) + self.raw_shape
        if tuple(out.shape) != want or out.dtype != np.uint8:
            raise ValueError(f"out must be uint8 {want}, got {out.dtype} {tuple(out.shape)}")

    def reset(self, out: np.ndarray) -> None:
        self._check(out)
        for i in range(len(self.envs)):
            self.episode_steps[i] = 0
            self._start_into(i, out)

    def step(self, actions, out: np.ndarray):
        self._check(out)
        n = len(self.envs)
        rew = np.zeros(n, dtype=np.float64)
        done = np.zeros(n, dtype=bool)
        for i in range(n):
            pair, r, d, _ = self._agent_step(i, int(actions[i]))
            self.episode_steps[i] += 1
            d = d or 0 < self.max_episode_steps <= self.episode_steps[i]
            rew[i], done[i] = r, d
            if d:
                self.episode_steps[i] = 0
                self._start_into(i, out)
            else:
                out[i] = pair
        return rew, done

    def seed(self, seed: int) -> None:
        for i, e in enumerate(self.envs):
            e.seed(seed + i)
