"""An in-process vector of N gym-API envs with flat fp32 observations, for the host-env AQL
engine (:mod:`apex_amd.engine.aql_host`) and the host-env vector Ape-X engine
(:mod:`apex_amd.engine.vector_host`, which has tighter shape limits of its own).

The envs are whatever :func:`apex_amd.envs.make` returns (the in-package classic-control envs,
or a real ``gym`` with ``APEX_USE_GYM=1``) or the callables handed in.  Env ``i`` is seeded
``seed + i``, the reference worker's seeding (batchrecoder_AQL.py:99).  One step of all envs
lands in ``staging``, one contiguous fp32 block that a single H2D copy moves::

    next_obs [N, obs] | reset_obs [N, obs] | reward [N] | done [N] | ended [N]

``next_obs`` is the step's own observation -- the terminal one when the episode ended --
``done`` the env's flag, and ``ended`` says the env was reset: ``done or episode_length >=
max_episode_length`` (batchrecoder_AQL.py:54-55).  A length-cap reset keeps ``done = 0``: the
reference stores the env's flag.  ``reset_obs`` is what the next action is chosen from: the new
episode's first observation after an end, ``next_obs`` otherwise.

No torch here: a worker-pool form can wrap this module the way ``proc_vector`` wraps
``raw_vector``.
"""
from __future__ import annotations

from typing import Callable, Sequence

import numpy as np

from .spaces import is_box, is_discrete

MAX_OBS = 64         # the acting kernels' widest observation (one lane per component)
MAX_ACTION_DIM = 8   # the candidate critic's widest action vector
MAX_ACTIONS = 64     # the proposal's widest categorical


def staging_views(block: np.ndarray, n: int, obs: int) -> dict:
    """The five views of a staging block of ``n * (2 * obs + 3)`` floats."""
    assert block.dtype == np.float32 and block.ndim == 1 and block.size == n * (2 * obs + 3)
    o = n * obs
    return {"next_obs": block[:o].reshape(n, obs), "reset_obs": block[o:2 * o].reshape(n, obs),
            "reward": block[2 * o:2 * o + n], "done": block[2 * o + n:2 * o + 2 * n],
            "ended": block[2 * o + 2 * n:]}


class HostVectorEnv:
    def __init__(self, env_fns: str | Sequence[Callable], n: int | None = None, seed: int = 0,
                 max_episode_length: int = 50000):
        if isinstance(env_fns, str):
            from .core import make

            env_id = env_fns
            if n is None or int(n) < 1:
                raise ValueError("HostVectorEnv(env_id, n): n >= 1 envs")
            env_fns = [lambda: make(env_id)] * int(n)
        else:
            env_fns = list(env_fns)
            if n is not None and int(n) != len(env_fns):
                raise ValueError(f"n = {n} but {len(env_fns)} env constructors")
        if not env_fns:
            raise ValueError("HostVectorEnv needs at least one env")
        self.envs = [fn() for fn in env_fns]
        self.seed = int(seed)
        self.max_episode_length = int(max_episode_length)
        e0 = self.envs[0]
        shape = tuple(e0.observation_space.shape)
        if len(shape) != 1:
            raise ValueError(f"HostVectorEnv takes flat observations, got shape {shape}")
        self.obs_dim = int(shape[0])
        sp = self.action_space = e0.action_space
        self.observation_space = e0.observation_space
        self.continuous = bool(is_box(sp))
        if self.continuous:
            if len(sp.shape) != 1:
                raise ValueError(f"HostVectorEnv takes flat Box actions, got shape {tuple(sp.shape)}")
            self.action_dim = self.n_actions = int(sp.shape[0])
            self.low = np.asarray(sp.low, dtype=np.float32).reshape(-1)
            self.high = np.asarray(sp.high, dtype=np.float32).reshape(-1)
        elif is_discrete(sp):
            self.action_dim, self.n_actions = 1, int(sp.n)
            self.low = self.high = np.zeros(1, dtype=np.float32)
        else:
            raise ValueError(f"HostVectorEnv takes Box or Discrete actions, got {sp!r}")
        if self.obs_dim > MAX_OBS:
            raise ValueError(f"observation dim {self.obs_dim} exceeds the acting kernels' limit of {MAX_OBS}")
        if self.action_dim > MAX_ACTION_DIM:
            raise ValueError(f"action dim {self.action_dim} exceeds the candidate critic's limit of {MAX_ACTION_DIM}")
        if not self.continuous and self.n_actions > MAX_ACTIONS:
            raise ValueError(f"{self.n_actions} discrete actions exceed the proposal's limit of {MAX_ACTIONS}")
        lim = getattr(e0, "_max_episode_steps", None)
        if lim is None:
            lim = getattr(getattr(e0, "spec", None), "max_episode_steps", None)
        self.max_episode_steps = None if lim is None else int(lim)
        for i, env in enumerate(self.envs):
            env.seed(self.seed + i)
        N = len(self.envs)
        self.staging = np.zeros(N * (2 * self.obs_dim + 3), dtype=np.float32)
        v = staging_views(self.staging, N, self.obs_dim)
        self.next_obs, self.reset_obs = v["next_obs"], v["reset_obs"]
        self.reward, self.done, self.ended = v["reward"], v["done"], v["ended"]
        self.episode_length = np.zeros(N, dtype=np.int64)

    def __len__(self) -> int:
        return len(self.envs)

    def reset(self) -> np.ndarray:
        """Start every env; the first observations fill ``reset_obs`` (returned)."""
        for i, env in enumerate(self.envs):
            self.reset_obs[i] = np.asarray(env.reset(), dtype=np.float32).reshape(-1)
        self.episode_length[:] = 0
        return self.reset_obs

    def _cast(self, a: np.ndarray):
        if self.continuous:
            return np.array(a, dtype=np.float32).reshape(self.action_space.shape)
        return int(a[0])

    def step(self, actions: np.ndarray) -> None:
        """Step env ``i`` with ``actions[i]`` (fp32 ``[N, action_dim]``; a Discrete env takes
        ``int(actions[i, 0])``) and fill the staging block."""
        actions = np.asarray(actions, dtype=np.float32).reshape(len(self.envs), self.action_dim)
        for i, env in enumerate(self.envs):
            o, r, d, _ = env.step(self._cast(actions[i]))
            self.next_obs[i] = np.asarray(o, dtype=np.float32).reshape(-1)
            self.reward[i] = r
            self.done[i] = 1.0 if d else 0.0
            self.episode_length[i] += 1
            if d or self.episode_length[i] >= self.max_episode_length:
                self.ended[i] = 1.0
                self.reset_obs[i] = np.asarray(env.reset(), dtype=np.float32).reshape(-1)
                self.episode_length[i] = 0
            else:
                self.ended[i] = 0.0
                self.reset_obs[i] = self.next_obs[i]

    def close(self) -> None:
        for env in self.envs:
            env.close()
