"""Fixtures of the host-env vector engine tests (``test_vector_host_host``,
``test_gpu_vector_host``): a numpy model of ``vec_host_tail`` (both forms), a vector env of the
``HostVectorEnv`` protocol that replays a recorded tape, and two scripted deterministic envs built
with ``envs.spaces``."""
import numpy as np

from apex_amd.envs import spaces
from apex_amd.envs.core import Env
from apex_amd.envs.host_vector import staging_views


# ------------------------------------------------------------------ vec_host_tail in numpy
def tail_state(E: int, obs: int, F: int, step: int = 0) -> dict:
    """The buffers ``vec_host_tail`` writes, zeroed, + the shard's step counter."""
    return dict(ring=np.zeros((F, obs), np.float32), reward=np.zeros(E, np.float32), done=np.zeros(E, np.float32),
                new_frame=np.zeros(E, np.int32), hist=np.zeros((E, 4), np.int32), ep_log=np.zeros((E, 4), np.float32),
                ep_ret=np.zeros(E, np.float32), ep_len=np.zeros(E, np.float32), step=int(step))


def tail_model(state: dict, stage: dict, reset: bool = False) -> None:
    """``vec_host_tail`` in numpy, env by env, on the buffers of :func:`tail_state` (updated in
    place; ``step`` is read only: ``nstep_emit`` bumps it).  ``stage``: the views of a staging
    block (``reset_obs``, ``reward``, ``done``, ``ended``; ``next_obs`` is not read).  All sums
    are fp32, in step order."""
    F, _ = state["ring"].shape
    E = state["reward"].shape[0]
    step = int(state["step"])
    for e in range(E):
        slot = ((step + (0 if reset else 1)) * E + e) % F      # (python ints: no overflow)
        state["ring"][slot] = stage["reset_obs"][e]
        state["new_frame"][e] = slot
        if reset:
            state["hist"][e, :] = slot
            state["ep_log"][e, :] = 0.0
            state["ep_ret"][e] = 0.0
            state["ep_len"][e] = 0.0
            continue
        r = np.float32(stage["reward"][e])
        state["reward"][e] = r
        state["done"][e] = 1.0 if stage["done"][e] != 0 else 0.0
        ret = np.float32(state["ep_ret"][e] + r)
        length = np.float32(state["ep_len"][e] + np.float32(1.0))
        if stage["ended"][e] != 0:
            state["ep_log"][e, 0] = ret
            state["ep_log"][e, 1] = length
            state["ep_log"][e, 2] = np.float32(state["ep_log"][e, 2] + np.float32(1.0))
            state["ep_ret"][e] = 0.0
            state["ep_len"][e] = 0.0
        else:
            state["ep_ret"][e] = ret
            state["ep_len"][e] = length


# ------------------------------------------------------------------ a recorded tape as a vector env
class TapeVectorEnv:
    """The ``HostVectorEnv`` protocol over a recorded tape: ``first_obs`` [N, obs] and a list of
    steps, each a dict with ``obs`` [N, obs] (the observation the next action is chosen from: the
    new episode's first one where ``done``), ``reward`` [N], ``done`` [N] and optionally
    ``actions`` [N]: what the step must receive, exactly.  ``ended`` = ``done``."""

    continuous = False
    action_dim = 1

    def __init__(self, first_obs, steps, n_actions: int, max_episode_steps=None):
        first_obs = np.asarray(first_obs, dtype=np.float32)
        self.n, self.obs_dim = first_obs.shape
        self.first_obs, self.steps, self.t = first_obs, steps, 0
        self.n_actions = int(n_actions)
        self.max_episode_steps = max_episode_steps
        self.staging = np.zeros(self.n * (2 * self.obs_dim + 3), dtype=np.float32)
        self.views = staging_views(self.staging, self.n, self.obs_dim)
        self.closed = False

    def __len__(self):
        return self.n

    def reset(self):
        self.views["reset_obs"][:] = self.first_obs
        return self.views["reset_obs"]

    def step(self, actions):
        s = self.steps[self.t]
        a = np.asarray(actions).reshape(-1)
        assert a.shape == (self.n,)
        if "actions" in s:
            assert np.array_equal(a, s["actions"]), (self.t, a, s["actions"])
        v = self.views
        v["next_obs"][:] = s["obs"]
        v["reset_obs"][:] = s["obs"]
        v["reward"][:] = s["reward"]
        v["done"][:] = s["done"]
        v["ended"][:] = s["done"]
        self.t += 1

    def close(self):
        self.closed = True


# ------------------------------------------------------------------ scripted deterministic envs
class ScriptedEnv(Env):
    """A deterministic gym-API env with ``obs_dim`` floats and ``n_actions`` discrete actions:
    the state rotates and decays, the action pushes one component, the reward says whether the
    action was the step's favoured one, and the episode ends after ``horizon`` steps or once a
    component leaves [-3, 3].  The reset draw comes from the env's seeded ``np_random``."""

    def __init__(self, obs_dim: int, n_actions: int, horizon: int = 13):
        super().__init__()
        self.obs_dim, self.n_actions, self.horizon = int(obs_dim), int(n_actions), int(horizon)
        big = np.full(self.obs_dim, np.finfo(np.float32).max, dtype=np.float32)
        self.observation_space = spaces.Box(-big, big, dtype=np.float32)
        self.action_space = spaces.Discrete(self.n_actions)
        self.x = np.zeros(self.obs_dim, np.float32)
        self.t = 0
        self.seen = []   # every action this env was stepped with

    def reset(self):
        self.x = self.np_random.uniform(-0.1, 0.1, size=self.obs_dim).astype(np.float32)
        self.t = 0
        return self.x.copy()

    def step(self, action):
        a = int(action)
        assert 0 <= a < self.n_actions, a
        self.seen.append(a)
        x = np.roll(self.x, 1) * np.float32(0.9)
        x[a % self.obs_dim] += np.float32(0.25 * (1 + a))
        self.x = x.astype(np.float32)
        r = (1.0 if a == self.t % self.n_actions else 0.0) - 0.125
        self.t += 1
        done = self.t >= self.horizon or bool(np.abs(self.x).max() > 3.0)
        return self.x.copy(), r, done, {}


def acrobot_like():
    """obs 6 / 3 actions: Acrobot-v1's shapes."""
    return ScriptedEnv(6, 3)


def widest():
    """obs 8 / 7 actions: the MLP kernels' limits (kVecMaxObs, kVecMaxA)."""
    return ScriptedEnv(8, 7)
