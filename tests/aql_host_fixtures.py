"""Fixtures of the host-env AQL engine tests (``test_gpu_aql_host``): a scripted vector env of
the ``HostVectorEnv`` protocol and a numpy model of ``aql_host_tail``."""
import numpy as np

from apex_amd.envs.host_vector import staging_views


class ScriptedVec:
    """The ``HostVectorEnv`` protocol over a list of prepared steps.  A step is a dict with
    ``next_obs`` / ``reset_obs`` [N, obs], ``reward`` / ``done`` / ``ended`` [N] and optionally
    ``env_act`` [N, adim]: the actions the step must receive, bit for bit."""

    def __init__(self, first_obs, steps, continuous, action_dim, n_actions, low=None, high=None,
                 max_episode_steps=None):
        first_obs = np.asarray(first_obs, dtype=np.float32)
        self.n, self.obs_dim = first_obs.shape
        self.first_obs, self.steps, self.t = first_obs, steps, 0
        self.continuous, self.action_dim, self.n_actions = bool(continuous), int(action_dim), int(n_actions)
        self.low = np.zeros(1, np.float32) if low is None else np.asarray(low, np.float32)
        self.high = np.zeros(1, np.float32) if high is None else np.asarray(high, np.float32)
        self.max_episode_steps = max_episode_steps
        self.staging = np.zeros(self.n * (2 * self.obs_dim + 3), dtype=np.float32)
        self.views = staging_views(self.staging, self.n, self.obs_dim)
        self.received = []

    def __len__(self):
        return self.n

    def reset(self):
        self.views["reset_obs"][:] = self.first_obs
        return self.views["reset_obs"]

    def step(self, actions):
        assert actions.shape == (self.n, self.action_dim) and actions.dtype == np.float32
        s = self.steps[self.t]
        if "env_act" in s:
            want = np.asarray(s["env_act"], dtype=np.float32)
            assert np.array_equal(actions.view(np.uint32), want.view(np.uint32)), (self.t, actions, want)
        self.received.append(actions.copy())
        for k in ("next_obs", "reset_obs", "reward", "done", "ended"):
            self.views[k][:] = s[k]
        self.t += 1


def tail_model(state: dict, step: dict, amu: np.ndarray, act_idx: np.ndarray, capacity: int, log_cap: int) -> None:
    """``aql_host_tail`` in numpy, env by env: ``state`` holds the replay tables ``st`` / ``st2`` /
    ``action`` / ``reward`` / ``done`` / ``a_mu``, ``filled``, ``obs_buf``, ``ep_len``, ``ep_ret``
    (fp32), ``ep_count`` and ``ep_log``; all updated in place.  Episodes that end in one step are
    logged in env order (the kernel's order among them is its waves')."""
    E = state["obs_buf"].shape[0]
    f = int(state["filled"])
    for e in range(E):
        slot = (f + e) % capacity
        state["st"][slot] = state["obs_buf"][e]
        state["st2"][slot] = step["next_obs"][e]
        state["a_mu"][slot] = amu[e]
        state["action"][slot] = act_idx[e]
        r = np.float32(step["reward"][e])
        state["reward"][slot] = r
        state["done"][slot] = 1.0 if step["done"][e] != 0 else 0.0
        length = int(state["ep_len"][e]) + 1
        if step["ended"][e] != 0:
            k = int(state["ep_count"]) % log_cap
            state["ep_log"][k, 0] = np.float32(state["ep_ret"][e]) + r
            state["ep_log"][k, 1] = np.float32(length)
            state["ep_count"] += 1
            state["ep_len"][e] = 0
            state["ep_ret"][e] = 0.0
        else:
            state["ep_len"][e] = length
            state["ep_ret"][e] = np.float32(state["ep_ret"][e]) + r
        state["obs_buf"][e] = step["reset_obs"][e]
    state["filled"] += E
