"""``HostVectorEnv`` against a plain per-env loop written here, and the ``train_aql
--host-envs`` flag combinations the parser refuses."""
import numpy as np
import pytest

from apex_amd import envs, train_aql
from apex_amd.envs import spaces
from apex_amd.envs.host_vector import HostVectorEnv, staging_views

N, SEED = 3, 11


def _actions(env_id: str, steps: int, adim: int) -> np.ndarray:
    rng = np.random.RandomState(5)
    if env_id.startswith("CartPole"):
        return rng.randint(0, 2, size=(steps, N, adim)).astype(np.float32)
    return rng.uniform(-1.5, 1.5, size=(steps, N, adim)).astype(np.float32)   # (past the bounds too)


def _plain_loop(env_id: str, actions: np.ndarray, cap: int):
    """The reference worker's loop, one env at a time: (next_obs, reset_obs, reward, done, ended)
    per step, and the first observations."""
    es = [envs.make(env_id) for _ in range(N)]
    for i, e in enumerate(es):
        e.seed(SEED + i)
    first = np.stack([np.asarray(e.reset(), dtype=np.float32) for e in es])
    length = [0] * N
    out = []
    for a in actions:
        row = []
        for i, e in enumerate(es):
            act = int(a[i, 0]) if spaces.is_discrete(e.action_space) else a[i].astype(np.float32).reshape(
                e.action_space.shape)
            o, r, d, _ = e.step(act)
            o = np.asarray(o, dtype=np.float32)
            length[i] += 1
            ended = bool(d) or length[i] >= cap
            nxt = np.asarray(e.reset(), dtype=np.float32) if ended else o
            if ended:
                length[i] = 0
            row.append((o, nxt, np.float32(r), np.float32(bool(d)), np.float32(ended)))
        out.append(row)
    return first, out


@pytest.mark.parametrize("env_id,cap,steps", [("CartPole-v0", 50000, 120), ("CartPole-v0", 7, 40),
                                              ("MountainCarContinuous-v0", 50000, 60),
                                              ("MountainCarContinuous-v0", 9, 40)])
def test_matches_a_plain_loop(env_id, cap, steps):
    vec = HostVectorEnv(env_id, N, seed=SEED, max_episode_length=cap)
    assert len(vec) == N and vec.max_episode_length == cap
    acts = _actions(env_id, steps, vec.action_dim)
    first, want = _plain_loop(env_id, acts, cap)
    got_first = vec.reset()
    assert got_first is vec.reset_obs and np.array_equal(got_first, first)      # per-env seeds seed + i
    assert len({tuple(r) for r in first}) == N                                  # (the seeds differ: so do the starts)
    n_done = n_cap = 0
    for a, rows in zip(acts, want):
        assert vec.step(a) is None
        for i, (o, nxt, r, d, ended) in enumerate(rows):
            assert np.array_equal(vec.next_obs[i], o) and np.array_equal(vec.reset_obs[i], nxt)
            assert vec.reward[i] == r and vec.done[i] == d and vec.ended[i] == ended
            n_done += int(d)
            if ended and not d:   # a length-cap reset keeps the env's flag
                n_cap += 1
                assert vec.done[i] == 0.0 and not np.array_equal(vec.next_obs[i], vec.reset_obs[i])
            if not ended:
                assert np.array_equal(vec.next_obs[i], vec.reset_obs[i])
    if env_id.startswith("CartPole") and cap > 100:
        assert n_done > 0          # terminal observation in next_obs, the new episode's first in reset_obs
    if cap < 100:
        assert n_cap > 0


def test_attributes_and_staging():
    cp = HostVectorEnv("CartPole-v0", 2, seed=0)
    assert (cp.obs_dim, cp.continuous, cp.action_dim, cp.n_actions, cp.max_episode_steps) == (4, False, 1, 2, 200)
    mc = HostVectorEnv([lambda: envs.make("MountainCarContinuous-v0")] * 4, seed=0)
    assert (len(mc), mc.obs_dim, mc.continuous, mc.action_dim, mc.n_actions) == (4, 2, True, 1, 1)
    assert mc.max_episode_steps == 999 and mc.max_episode_length == 50000
    assert mc.low.dtype == np.float32 and mc.low.tolist() == [-1.0] and mc.high.tolist() == [1.0]
    st = mc.staging
    assert st.dtype == np.float32 and st.flags.c_contiguous and st.shape == (4 * (2 * 2 + 3),)
    v = staging_views(st, 4, 2)
    for name, shape in (("next_obs", (4, 2)), ("reset_obs", (4, 2)), ("reward", (4,)), ("done", (4,)),
                        ("ended", (4,))):
        assert v[name].shape == shape and np.shares_memory(v[name], st)
        assert np.shares_memory(getattr(mc, name), v[name])
    offs = [v[k].ctypes.data - st.ctypes.data for k in ("next_obs", "reset_obs", "reward", "done", "ended")]
    assert offs == [0, 32, 64, 80, 96]            # one block, in this order
    import inspect

    import apex_amd.envs.host_vector as hv
    assert "import torch" not in inspect.getsource(hv) and "torch" not in vars(hv)   # a worker pool can wrap it


class _Recorder(envs.Env):
    """An env that records what ``step`` was handed."""

    def __init__(self, space, obs=3):
        super().__init__()
        self.action_space = space
        self.observation_space = spaces.Box(-np.ones(obs, np.float32), np.ones(obs, np.float32))
        self.got = []

    def reset(self):
        return np.zeros(self.observation_space.shape, np.float32)

    def step(self, a):
        self.got.append(a)
        return np.zeros(self.observation_space.shape, np.float64), 1, False, {}


def test_action_casts():
    d = HostVectorEnv([lambda: _Recorder(spaces.Discrete(5))] * 2)
    d.reset()
    d.step(np.array([[3.0], [0.0]], dtype=np.float32))
    assert [e.got for e in d.envs] == [[3], [0]] and all(type(e.got[0]) is int for e in d.envs)
    assert d.next_obs.dtype == np.float32 and d.reward.tolist() == [1.0, 1.0]
    b = HostVectorEnv([lambda: _Recorder(spaces.Box(-1.0, 1.0, shape=(3,)))] * 2)
    b.reset()
    a = np.arange(6, dtype=np.float64).reshape(2, 3)
    b.step(a)
    for i, e in enumerate(b.envs):
        (got,) = e.got
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (3,)
        assert got.tolist() == a[i].tolist() and not np.shares_memory(got, b.staging)
    assert b.max_episode_steps is None


def test_size_limits():
    with pytest.raises(ValueError, match="64"):
        HostVectorEnv([lambda: _Recorder(spaces.Discrete(2), obs=65)])
    with pytest.raises(ValueError, match="8"):
        HostVectorEnv([lambda: _Recorder(spaces.Box(-1.0, 1.0, shape=(9,)))])
    HostVectorEnv([lambda: _Recorder(spaces.Box(-1.0, 1.0, shape=(8,)), obs=64)])   # the limits themselves pass
    with pytest.raises(ValueError):
        HostVectorEnv("CartPole-v0", 0)
    with pytest.raises(ValueError):
        HostVectorEnv([])


def test_host_env_flags():
    p = train_aql.parser()
    a = p.parse_args(["--host-envs", "--env", "MountainCarContinuous-v0"])
    assert a.host_envs and a.n_envs == 10 and a.max_episode_length == 50000 and not a.host_serial
    assert p.parse_args([]).n_envs == 256 and not p.parse_args([]).host_envs
    assert p.parse_args(["--host-envs", "--n-envs", "4", "--host-serial"]).n_envs == 4
    assert p.parse_args(["--host-envs", "--eval-mode", "host"]).eval_mode == "host"


@pytest.mark.parametrize("extra,words", [(["--eval-mode", "rollout"], ("--eval-mode rollout", "--host-envs")),
                                         (["--eval-mode", "async"], ("--eval-mode async", "--host-envs")),
                                         (["--gpus", "2"], ("--gpus 2", "--host-envs")),
                                         (["--overlap"], ("--overlap", "--host-envs"))])
def test_host_env_flag_combinations_rejected(extra, words, capsys):
    with pytest.raises(SystemExit) as e:
        train_aql.parser().parse_args(["--host-envs", *extra])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert all(w in err for w in words), err


def test_gpu_engine_error_points_to_host_envs():
    from apex_amd.engine.aql import AQLEngine, AQLEngineConfig

    with pytest.raises(ValueError, match="--host-envs") as e:
        AQLEngine(AQLEngineConfig(env_id="MountainCarContinuous-v0"), "cpu")
    assert "GPU AQL env must be one of" in str(e.value) and "AQLHostEngine" in str(e.value)
