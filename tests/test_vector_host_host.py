"""Host side of the host-env vector engine (``engine/vector_host.py``): ``host_env_spec``, the
numpy model of ``vec_host_tail`` against real host envs, and the ``train_vector`` flags."""
import numpy as np
import pytest

from apex_amd import envs
from apex_amd.envs.host_vector import HostVectorEnv

from . import vector_host_fixtures as fx


# ------------------------------------------------------------------ host_env_spec
def test_host_env_spec_accepts():
    from apex_amd.engine.vector_host import host_env_spec

    assert host_env_spec(HostVectorEnv([fx.acrobot_like] * 2)) == (6, 3, None)
    assert host_env_spec(HostVectorEnv([fx.widest] * 3)) == (8, 7, None)
    assert host_env_spec(HostVectorEnv("CartPole-v0", 2)) == (4, 2, 200)
    assert host_env_spec(fx.TapeVectorEnv(np.zeros((2, 1), np.float32), [], 1, max_episode_steps=9)) == (1, 1, 9)


def test_host_env_spec_refuses():
    from apex_amd.engine.vector_host import host_env_spec

    with pytest.raises(ValueError, match="discrete"):
        host_env_spec(HostVectorEnv("Pendulum-v0", 2))
    with pytest.raises(ValueError, match=r"limit of 8 \(kVecMaxObs\)"):
        host_env_spec(HostVectorEnv([lambda: fx.ScriptedEnv(9, 3)]))
    with pytest.raises(ValueError, match=r"limit of 7 \(kVecMaxA\)"):
        host_env_spec(HostVectorEnv([lambda: fx.ScriptedEnv(4, 8)]))


# ------------------------------------------------------------------ the tail model on real envs
def _drive(cap: int, steps: int = 500, E: int = 3, seed: int = 4):
    """``HostVectorEnv("CartPole-v0", E)`` under random actions through the numpy tail model, next
    to ``E`` envs of the same seeds stepped by hand with plain Python bookkeeping.  Returns the
    per-step records: (model state copies, the hand-kept episode ends of the step)."""
    vec = HostVectorEnv("CartPole-v0", E, seed=seed, max_episode_length=cap)
    obs, F = vec.obs_dim, 2 * E + 3
    st = fx.tail_state(E, obs, F)
    vec.reset()
    fx.tail_model(st, dict(reset_obs=vec.reset_obs), reset=True)
    sim = [envs.make("CartPole-v0") for _ in range(E)]
    for i, e in enumerate(sim):
        e.seed(seed + i)
    cur = [np.asarray(e.reset(), dtype=np.float32) for e in sim]
    assert np.array_equal(st["ring"][st["new_frame"]], np.stack(cur))
    assert (st["hist"] == st["new_frame"][:, None]).all()
    ret, length, count = [0.0] * E, [0] * E, [0] * E
    rng = np.random.RandomState(1)
    out = []
    for t in range(steps):
        a = rng.randint(0, 2, size=E).astype(np.int32)
        vec.step(a)
        fx.tail_model(st, dict(reset_obs=vec.reset_obs, reward=vec.reward, done=vec.done, ended=vec.ended))
        st["step"] += 1   # (nstep_emit's bump)
        ends = []
        for i, e in enumerate(sim):
            o, r, d, _ = e.step(int(a[i]))
            ret[i] += float(r)
            length[i] += 1
            capped = length[i] >= cap
            assert st["done"][i] == float(d) and st["reward"][i] == np.float32(r)
            if d or capped:
                count[i] += 1
                ends.append((i, bool(d), capped))
                assert st["ep_log"][i].tolist() == [ret[i], float(length[i]), float(count[i]), 0.0], (t, i)
                assert st["ep_ret"][i] == 0 and st["ep_len"][i] == 0
                ret[i], length[i] = 0.0, 0
                cur[i] = np.asarray(e.reset(), dtype=np.float32)
            else:
                assert st["ep_ret"][i] == ret[i] and st["ep_len"][i] == length[i]
                cur[i] = np.asarray(o, dtype=np.float32)
            assert vec.ended[i] == float(d or capped)
            slot = ((t + 1) * E + i) % F
            assert st["new_frame"][i] == slot and np.array_equal(st["ring"][slot], cur[i]), (t, i)
        out.append(ends)
    return st, out, count


def test_tail_model_logs_true_episode_returns_and_lengths():
    st, ends, count = _drive(cap=50000)
    n = sum(len(x) for x in ends)
    assert n >= 15 and all(d and not capped for x in ends for _, d, capped in x)   # CartPole's own ends only
    assert st["ep_log"][:, 2].tolist() == [float(c) for c in count] and min(count) >= 3
    assert (st["ep_log"][:, 0] == st["ep_log"][:, 1]).all()   # CartPole: return == length


def test_tail_model_done_against_ended_under_a_cap_of_7():
    st, ends, count = _drive(cap=7)
    caps = [x for step in ends for x in step if x[2] and not x[1]]
    assert len(caps) >= 150     # (of at most 3 * 500 // 7 = 213: most episodes are cut at 7 steps) ...
    assert (st["ep_log"][:, 1] <= 7).all() and sum(count) == sum(len(x) for x in ends)
    # ... and a cap reset never set done (each step's done was compared with the env's own flag in _drive)


# ------------------------------------------------------------------ the CLI's flags
def test_parser_host_flags():
    from apex_amd import train_vector

    p = train_vector.parser()
    a = p.parse_args(["--host-envs", "--env", "Acrobot-v1", "--learner-steps", "4", "--host-serial"])
    assert a.host_envs and a.env == "Acrobot-v1" and a.learner_steps == 4 and a.host_serial
    assert a.max_episode_length == 50000 and a.eval_mode == "step"
    assert p.parse_args(["--host-envs", "--max-episode-length", "9"]).max_episode_length == 9
    d = p.parse_args([])
    assert not d.host_envs and d.learner_steps == 1 and not d.host_serial and d.env == "MountainCar-v0"
    for bad in (["--host-envs", "--eval-mode", "rollout"], ["--host-envs", "--eval-mode", "async"],
                ["--env", "Acrobot-v1"], ["--env", "Pendulum-v0"]):
        with pytest.raises(SystemExit) as ei:
            p.parse_args(bad)
        assert ei.value.code == 2, bad
