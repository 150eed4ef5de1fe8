"""Host side of the vector engine's rollout evaluation: the ``--eval-mode`` flag of
``train_vector`` and the hand-set policies of ``tests/vector_policies.py``, which must show on
the host (fp64 net, fp32 states, envs/classic.py, host-uniform resets) what the GPU tests use
them for, and stay far inside those tests' 1 % cap on steps near a termination threshold."""
import numpy as np
import pytest

from . import vector_policies as vp


def test_eval_mode_flag():
    from apex_amd import train_vector

    p = train_vector.parser()
    assert p.parse_args([]).eval_mode == "step"
    for mode in ("step", "rollout", "async"):
        assert p.parse_args(["--eval-mode", mode]).eval_mode == mode
    assert train_vector.EVAL_MODES == ("step", "rollout", "async")
    for bad in ("sync", "", "Step"):
        with pytest.raises(SystemExit):
            p.parse_args(["--eval-mode", bad])


def _play(recipe, env_id, seed, noise, episodes=20):
    rng = np.random.default_rng(seed)
    r = vp.host_episodes(vp.make_policy(env_id, recipe, seed, noise), env_id,
                         vp.host_reset_draws(env_id, episodes, rng))
    print(recipe, env_id, seed, noise, "lengths", min(r["lengths"]), max(r["lengths"]), "ended", r["ended"],
          "actions", r["actions"].tolist(), "near", r["near"], "of", r["steps"], f"min gap {r['min_gap']:.2e}")
    # the fixtures stay within the GPU tests' cap on left-out steps by themselves, and no argmax is a near-tie
    assert r["near"] <= 0.01 * r["steps"]
    assert r["min_gap"] > 1e-4
    return r


@pytest.mark.parametrize("seed,noise", vp.SEEDS)
def test_balance_runs_to_the_time_limit(seed, noise):
    r = _play("balance", "CartPole-v0", seed, noise)
    assert r["lengths"] == [200] * 20 and r["ended"] == [2] * 20
    assert abs(int(r["actions"][0]) - int(r["actions"][1])) <= 0.02 * r["steps"]  # actions split 50/50


def test_balance_holds_for_500_steps():
    r = _play("balance", "CartPole-v1", 1, 0.02, episodes=5)
    assert r["lengths"] == [500] * 5 and r["ended"] == [2] * 5


@pytest.mark.parametrize("seed,noise", vp.SEEDS)
def test_angle_ends_by_terminals_of_differing_lengths(seed, noise):
    r = _play("angle", "CartPole-v0", seed, noise)
    assert r["ended"] == [1] * 20
    assert 15 <= min(r["lengths"]) and max(r["lengths"]) <= 100 and len(set(r["lengths"])) >= 8
    assert abs(int(r["actions"][0]) - int(r["actions"][1])) <= 0.1 * r["steps"]


@pytest.mark.parametrize("seed,noise", vp.SEEDS)
def test_pump_reaches_the_goal(seed, noise):
    r = _play("pump", "MountainCar-v0", seed, noise)
    assert r["ended"].count(1) >= 18  # (an episode or two may run to the time limit)
    assert min(r["lengths"]) >= 80 and len(set(r["lengths"])) >= 5
    assert (r["actions"] > 0).all()  # all three actions occur


def test_philox_reset_draws_lie_in_the_reset_ranges():
    c = vp.philox_reset_draws("CartPole-v0", 12, 20)
    assert c.shape == (20, 4) and (np.abs(c) <= 0.05).all() and np.unique(c).size == 80
    m = vp.philox_reset_draws("MountainCar-v0", 13, 9)
    assert m.shape == (9, 2) and ((m[:, 0] >= -0.6) & (m[:, 0] <= -0.4)).all() and (m[:, 1] == 0).all()
