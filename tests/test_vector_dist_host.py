"""Categorical (C51) heads of the MLP dueling DQN on the host: the model's shapes and its expected Q,
the checkpoint round trip, and every refusal of ``dist_atoms`` (no GPU)."""
import pytest
import torch

from apex_amd.engine.dqn import DQNEngineConfig
from apex_amd.engine.vector import PARAM_KEYS, VectorEngineConfig
from apex_amd.models.dqn import DuelingDQN


def test_model_shapes_keys_and_expected_q():
    torch.manual_seed(0)
    m = DuelingDQN.from_shapes((9,), 3, atoms=33, v_min=-2.0, v_max=3.0)
    sd = m.state_dict()
    assert tuple(sd) == PARAM_KEYS   # the ten keys, no support buffer
    assert sd["advantage.2.weight"].shape == (3 * 33, 128) and sd["value.2.weight"].shape == (33, 128)
    x = torch.randn(5, 9)
    p, z = m.dist(x), m.support(x)
    assert p.shape == (5, 3, 33) and z.shape == (33,)
    assert float(z[0]) == -2.0 and float(z[-1]) == pytest.approx(3.0)
    torch.testing.assert_close(p.sum(-1), torch.ones(5, 3))
    torch.testing.assert_close(m(x), (p * z).sum(-1))
    # unit a * N + z of advantage.2, the mean over actions per atom
    h = m.features(x)
    adv, val = m.advantage(h).view(5, 3, 33), m.value(h).view(5, 1, 33)
    torch.testing.assert_close(p, torch.softmax(val + adv - adv.mean(1, keepdim=True), -1))


def test_checkpoint_round_trip(tmp_path):
    torch.manual_seed(1)
    m = DuelingDQN.from_shapes((4,), 2, atoms=51, v_min=0.0, v_max=100.0)
    torch.save(m.state_dict(), tmp_path / "m.pth")
    m2 = DuelingDQN.from_shapes((4,), 2, atoms=51, v_min=0.0, v_max=100.0)
    m2.load_state_dict(torch.load(tmp_path / "m.pth"))
    x = torch.randn(3, 4)
    assert torch.equal(m(x), m2(x))


def test_atoms_zero_is_the_scalar_model():
    torch.manual_seed(2)
    a = DuelingDQN.from_shapes((4,), 2)
    torch.manual_seed(2)
    b = DuelingDQN.from_shapes((4,), 2, atoms=0)
    assert b.atoms == 0 and b.advantage[2].weight.shape == (2, 128) and b.value[2].weight.shape == (1, 128)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    with pytest.raises(ValueError, match="not a categorical model"):
        b.dist(torch.zeros(1, 4))


@pytest.mark.parametrize("kw,msg", [
    (dict(obs_shape=(4, 84, 84), atoms=51), "MLP form"),
    (dict(obs_shape=(4,), atoms=51, noisy=True), "noisy"),
    (dict(obs_shape=(4,), atoms=1), "atoms >= 2"),
    (dict(obs_shape=(4,), atoms=51, v_min=1.0, v_max=1.0), "v_min < v_max"),
])
def test_model_refusals(kw, msg):
    with pytest.raises(ValueError, match=msg):
        DuelingDQN.from_shapes(kw.pop("obs_shape"), 2, **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(), "set wide_net"),
    (dict(wide_net=True, wide_dtype="bf16"), "bf16 operands .* follow-up"),
    (dict(wide_net=True, tall_obs=True), "tall_obs is a follow-up"),
    (dict(wide_net=True, noisy_heads=True), "noisy_heads is a follow-up"),
    (dict(wide_net=True, dist_atoms=1), r"\[2, 64\]"),
    (dict(wide_net=True, dist_atoms=65), r"\[2, 64\]"),
    (dict(wide_net=True, v_min=2.0, v_max=2.0), "v_min < v_max"),
])
def test_config_refusals(kw, msg):
    with pytest.raises(ValueError, match=msg):
        VectorEngineConfig(env_id="CartPole-v0", **{"dist_atoms": 51, **kw}).validate()
    assert VectorEngineConfig(env_id="CartPole-v0", wide_net=True, dist_atoms=51).validate().dist_atoms == 51
    with pytest.raises(ValueError, match="dist_atoms is an option of the vector Ape-X engines"):
        DQNEngineConfig(env_id="CartPole-v0", dist_atoms=51).validate()


def test_cli_flags():
    from apex_amd.train_vector import config_from_args, parser

    a = parser().parse_args(["--env", "CartPole-v0", "--wide", "--atoms", "51", "--v-min", "0", "--v-max", "100"])
    cfg = config_from_args(a)
    assert (cfg.dist_atoms, cfg.v_min, cfg.v_max) == (51, 0.0, 100.0)
    for bad in (["--atoms", "51"], ["--wide", "--atoms", "51", "--noisy"],
                ["--wide", "--atoms", "51", "--eval-mode", "rollout"]):
        with pytest.raises(SystemExit):
            parser().parse_args(["--env", "CartPole-v0", *bad])
