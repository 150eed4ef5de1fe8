"""Host-only plumbing of ``noisy_heads``: the model and its checkpoint, ``--noisy``, the ``dqn_frame`` refusal."""
import pytest
import torch

from apex_amd import train_vector
from apex_amd.engine import vector
from apex_amd.engine.dqn import DQNEngineConfig
from apex_amd.models.dqn import DuelingDQN
from apex_amd.models.noisy import NoisyLinear


def test_noisy_model_keys_round_trip_and_a_plain_model_refuses_the_file(tmp_path):
    m = DuelingDQN.from_shapes((9,), 3, noisy=True)
    keys = ("weight_mu", "weight_sigma", "bias_mu", "bias_sigma", "weight_epsilon", "bias_epsilon")
    want = ["features.0.weight", "features.0.bias"] + [f"{l}.{k}" for l in DuelingDQN.NOISY_LAYERS for k in keys]
    assert list(m.state_dict()) == want and isinstance(m.features[0], torch.nn.Linear)
    assert all(isinstance(l, NoisyLinear) and l.std_init == 0.4 for l in m.noisy_layers())
    assert m.flatten_parameters().numel() == 128 * 9 + 128 + 2 * (2 * 128 * 128 + 2 * 128 + 3 * 128 + 3 + 128 + 1)
    assert [n for n, _, _ in m.param_segments()] == [k for k in want if "epsilon" not in k]
    path = vector.save_state_dict(m, str(tmp_path / "model.pth"))
    back = vector.load_state_dict(path, model=DuelingDQN.from_shapes((9,), 3, noisy=True)).state_dict()
    assert list(back) == want and all(torch.equal(a, b) for a, b in zip(back.values(), m.state_dict().values()))
    with pytest.raises(RuntimeError):
        vector.load_state_dict(path, model=DuelingDQN.from_shapes((9,), 3))
    assert list(DuelingDQN.from_shapes((9,), 3).state_dict()) == list(vector.PARAM_KEYS)


@pytest.mark.parametrize("flags", [[], ["--wide"], ["--wide", "--dtype", "bf16"], ["--host-envs", "--wide", "--tall"],
                                   ["--host-envs", "--wide", "--tall", "--dtype", "bf16", "--ring-dtype", "bf16"]])
def test_noisy_flag_composes_with_the_modes(flags):
    parse = lambda *f: train_vector.config_from_args(train_vector.parser().parse_args(["--env", "CartPole-v0", *f]))  # noqa: E731
    cfg, off = parse("--noisy", *flags), parse(*flags)
    assert cfg.noisy_heads and not off.noisy_heads and not vector.VectorEngineConfig().noisy_heads
    assert (cfg.wide_net, cfg.wide_dtype, cfg.tall_obs, cfg.tall_dtype, cfg.ring_dtype) == (
        off.wide_net, off.wide_dtype, off.tall_obs, off.tall_dtype, off.ring_dtype)
    with pytest.raises(SystemExit):   # the modes' own refusals stand
        parse("--noisy", "--dtype", "bf16")
    with pytest.raises(ValueError, match="noisy_heads"):   # the one-launch dqn_frame engine refuses the option
        DQNEngineConfig(noisy_heads=True).validate()
