"""The tall mode's host-side plumbing (no GPU): ``host_env_spec`` limits, ``VectorEngineConfig.tall_obs``
validation and the CLI's ``--tall``."""
from types import SimpleNamespace

import pytest

from apex_amd import train_vector
from apex_amd.engine.vector import VectorEngineConfig
from apex_amd.engine.vector_host import host_env_spec


def _vec(obs, A=3):
    return SimpleNamespace(obs_dim=obs, n_actions=A, continuous=False, max_episode_steps=None)


def test_host_env_spec_tall_limits():
    assert host_env_spec(_vec(1024, 32), wide=True, tall=True) == (1024, 32, None)
    with pytest.raises(ValueError, match="limit of 1024"):
        host_env_spec(_vec(1025), wide=True, tall=True)
    with pytest.raises(ValueError, match="wide"):
        host_env_spec(_vec(129), tall=True)
    with pytest.raises(ValueError, match="limit of 128"):
        host_env_spec(_vec(129), wide=True)


def test_config_takes_tall_only_with_fp32_wide_net():
    assert not VectorEngineConfig().tall_obs
    assert VectorEngineConfig(wide_net=True, tall_obs=True).validate().tall_obs
    with pytest.raises(ValueError, match="wide_net"):
        VectorEngineConfig(tall_obs=True).validate()
    with pytest.raises(ValueError, match="bf16 tall mode is out of scope"):
        VectorEngineConfig(wide_net=True, wide_dtype="bf16", tall_obs=True).validate()


def test_cli_tall_belongs_to_wide_host_envs(capsys):
    p = train_vector.parser()
    cfg = train_vector.config_from_args(p.parse_args(["--host-envs", "--wide", "--tall"]))
    assert cfg.wide_net and cfg.tall_obs
    assert not train_vector.config_from_args(p.parse_args(["--host-envs", "--wide"])).tall_obs
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--host-envs", "--tall"])
    assert e.value.code == 2 and "--wide" in capsys.readouterr().err
