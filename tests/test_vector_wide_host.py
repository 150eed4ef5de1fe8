"""The wide MLP path's host-side plumbing (no GPU): ``host_env_spec`` limits, ``HostVectorEnv``'s
``max_obs`` and the CLI's refusal of ``--wide --eval-envs``."""
from types import SimpleNamespace

import pytest

from apex_amd import train_vector
from apex_amd.engine.vector_host import host_env_spec
from apex_amd.envs.host_vector import HostVectorEnv

from .vector_host_fixtures import ScriptedEnv


def _vec(obs, A):
    return SimpleNamespace(obs_dim=obs, n_actions=A, continuous=False, max_episode_steps=None)


@pytest.mark.parametrize("obs,A,wide,ok", [(9, 3, True, True), (128, 32, True, True), (129, 3, True, False),
                                           (9, 33, True, False), (9, 3, False, False), (8, 8, False, False)])
def test_host_env_spec_limits(obs, A, wide, ok):
    call = (lambda: host_env_spec(_vec(obs, A), wide=True)) if wide else (lambda: host_env_spec(_vec(obs, A)))
    if ok:
        assert call() == (obs, A, None)
    else:
        with pytest.raises(ValueError, match="limit"):
            call()


def test_host_vector_env_max_obs():
    with pytest.raises(ValueError, match="limit of 64"):
        HostVectorEnv([lambda: ScriptedEnv(128, 32)])
    vec = HostVectorEnv([lambda: ScriptedEnv(128, 32)] * 2, max_obs=128)
    assert host_env_spec(vec, wide=True)[:2] == (128, 32)


def test_cli_refuses_wide_with_eval_envs(capsys):
    p = train_vector.parser()
    assert train_vector.config_from_args(p.parse_args(["--host-envs", "--wide"])).wide_net
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--host-envs", "--wide", "--eval-envs", "4"])
    assert e.value.code == 2 and "narrow only" in capsys.readouterr().err
