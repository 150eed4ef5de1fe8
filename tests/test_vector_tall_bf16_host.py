"""The bf16 tall mode's host-side plumbing (no GPU): ``VectorEngineConfig.tall_dtype`` validation, the kernel
picker and the CLI's ``--tall --dtype bf16``."""
from types import SimpleNamespace

import pytest

from apex_amd import train_vector
from apex_amd.engine.vector import VectorEngineConfig, wide_kernel


def test_config_takes_tall_dtype_only_with_fp32_tall_obs():
    assert VectorEngineConfig().tall_dtype == "fp32"
    assert VectorEngineConfig(wide_net=True, tall_obs=True, tall_dtype="bf16").validate().tall_dtype == "bf16"
    with pytest.raises(ValueError, match="tall_obs"):
        VectorEngineConfig(wide_net=True, tall_dtype="bf16").validate()
    with pytest.raises(ValueError, match="tall_dtype='bf16'"):   # the refusal of the old spelling points here
        VectorEngineConfig(wide_net=True, wide_dtype="bf16", tall_obs=True).validate()
    with pytest.raises(ValueError, match="out of scope"):
        VectorEngineConfig(wide_net=True, wide_dtype="bf16", tall_obs=True, tall_dtype="bf16").validate()
    with pytest.raises(ValueError, match="tall_dtype must be one of"):
        VectorEngineConfig(wide_net=True, tall_obs=True, tall_dtype="fp16").validate()


@pytest.mark.parametrize("name", ["act", "host_eval_act", "learn", "grad"])
def test_wide_kernel_picks_the_bf16_tall_launches(name):
    hip = SimpleNamespace(**{p + name: p + name for p in ("vecw_", "vecwb_", "vect_", "vectb_")})
    assert wide_kernel(hip, name, "fp32", True, "bf16") == "vectb_" + name
    assert wide_kernel(hip, name, "fp32", True) == "vect_" + name
    assert wide_kernel(hip, name, "bf16") == "vecwb_" + name
    with pytest.raises(ValueError, match="tall=True"):
        wide_kernel(hip, name, "fp32", False, "bf16")
    with pytest.raises(ValueError, match="out of scope"):
        wide_kernel(hip, name, "bf16", True)


def test_cli_tall_bf16_maps_to_tall_dtype(capsys):
    p = train_vector.parser()
    cfg = train_vector.config_from_args(p.parse_args(["--host-envs", "--wide", "--tall", "--dtype", "bf16"]))
    assert (cfg.wide_net, cfg.wide_dtype, cfg.tall_obs, cfg.tall_dtype) == (True, "fp32", True, "bf16")
    cfg = train_vector.config_from_args(p.parse_args(["--host-envs", "--wide", "--dtype", "bf16"]))
    assert (cfg.wide_dtype, cfg.tall_obs, cfg.tall_dtype) == ("bf16", False, "fp32")
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--host-envs", "--tall", "--dtype", "bf16"])
    assert e.value.code == 2 and "--wide" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--host-envs", "--wide", "--tall", "--dtype", "bf16", "--eval-envs", "4"])
    assert e.value.code == 2
