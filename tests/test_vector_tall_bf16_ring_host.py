"""The bf16 observation ring's host-side plumbing (no GPU): the config, the kernel picker and the CLI."""
from types import SimpleNamespace

import pytest

from apex_amd import train_vector
from apex_amd.engine.vector import VectorEngineConfig, ring_bytes, wide_kernel
from apex_amd.engine.vector_host import host_env_spec

TALL_BF16 = dict(wide_net=True, tall_obs=True, tall_dtype="bf16")


def test_config_takes_a_bf16_ring_only_with_the_tall_bf16_kernels():
    assert VectorEngineConfig().ring_dtype == "fp32" and (ring_bytes("fp32"), ring_bytes("bf16")) == (4, 2)
    assert VectorEngineConfig(**TALL_BF16, ring_dtype="bf16").validate(device_env=False).ring_dtype == "bf16"
    for kw in (dict(), dict(wide_net=True), dict(wide_net=True, wide_dtype="bf16"), dict(wide_net=True, tall_obs=True)):
        with pytest.raises(ValueError, match="ring_dtype='bf16' is a layout of the tall bf16 kernels: set tall_obs"):
            VectorEngineConfig(**kw, ring_dtype="bf16").validate(device_env=False)
    with pytest.raises(ValueError, match="host-env engine"):   # VectorApexEngine's device envs keep fp32
        VectorEngineConfig(**TALL_BF16, ring_dtype="bf16").validate()
    with pytest.raises(ValueError, match="ring_dtype must be one of"):
        VectorEngineConfig(**TALL_BF16, ring_dtype="u8").validate(device_env=False)


@pytest.mark.parametrize("name", ["act", "learn", "grad"])
def test_wide_kernel_takes_a_bf16_ring_only_for_the_tall_bf16_launches(name):
    hip = SimpleNamespace(**{p + name: p + name for p in ("vecw_", "vecwb_", "vect_", "vectb_")})
    assert wide_kernel(hip, name, "fp32", True, "bf16", ring_dtype="bf16") == "vectb_" + name
    for args in (("fp32",), ("bf16",), ("fp32", True)):
        with pytest.raises(ValueError, match="layout of the tall bf16 kernels"):
            wide_kernel(hip, name, *args, ring_dtype="bf16")


def test_cli_ring_dtype_needs_tall_bf16_and_host_env_spec_is_unchanged(capsys):
    p, flags = train_vector.parser(), ["--host-envs", "--wide", "--tall", "--dtype", "bf16"]
    cfg = train_vector.config_from_args(p.parse_args(flags + ["--ring-dtype", "bf16"]))
    assert (cfg.tall_obs, cfg.tall_dtype, cfg.ring_dtype) == (True, "bf16", "bf16")
    assert train_vector.config_from_args(p.parse_args(flags)).ring_dtype == "fp32"
    for bad in (["--host-envs", "--wide", "--tall"], ["--host-envs", "--wide", "--dtype", "bf16"], ["--wide"]):
        with pytest.raises(SystemExit) as e:
            p.parse_args(bad + ["--ring-dtype", "bf16"])
        assert e.value.code == 2 and "--tall --dtype bf16" in capsys.readouterr().err
    assert host_env_spec(SimpleNamespace(obs_dim=1024, n_actions=32, max_episode_steps=7), True, True) == (1024, 32, 7)
