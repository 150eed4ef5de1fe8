"""``wide_dtype`` / ``--dtype`` validation of the wide MLP path (no GPU)."""
import pytest

from apex_amd import train_vector
from apex_amd.engine.vector import VectorEngineConfig


def test_config_takes_bf16_only_with_wide_net():
    assert VectorEngineConfig().wide_dtype == "fp32"
    assert VectorEngineConfig(wide_net=True, wide_dtype="bf16").validate().wide_dtype == "bf16"
    with pytest.raises(ValueError, match="wide_net"):
        VectorEngineConfig(wide_dtype="bf16").validate()
    with pytest.raises(ValueError, match="wide_dtype"):
        VectorEngineConfig(wide_net=True, wide_dtype="fp16").validate()


def test_cli_dtype_belongs_to_wide(capsys):
    p = train_vector.parser()
    cfg = train_vector.config_from_args(p.parse_args(["--host-envs", "--wide", "--dtype", "bf16"]))
    assert cfg.wide_net and cfg.wide_dtype == "bf16"
    assert train_vector.config_from_args(p.parse_args(["--wide"])).wide_dtype == "fp32"
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--dtype", "bf16"])
    assert e.value.code == 2 and "--wide" in capsys.readouterr().err
