"""Host side of the AQL rollout tests: the ``train_aql --eval-mode`` flag, and self-checks of
the fixtures the GPU tests (``test_gpu_aql_rollout``) rely on."""
import pytest

from apex_amd import train_aql

from . import aql_rollout_fixtures as fx


def test_eval_mode_flag():
    p = train_aql.parser()
    assert train_aql.EVAL_MODES == ("host", "rollout", "async")
    assert p.parse_args([]).eval_mode == "host"                       # today's evaluator stays the default
    for m in train_aql.EVAL_MODES:
        assert p.parse_args(["--eval-mode", m]).eval_mode == m
    with pytest.raises(SystemExit):
        p.parse_args(["--eval-mode", "step"])
    assert p.parse_args(["--gpus", "2"]).eval_mode == "host"
    assert p.parse_args(["--gpus", "2", "--eval-mode", "host"]).gpus == 2


@pytest.mark.parametrize("mode", ["rollout", "async"])
def test_eval_mode_rejected_with_several_gpus(mode, capsys):
    with pytest.raises(SystemExit) as e:
        train_aql.parser().parse_args(["--gpus", "2", "--eval-mode", mode])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--eval-mode" in err and "--gpus 2" in err


def test_device_evaluator_names_are_exported():
    from apex_amd import engine
    from apex_amd.engine.aql import AQLEngine

    for name in ("AQLEvaluator", "AQLRolloutBuffers", "AQLEngine"):
        assert hasattr(engine, name)
    for name in ("evaluate", "rollout_evaluate"):
        assert callable(getattr(AQLEngine, name))


@pytest.mark.parametrize("seed", fx.CARTPOLE_SEEDS)
def test_cartpole_fixture_self_check(seed):
    """The GPU tests' CartPole weights and env seeds, on the host alone: the greedy episodes have
    different lengths (the rollout's row masking is exercised), and at most 1 % of the steps land
    within 1e-4 of a termination threshold -- the cap of the steps the GPU env check leaves out."""
    lengths, steps, near = fx.host_cartpole_episodes(fx.host_cartpole_model(), seed, 9)
    print(seed, lengths, steps, near)
    assert len(set(lengths[:8])) > 1, lengths
    assert near <= 0.01 * steps, (near, steps)
