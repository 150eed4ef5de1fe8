"""Host-side contract of the GPU AQL.py engine (engine/aql_frame.py, trainers/aql.py --engine gpu):
the cosine schedule's closed form, config defaults and validation, the first-learning-frame rule,
the host model of the per-frame epsilon stream and the CLI switch.  No GPU."""
import inspect
import os

import numpy as np
import pytest
import torch

from apex_amd.algo.schedules import cosine_lr
from apex_amd.engine import AQLFrameConfig, AQLFrameEngine  # noqa: F401
from apex_amd.engine.aql_frame import MAX_CAND_FLOATS, MAX_T, frame_seeds, host_epsilons
from apex_amd.trainers import aql as trainer

from .actor_oracle import uniform4

EPS_SEED = 11      # cfg.seed of the GPU epsilon test (tests/test_gpu_aql_frame.py)
EPS_FRAMES = 4000


def torch_cosine(k: int, lr0: float, T_max: int, eta_min: float) -> float:
    """``CosineAnnealingLR`` stepped k times (the optimizer's lr is a Python double)."""
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr0)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_max, eta_min=eta_min)
    for _ in range(k):
        opt.step()
        sch.step()
    return float(opt.param_groups[0]["lr"])


@pytest.mark.parametrize("T_max", [10, 1000, 100_000])
def test_cosine_lr_matches_the_torch_scheduler(T_max):
    """The fp64 closed form rounded to fp32 against the scheduler's (recursive) value rounded to
    fp32: within 6e-8 relative, half an fp32 ulp."""
    lr0 = 1e-4
    eta = lr0 / 1000
    for k in (0, 1, T_max // 2, T_max - 1, T_max):
        ref = float(np.float32(torch_cosine(k, lr0, T_max, eta)))
        got = float(np.float32(cosine_lr(k, lr0, T_max, eta)))
        assert abs(got - ref) <= 6e-8 * ref, (T_max, k, got, ref)
    assert cosine_lr(0, lr0, T_max, eta) == lr0
    assert abs(cosine_lr(T_max, lr0, T_max, eta) - eta) <= 1e-18
    assert cosine_lr(7, 3e-4, T_max, 3e-4) == 3e-4   # eta_min == lr: a constant schedule, exactly


def test_config_defaults_are_aql_py():
    c = AQLFrameConfig()
    ref = {k: p.default for k, p in inspect.signature(trainer.train_AQL.__init__).parameters.items()
           if p.default is not inspect.Parameter.empty}
    assert c.env_id == "Pendulum-v0" and c.n_envs == 1
    assert c.lr == ref["lr"] == 1e-4 and c.eta_min() == 1e-4 / 1000
    assert c.batch_size == ref["batch_size"] == 32
    assert c.gamma == ref["gamma"] == 0.99
    assert c.capacity == ref["buffer_size"] == 100_000
    assert (c.propose_sample, c.uniform_sample) == (ref["propose_sample"], ref["uniform_sample"]) == (100, 100)
    assert c.action_var == ref["action_var"] == 0.25 and c.ent_lam == ref["ent_lam"] == 0.8
    assert c.alpha == ref["prior_alpha"] == 0.6 and c.beta_start == ref["prior_beta_start"] == 0.4
    assert c.target_update_interval == ref["target_update_interval"] == 1000
    assert c.save_interval == ref["save_interval"] == 10_000 and c.max_step == ref["max_step"] == 1_000_000
    assert c.max_norm == 40.0 and (c.eps_hi, c.eps_lo, c.eps_p) == (0.5, 0.05, 0.1)
    assert c.exact_mass is False and c.fused is True
    assert c.candidates() == (200, 1)
    assert c.validate() is c


def test_validate_rejects():
    assert (MAX_T, MAX_CAND_FLOATS) == (1024, 4608)
    AQLFrameConfig(propose_sample=512, uniform_sample=512).validate()                        # T = 1024, adim 1
    AQLFrameConfig(env_id="BipedalWalker-v3", propose_sample=900, uniform_sample=21).validate()  # 921 * 5 = 4605
    AQLFrameConfig(env_id="CartPole-v0", propose_sample=3).validate()                        # T = 2 + 3
    assert AQLFrameConfig(env_id="CartPole-v0", propose_sample=3).candidates() == (5, 1)
    for bad in (dict(n_envs=2), dict(n_envs=0),
                dict(propose_sample=513, uniform_sample=512),                                # T > 1024
                dict(env_id="BipedalWalker-v3", propose_sample=900, uniform_sample=22),      # 922 * 5 > 4608
                dict(propose_sample=0, uniform_sample=0),                                    # T = 0
                dict(capacity=32), dict(capacity=8, batch_size=8), dict(batch_size=0), dict(batch_size=65),
                dict(target_update_interval=0), dict(env_id="MountainCarContinuous-v0"), dict(max_step=0),
                dict(max_episode_steps=0)):
        with pytest.raises(ValueError):
            AQLFrameConfig(**bad).validate()


@pytest.mark.parametrize("B", [1, 8, 32, 64])
def test_first_learning_frame_is_the_reference_rule(B):
    """AQL.py: a frame inserts, then learns iff ``len(buffer) > batch_size``."""
    length, t = 0, 0
    while True:
        length += 1
        if length > B:
            break
        t += 1
    assert AQLFrameConfig(batch_size=B).first_learning_frame() == t == B


def test_host_epsilon_model_share():
    """The seed of the GPU epsilon test: the host model alone is inside +-4 sigma of
    Binomial(4000, 0.1), and every epsilon is one of the two values."""
    eps = host_epsilons(EPS_SEED, EPS_FRAMES, uniform4=uniform4)
    assert set(eps) == {0.5, float(np.float32(0.05))}
    share = sum(e != 0.5 for e in eps) / EPS_FRAMES
    assert 0.08 <= share <= 0.12, share
    s = frame_seeds(EPS_SEED)
    assert len({s["env"], s["prop"], s["sel"], s["eps"]}) == 4 and all(0 <= v < 1 << 48 for v in s.values())


def test_cli_engine_switch(monkeypatch, tmp_path):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as ei:
        trainer.main(["--engine", "gpu", "--env", "Pendulum-v0", "--max-step", "5", "--save-dir", str(tmp_path)])
    assert str(ei.value) == trainer.GPU_ENGINE_ERROR and "--engine gpu needs a ROCm GPU" in str(ei.value)
    assert not list(tmp_path.iterdir())
    with pytest.raises(SystemExit):
        trainer.main(["--engine", "tpu"])
    with pytest.raises(SystemExit):
        trainer.main(["--engine", "gpu", "--dis"])


def test_cli_host_engine_still_runs(monkeypatch, tmp_path):
    """``--engine host`` (the default) is the host loop: the 50-step Pendulum smoke."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.chdir(tmp_path)   # (the host trainer's writer logs under the working directory)
    trainer.main(["--engine", "host", "--env", "Pendulum-v0", "--max-step", "50", "--save-dir", str(tmp_path)])
    assert os.path.exists(tmp_path / "model0.pth") and os.path.exists(tmp_path / "model49.pth")
