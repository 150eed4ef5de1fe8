"""Models: checkpoint contract (keys / shapes / dtypes), param counts, differential
forward against the reference model classes, losses vs reference utils."""
import random

import numpy as np
import torch

from apex_amd.envs import make
from apex_amd.model import AQL, DuelingDQN, NoisyLinear
from apex_amd.models.dqn import env_spec

from . import goldens

ATARI_KEYS = [("features.0.weight", (32, 4, 8, 8)), ("features.0.bias", (32,)), ("features.2.weight", (64, 32, 4, 4)),
              ("features.2.bias", (64,)), ("features.4.weight", (64, 64, 3, 3)), ("features.4.bias", (64,)),
              ("advantage.0.weight", (128, 3136)), ("advantage.0.bias", (128,)), ("advantage.2.weight", (18, 128)),
              ("advantage.2.bias", (18,)), ("value.0.weight", (128, 3136)), ("value.0.bias", (128,)),
              ("value.2.weight", (1, 128)), ("value.2.bias", (1,))]


def test_dueling_state_dict_contract():
    m = DuelingDQN.from_shapes((4, 84, 84), 18)
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == ATARI_KEYS
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert sum(p.numel() for p in m.parameters()) == 883_507
    assert sum(p.numel() for p in DuelingDQN.from_shapes((4, 84, 84), 6).parameters()) == 881_959
    assert sum(p.numel() for p in DuelingDQN(make("CartPole-v0")).parameters()) == 34_051


def test_flat_parameters_keep_state_dict(tmp_path):
    m = DuelingDQN.from_shapes((4, 84, 84), 6)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    flat = m.flatten_parameters()
    assert flat.numel() == 881_959
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k])
    flat.add_(1.0)
    assert torch.equal(m.features[0].bias, before["features.0.bias"] + 1)
    torch.save(m.state_dict(), tmp_path / "model.pth")
    m2 = DuelingDQN.from_shapes((4, 84, 84), 6)
    m2.load_state_dict(torch.load(tmp_path / "model.pth", weights_only=True))
    x = torch.rand(2, 4, 84, 84) * 255
    torch.testing.assert_close(m(x), m2(x))


def test_aql_param_counts_and_keys():
    aql = AQL(make("CartPole-v0"), propose_sample=1, uniform_sample=50, device="cpu")
    assert aql.total_sample == 3 and sum(p.numel() for p in aql.parameters()) == 38_660
    keys = list(aql.state_dict())
    assert "q.advantage1.weight_epsilon" in keys and "proposal.dist_feature.2.bias" in keys
    bip = AQL(make("BipedalWalker-v3"), propose_sample=1, uniform_sample=50, device="cpu")
    assert bip.total_sample == 51 and sum(p.numel() for p in bip.parameters()) == 51_526
    a, a_mu, q = bip.act(make("BipedalWalker-v3").reset(), 0.0)
    assert a_mu.shape == (1, 51, 4) and q.shape == (1, 51)


def _dueling_forward_case():
    """Weights and input of the dueling differential test, from NumPy's legacy generator (the
    3.5 MB of Atari-sized weights are regenerated, not stored: that stream never changes)."""
    env = env_spec((4, 84, 84), 18)
    ours = DuelingDQN(env)
    rng = np.random.RandomState(11)
    with torch.no_grad():
        for p in ours.parameters():
            fan_in = p[0].numel() if p.dim() > 1 else p.numel()
            p.copy_(torch.from_numpy((rng.standard_normal(tuple(p.shape)) / np.sqrt(fan_in)).astype(np.float32)))
    x = torch.from_numpy(rng.randint(0, 256, (3, 4, 84, 84)).astype(np.float32))
    return env, ours, x


def _dueling_outputs(model, x):
    """In float64 on both sides: the recorded outputs are compared on other machines, whose
    fp32 convolutions sum in another order (8e-5 on |q| ~ 100 between two CPUs); in fp64 that
    difference is ~1e-13, far inside assert_close's fp64 tolerance of 1e-7."""
    model, x = model.double(), x.double()
    random.seed(0)
    a = model.act(x[0], 0.3)
    return {"q": model(x).detach().numpy(), "act_action": np.int64(a[0]), "act_q": np.asarray(a[1])}


def test_dueling_forward_matches_reference_model():
    """The reference's DuelingDQN with this model's state_dict loaded (strict), same input
    (recorded: tests/golden/models_dueling.npz, with the reference's own state_dict layout)."""
    g = goldens.load("models_dueling")
    env, ours, x = _dueling_forward_case()
    # their checkpoint loads into ours: same keys, order, shapes and dtypes (and ours loaded into
    # theirs when the outputs below were recorded)
    sd = {k: v.clone() for k, v in ours.state_dict().items()}
    assert list(sd) == g["ref_keys"].tolist()
    assert [list(v.shape) for v in sd.values()] == [s[s >= 0].tolist() for s in g["ref_shapes"]]
    assert [str(v.dtype) for v in sd.values()] == g["ref_dtypes"].tolist()
    ours.load_state_dict({k: torch.zeros(tuple(s[s >= 0].tolist()), dtype=getattr(torch, d.split(".")[1]))
                          for k, s, d in zip(g["ref_keys"].tolist(), g["ref_shapes"], g["ref_dtypes"].tolist())})
    ours.load_state_dict(sd)
    o = _dueling_outputs(ours, x)
    assert o["q"].dtype == g["q"].dtype == np.float64
    torch.testing.assert_close(torch.from_numpy(o["q"]), torch.from_numpy(g["q"]))
    assert o["act_action"] == g["act_action"]
    np.testing.assert_allclose(o["act_q"], g["act_q"])


AQL_FORWARD_ENVS = ("CartPole-v0", "BipedalWalker-v3")


def _aql_act(model, s):
    torch.manual_seed(7)
    np.random.seed(7)
    random.seed(7)
    r = model.act(s, 0.0)
    return {"action": np.asarray(r[0]), "a_mu": np.asarray(r[1]), "q": r[2].detach().numpy()}


def test_aql_forward_matches_reference_model():
    """The reference's AQL (propose 2 + uniform 5) acting on the same state with the same RNG
    streams; its freshly initialised state_dict is the recorded checkpoint loaded here
    (tests/golden/models_aql_<env>.npz)."""
    for env_id in AQL_FORWARD_ENVS:
        g = goldens.load("models_aql_" + env_id)
        env = make(env_id)
        ours = AQL(env, propose_sample=2, uniform_sample=5, device="cpu")
        ours.load_state_dict(goldens.get_state(g, "state"))
        r2 = _aql_act(ours, g["s"])
        assert int(g["action"]) == int(r2["action"])
        # proposals are fp32 network outputs (+ seeded noise) recorded on another machine: the
        # fp32 tolerance of the Q comparison below, not NumPy's 1e-7 (one fp32 ulp)
        np.testing.assert_allclose(g["a_mu"], r2["a_mu"], rtol=1.3e-6, atol=1e-5)
        torch.testing.assert_close(torch.from_numpy(g["q"]), torch.from_numpy(r2["q"]))


def _loss_case():
    """Models and batch of the loss differential test; the initial weights are recorded in
    tests/golden/models_loss.npz so both sides start from the same checkpoint."""
    env = make("CartPole-v0")
    torch.manual_seed(0)
    model, tgt = DuelingDQN(env), DuelingDQN(env)
    B = 32
    g = torch.Generator().manual_seed(1)
    batch = (torch.randn(B, 4, generator=g), torch.randint(0, 2, (B,), generator=g), torch.randn(B, generator=g),
             torch.randn(B, 4, generator=g), (torch.rand(B, generator=g) < 0.2).float(), torch.rand(B, generator=g))
    # float64 on both sides (see _dueling_outputs): recorded results, compared on other machines
    batch = tuple(t.double() if t.is_floating_point() else t for t in batch)
    return env, model.double(), tgt.double(), batch


def _loss_and_update(u, model, tgt, batch):
    """compute_loss + update_parameters of either implementation's utils module ``u``."""
    opt = torch.optim.RMSprop(model.parameters(), 1e-3, alpha=0.95, eps=1.5e-7, centered=True)
    loss, prios = u.compute_loss(model, tgt, batch, 3, 0.99)
    out = {"loss": loss.detach().numpy().copy(), "prios": np.asarray(prios).copy()}
    out["grad_norm"] = np.asarray(torch.as_tensor(u.update_parameters(loss, model, opt, 40)).detach().numpy())
    goldens.put_state(out, "after", model.state_dict())
    return out


def test_compute_loss_matches_reference_utils():
    """The reference's utils.compute_loss / update_parameters on the same models and batch
    (recorded: tests/golden/models_loss.npz)."""
    from apex_amd import utils

    g = goldens.load("models_loss")
    env, model, tgt, batch = _loss_case()
    model.load_state_dict(goldens.get_state(g, "model"))
    tgt.load_state_dict(goldens.get_state(g, "target"))
    assert all(p.dtype == torch.float64 for p in model.parameters())
    o = _loss_and_update(utils, model, tgt, batch)
    torch.testing.assert_close(torch.from_numpy(o["loss"]), torch.from_numpy(g["loss"]))
    np.testing.assert_allclose(o["prios"], g["prios"], rtol=1e-6)
    torch.testing.assert_close(torch.from_numpy(o["grad_norm"]), torch.from_numpy(g["grad_norm"]))
    after = goldens.get_state(g, "after")
    assert list(after) == list(model.state_dict())
    for a, b in zip(model.state_dict().values(), after.values()):
        torch.testing.assert_close(a, b)


def test_noisy_linear_modes():
    torch.manual_seed(0)
    nl = NoisyLinear(8, 4, device="cpu")
    x = torch.randn(3, 8)
    nl.train()
    y1 = nl(x)
    nl.reset_noise()
    y2 = nl(x)
    assert not torch.allclose(y1, y2)
    nl.eval()
    torch.testing.assert_close(nl(x), torch.nn.functional.linear(x, nl.weight_mu, nl.bias_mu))
    assert set(nl.state_dict()) == {"weight_mu", "weight_sigma", "weight_epsilon", "bias_mu", "bias_sigma",
                                    "bias_epsilon"}
