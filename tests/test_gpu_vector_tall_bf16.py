"""The tall mode's bf16-operand kernels (ops/csrc/vector_tall_bf16_kernels.hip, ``tall_dtype="bf16"``): the bf16
wide tests' contract (test_gpu_vector_wide_bf16) at the tall tests' shapes (test_gpu_vector_tall).

Against fp64 with ``.to(bfloat16)`` at the contract's rounding points the bound is ``_check``'s: kernel error <=
K_TALL_BF16 x the error of fp32 PyTorch with the same rounding points, same floors.  On inputs whose every operand,
product and sum is exactly representable -- asserted on the reference alone: fp64 with the rounding points equals
fp64 without them -- Q and the flat gradient equal fp64 bit for bit: slab seams, the zero padding, the clamped
tail loads and the ring gather have no rounding to hide behind."""
import numpy as np
import pytest
import torch

from apex_amd.models.dqn import DuelingDQN

from . import actor_oracle as ao
from . import test_gpu_vector_wide as wide
from . import test_gpu_vector_wide_bf16 as wbf
from .test_gpu_vector_tall import _exact_reference, _tall_engine
from .test_gpu_vector_wide import _bias, _check, _np
from .test_gpu_vector_wide_bf16 import _bf, _forward, _sparse
from .test_gpu_vector_wide_eval import _act, _evaluator, _tape
from .vector_host_fixtures import TapeVectorEnv

pytestmark = pytest.mark.gpu

# 2 x the worst ratio measured on an MI355X, up to a power of two (profiles/vector_tall_bf16.md), for the learner
# steps (3.63, dL/d value.2.weight at obs 260 / B 33, step 3) and for the act cases.  The act cases' worst, 3231.86
# at obs 1024 / E 70, is ONE bf16 rounding of one feature: row 17's f[40] lies 2.6e-5 of a bf16 ulp from a rounding
# midpoint in fp64, inside the fp32 accumulation error of a 1024-term sum, so the kernel's summation order rounds it
# down where fp64 -- and, on this draw, fp32 PyTorch's order -- round it up.  With that one element flipped in the
# reference the row's error is 3.5e-7; the other 69 rows are within 8.0e-7 of fp64, the other two cases' ratios
# are 0.88 and 1.00.  fp32 PyTorch meets the same flip elsewhere (its Q error at obs 260 / B 33, step 1, is 4.1e-4).
K_TALL_BF16 = 8.0
K_TALL_BF16_ACT = 8192.0


def _engine(cuda, obs, A, B=32, seed=0, vec=None, wide_dtype=None, **kw):
    return _tall_engine(cuda, obs, A, B, seed, vec, tall_dtype="bf16", **kw)


@pytest.fixture(autouse=True)
def _tall_bf16(monkeypatch):
    """The bf16 wide tests' learner-step body over a tall bf16 engine, bounded by K_TALL_BF16."""
    monkeypatch.setattr(wide, "K_E32", K_TALL_BF16)
    monkeypatch.setattr(wbf, "_host_engine", _engine)


def _shard(cuda, x, A, m):
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.vector_host import VectorHostShard

    rp = HBMReplay(4096, n_envs=len(x), n_step=3, device=cuda, frame_bytes=4 * x.shape[1])
    sh = VectorHostShard(rp, TapeVectorEnv(x, [], A), seed=5, wide=True, tall=True, tall_dtype="bf16")
    sh.set_policy(m.to(cuda))
    sh.act()
    torch.cuda.synchronize()
    return sh


def _exact_params(gen, obs, A, bv2=None):
    """Every column of features.0 carries exactly one weight (unit r owns columns r, r + 128, ...): with x in
    {-1, 0, 1} a pre-activation is a multiple of 1/8 below 5, which bf16 holds; the later layers are sparse."""
    eighths = lambda n: torch.randint(-4, 5, (n,), generator=gen).double() / 8  # noqa: E731
    v0, v1 = torch.tensor([-.5, -.25, -.125, .125, .25, .5]).double(), torch.tensor([-1., -.5, .5, 1.]).double()
    w0, c = torch.zeros(128, obs, dtype=torch.float64), torch.arange(obs)
    w0[c % 128, c] = v0[torch.randint(6, (obs,), generator=gen)]
    return [w0, eighths(128), _sparse(gen, 128, 128, 2, v1), eighths(128), _sparse(gen, A, 128, 2, v1), eighths(A),
            _sparse(gen, 128, 128, 2, v1), eighths(128), _sparse(gen, 1, 128, 2, v1),
            eighths(1) if bv2 is None else torch.tensor([bv2]).double()]


@pytest.mark.parametrize("obs,A", [(260, 16), (1024, 32)])
def test_tall_bf16_act_is_exact_on_exact_inputs(cuda, obs, A, E=33):
    gen = torch.Generator().manual_seed(obs)
    x = torch.randint(-1, 2, (E, obs), generator=gen).double()
    P = _exact_params(gen, obs, A)
    q64, _, pre = _forward(P, x)
    with torch.no_grad():
        m64 = DuelingDQN.from_shapes((obs,), A).double()
        for p, v in zip(m64.parameters(), P):
            p.copy_(v)
        # the precondition, on the reference alone: the rounding points change nothing, Q is an fp32 number
        assert torch.equal(m64(x), q64) and all(torch.equal(_bf(t), t) for t in pre + P[0::2])
    assert torch.equal(q64.float().double(), q64) and bool((P[0] != 0).any(0).all())
    assert min(float(t.abs().max()) for t in pre) > 0
    sh = _shard(cuda, x.float().numpy(), A, m64.float())
    assert np.array_equal(_np(sh.q).astype(np.float64), q64.numpy())
    want = ao.select_actions_ref(_np(sh.q), _np(sh.eps), sh.act_seed, int(sh.step_counter.item()))
    assert np.array_equal(_np(sh.actions), want)
    sh.close()


@pytest.mark.parametrize("obs,A", [(260, 16), (1024, 32)])
def test_tall_bf16_learner_is_exact_on_exact_inputs(cuda, obs, A, B=33, E=8):
    gen = torch.Generator().manual_seed(obs)
    pick = lambda vals, *shape: torch.tensor(vals)[torch.randint(len(vals), shape, generator=gen)]  # noqa: E731
    rows = torch.randint(-1, 2, (13, E, obs), generator=gen).float().numpy()
    tape = [dict(obs=rows[t + 1], reward=pick([0., 1.], E).numpy(), done=pick([0., 0., 0., 1.], E).numpy())
            for t in range(12)]
    eng = _engine(cuda, obs, A, B, vec=TapeVectorEnv(rows[0], tape, A), gamma=0.5)
    L, rp = eng.learner, eng.replay
    # Q(s, a) - y >= 1: the clipped TD error is 1, g = w / B
    P, T = _exact_params(gen, obs, A, 64.0), _exact_params(gen, obs, A, 0.0)
    with torch.no_grad():
        for net, vals in ((L.model, P), (L.target, T)):
            for p, v in zip(net.parameters(), vals):
                p.copy_(v)
    for _ in range(12):
        eng.actor_step()
    L.idx.copy_(torch.randint(len(rp), (B,), generator=gen).int())
    L.w.copy_(B * pick([.25, .125, .0625], B))
    L.forward_backward()
    torch.cuda.synchronize()
    idx = L.idx.long()
    batch = (L.ring[rp.s_ids[idx, 3].long()].cpu(), rp.action[idx].long().cpu(), rp.reward[idx].cpu(),
             L.ring[rp.s2_ids[idx, 3].long()].cpu(), rp.done[idx].cpu(), L.w.cpu())
    q64, g64 = _exact_reference(P, T, *batch, 0.125, torch.float64)
    qb, _, _, gb = wbf._reference(P, T, batch, eng.cfg, torch.float64)
    # the precondition, on the reference alone: fp64 with the rounding points equals fp64 without them
    assert np.array_equal(qb, q64.numpy()) and np.array_equal(np.concatenate(gb), g64.numpy())
    assert torch.equal(q64.float().double(), q64) and torch.equal(g64.float().double(), g64)
    assert bool((g64[:128 * obs].view(128, obs) != 0).any(0).all())   # every column of x reaches dW0
    assert torch.equal(torch.cat([L.q_s, L.q_s2, L.qt_s2]).cpu().double(), q64)
    assert torch.equal(L.flat_grad.cpu().double(), g64)
    eng.close()


# 129: one column past a multiple of 16 and of the slab's round, unaligned rows (dword loads); 260: two slabs, the
# last 4 wide, a second workgroup with one live row; 1024: four full slabs, three workgroups
@pytest.mark.parametrize("obs,A,E", [(129, 3, 1), (260, 18, 33), (1024, 32, 70)])
def test_tall_bf16_act_matches_fp64_with_the_same_rounding(cuda, obs, A, E, monkeypatch):
    monkeypatch.setattr(wide, "K_E32", K_TALL_BF16_ACT)
    gen = torch.Generator().manual_seed(obs)
    x = torch.randn(E, obs, generator=gen)
    torch.manual_seed(obs)
    m = DuelingDQN.from_shapes((obs,), A)
    _bias(m, gen)
    P = [p.detach().clone() for p in m.parameters()]
    sh = _shard(cuda, x.numpy(), A, m)
    with torch.no_grad():
        q64, q32 = _forward([p.double() for p in P], x.double())[0].numpy(), _forward(P, x)[0].numpy()
    _check(f"tall bf16 act obs={obs} A={A} E={E}", _np(sh.q), q32, q64)
    want = ao.select_actions_ref(_np(sh.q), _np(sh.eps), sh.act_seed, int(sh.step_counter.item()))
    assert np.array_equal(_np(sh.actions), want)
    sh.close()


@pytest.mark.parametrize("obs,A,B", [(129, 3, 1), (260, 18, 33), (1024, 32, 96)])
def test_tall_bf16_learner_step_matches_fp64_with_the_same_rounding(cuda, obs, A, B):
    """``test_bf16_learner_step_matches_fp64_with_the_same_rounding``'s three SGD steps (Q rows, loss, priorities,
    the ten gradient tensors, norm partials, both Huber branches) on a tall bf16 engine."""
    wbf.test_bf16_learner_step_matches_fp64_with_the_same_rounding(cuda, obs, A, B)


@pytest.mark.parametrize("N", [1, 33, 64])
def test_tall_bf16_fused_evaluator_act_equals_its_step_form(cuda, N, obs=260, A=18):
    eng = _engine(cuda, obs, A, seed=obs)
    gen = torch.Generator().manual_seed(N)
    _bias(eng.learner.model, gen)
    rows, tape = _tape(obs, N, 3, gen)
    fused, step = _evaluator(eng, rows, tape), _evaluator(eng, rows, tape, "step")
    for k in range(3):
        (q, act), (qs, acts) = _act(fused), _act(step)
        assert np.abs(q).max() > 0
        assert np.array_equal(q.view(np.uint32), qs.view(np.uint32)) and np.array_equal(act, acts), k
    fused.close(), step.close(), eng.close()


def test_tall_bf16_forward_backward_reruns_are_bit_equal(cuda, obs=1024, A=18, B=96):
    eng = _engine(cuda, obs, A, B)
    eng.fill()
    L = eng.learner
    L.sample()
    out = []
    for _ in range(2):
        L.flat_grad.fill_(7.0)
        L.forward_backward()
        torch.cuda.synchronize()
        out.append((L.flat_grad.clone(), L.part.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][1].sum()) == pytest.approx(float(out[0][0].double().pow(2).sum()), rel=1e-12)
    eng.close()


def test_tall_bf16_eager_and_graph_are_bit_equal(cuda, obs=260, A=18):
    out = []
    for capture in (False, True):
        eng = _engine(cuda, obs, A, seed=3, lr=1e-3)
        eng.fill()
        if capture:
            eng.capture(warmup_iters=3)
        while eng.learn_steps < 30:
            eng.train_step()
        torch.cuda.synchronize()
        rp = eng.replay
        out.append([t.clone() for t in (eng.learner.flat, rp.s_ids, rp.s2_ids, rp.action, rp.reward, rp.done)])
        assert (eng._g_learn is not None) == capture and bool(torch.isfinite(eng.learner.flat).all())
        eng.close()
    assert all(torch.equal(a, b) for a, b in zip(*out))
