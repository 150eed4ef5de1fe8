"""The tall mode of the wide MLP kernels (ops/csrc/vector_tall_kernels.hip, ``tall_obs``: 128 < obs <= 1024).

Against fp64 the bound is ``test_gpu_vector_wide``'s, kernel error <= K_TALL x the error of fp32 PyTorch (CPU)
against the same fp64 reference with the same floors; K_TALL is twice the worst ratio measured on an MI355X
over all cases here, up to a power of two (profiles/vector_tall.md).  On inputs whose every product and sum is
an fp32 number -- asserted: fp32 PyTorch equals fp64 there -- the Q rows and the flat gradient equal fp64 bit
for bit: slab seams, padding and the ring gather have no rounding to hide behind."""
import numpy as np
import pytest
import torch

from apex_amd.models.dqn import DuelingDQN

from . import actor_oracle as ao
from . import test_gpu_vector_wide as wide
from .test_gpu_vector_wide import _bias, _cast, _check, _err, _np
from .test_gpu_vector_wide_eval import _act, _evaluator, _tape
from .vector_host_fixtures import ScriptedEnv, TapeVectorEnv

pytestmark = pytest.mark.gpu

# 2 x the worst per-step ratio measured on an MI355X over all cases, up to a power of two (profiles/vector_tall.md:
# 7.21, dL/d value.2.bias at obs 260 / B 33, step 3: kernel 4.3e-7 -- the error of that step's Q rows, 5.7e-7, which
# the sum of the clipped TD errors inherits -- against an fp32 draw under the floor of one rounding, 6.0e-8.  Every
# other quantity of every case stays within 2.3; the wide test's worst, 3.62, is the same tensor)
K_TALL = 16.0


def _tall_engine(cuda, obs, A, B=32, seed=0, vec=None, **kw):
    from apex_amd.engine.vector import VectorEngineConfig
    from apex_amd.engine.vector_host import VectorHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    vec = vec if vec is not None else HostVectorEnv([lambda: ScriptedEnv(obs, A)] * 16, seed=seed, max_obs=1024)
    cfg = VectorEngineConfig(env_id="scripted", batch_size=B, replay_capacity=4096, wide_net=True, tall_obs=True,
                             seed=seed, **kw)
    return VectorHostEngine(cfg, vec, cuda)


@pytest.fixture(autouse=True)
def _tall(monkeypatch):
    """The wide tests' checks and learner-step body over a tall engine, bounded by K_TALL."""
    monkeypatch.setattr(wide, "K_E32", K_TALL)
    monkeypatch.setattr(wide, "_host_engine", _tall_engine)


# 129: one column past the first slab, unaligned weight rows; 260: three slabs, the last 4 wide, obs % 8 == 4, a second
# workgroup with one live row; 1024: every slab full, three workgroups
@pytest.mark.parametrize("obs,A,E", [(129, 3, 1), (260, 18, 33), (1024, 32, 70)])
def test_tall_act_matches_fp64_and_the_draw(cuda, obs, A, E):
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.vector_host import VectorHostShard

    gen = torch.Generator().manual_seed(obs)
    first = torch.randn(E, obs, generator=gen).numpy()
    rp = HBMReplay(4096, n_envs=E, n_step=3, device=cuda, frame_bytes=4 * obs)
    sh = VectorHostShard(rp, TapeVectorEnv(first, [], A), seed=5, wide=True, tall=True)
    torch.manual_seed(obs)
    m = DuelingDQN.from_shapes((obs,), A)
    _bias(m, gen)
    sh.set_policy(m.to(cuda))
    sh.act()
    torch.cuda.synchronize()
    x = sh.observe().cpu()
    assert np.array_equal(_np(x), first)
    with torch.no_grad():
        q64, q32 = _cast(m, torch.float64)(x.double()).numpy(), _cast(m, torch.float32)(x).numpy()
    assert _err(q32, q64) > 0
    _check(f"tall act obs={obs} A={A} E={E}", _np(sh.q), q32, q64)
    want = ao.select_actions_ref(_np(sh.q), _np(sh.eps), sh.act_seed, int(sh.step_counter.item()))
    assert np.array_equal(_np(sh.actions), want)
    sh.close()


@pytest.mark.parametrize("obs,A,B", [(129, 3, 1), (260, 18, 33), (1024, 32, 96)])
def test_tall_learner_step_matches_fp64(cuda, obs, A, B):
    """``test_wide_learner_step_matches_fp64``'s three SGD steps (Q rows, loss, priorities, the ten gradient
    tensors, norm partials, optimizer) on a tall engine."""
    wide.test_wide_learner_step_matches_fp64(cuda, obs, A, B)


def _exact_reference(P, T, s, a, rew, s2, done, w, gamma_n, dt):
    """Q(s) | Q(s') | Q_target(s') and the flat gradient in ``dt``, the kernels' formulas operation for operation."""
    P, T = [p.to(dt) for p in P], [p.to(dt) for p in T]
    s, rew, s2, done, w = (t.to(dt) for t in (s, rew, s2, done, w))

    def fwd(N, x):
        f = torch.relu(x @ N[0].T + N[1])
        ha, hv = torch.relu(f @ N[2].T + N[3]), torch.relu(f @ N[6].T + N[7])
        adv, val = ha @ N[4].T + N[5], hv @ N[8].T + N[9]
        return val + adv - adv.sum(1, keepdim=True) / adv.shape[1], f, ha, hv

    (q, f, ha, hv), q2, qt = fwd(P, s), fwd(P, s2)[0], fwd(T, s2)[0]
    B, A, ar = q.shape[0], q.shape[1], torch.arange(q.shape[0])
    y = rew + gamma_n * qt[ar, q2.argmax(1)] * (1 - done)
    g = w / B * (q[ar, a] - y).clamp(-1, 1)
    dV = g[:, None]
    dA = dV * (torch.nn.functional.one_hot(a, A).to(dt) - 1 / A)
    dha, dhv = (dA @ P[4]) * (ha > 0), (dV @ P[8]) * (hv > 0)
    dF = (dha @ P[2] + dhv @ P[6]) * (f > 0)
    grads = (dF.T @ s, dF.sum(0), dha.T @ f, dha.sum(0), dA.T @ ha, dA.sum(0), dhv.T @ f, dhv.sum(0), dV.T @ hv,
             dV.sum(0))
    return torch.cat([q, q2, qt]), torch.cat([t.reshape(-1) for t in grads])


@pytest.mark.parametrize("obs,A", [(260, 16), (1024, 32)])
def test_tall_learner_is_exact_on_exact_inputs(cuda, obs, A, B=33, E=8):
    gen = torch.Generator().manual_seed(obs)
    pick = lambda vals, *shape: torch.tensor(vals)[torch.randint(len(vals), shape, generator=gen)]  # noqa: E731

    def sparse(rows, cols, vals, nnz=2):
        w = torch.zeros(rows, cols)
        for r in range(rows):
            w[r, torch.randperm(cols, generator=gen)[:nnz]] = pick(vals, nnz)
        return w

    def params(bv2):   # features.0 dense: every observation column and every slab seam carries weight
        eighths = lambda n: torch.randint(-4, 5, (n,), generator=gen) / 8  # noqa: E731
        v = [-1., -.5, .5, 1.]
        return [pick([-.5, -.25, -.125, .125, .25, .5], 128, obs), eighths(128), sparse(128, 128, v), eighths(128),
                sparse(A, 128, v), eighths(A), sparse(128, 128, v), eighths(128), sparse(1, 128, v),
                torch.tensor([bv2])]

    rows = torch.randint(-1, 2, (13, E, obs), generator=gen).float().numpy()
    tape = [dict(obs=rows[t + 1], reward=pick([0., 1.], E).numpy(), done=pick([0., 0., 0., 1.], E).numpy())
            for t in range(12)]
    eng = _tall_engine(cuda, obs, A, B, vec=TapeVectorEnv(rows[0], tape, A), gamma=0.5)
    L, rp = eng.learner, eng.replay
    P, T = params(64.0), params(0.0)   # Q(s, a) - y >= 1: the clipped TD error is 1, g = w / B
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
    (q64, g64), (q32, g32) = (_exact_reference(P, T, *batch, 0.125, dt) for dt in (torch.float64, torch.float32))
    assert torch.equal(q32.double(), q64) and torch.equal(g32.double(), g64)   # the precondition
    assert bool((g64[:128 * obs].view(128, obs) != 0).any(0).all())   # every column of x reaches dW0
    assert torch.equal(torch.cat([L.q_s, L.q_s2, L.qt_s2]).cpu().double(), q64)
    assert torch.equal(L.flat_grad.cpu().double(), g64)
    eng.close()


@pytest.mark.parametrize("N", [1, 33, 64])
def test_tall_fused_evaluator_act_equals_its_step_form(cuda, N, obs=260, A=18):
    eng = _tall_engine(cuda, obs, A, seed=obs)
    gen = torch.Generator().manual_seed(N)
    _bias(eng.learner.model, gen)
    rows, tape = _tape(obs, N, 3, gen)
    fused, step = _evaluator(eng, rows, tape), _evaluator(eng, rows, tape, "step")
    for k in range(3):
        (q, act), (qs, acts) = _act(fused), _act(step)
        assert np.abs(q).max() > 0
        assert np.array_equal(q.view(np.uint32), qs.view(np.uint32)) and np.array_equal(act, acts), k
    fused.close(), step.close(), eng.close()


def test_tall_forward_backward_reruns_are_bit_equal(cuda, obs=1024, A=18, B=96):
    eng = _tall_engine(cuda, obs, A, B)
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
