"""The bf16-operand wide MLP kernels (ops/csrc/vector_wide_bf16_kernels.hip, ``wide_dtype="bf16"``).

1. Inputs whose every operand, product and sum is exactly representable leave the kernels no rounding
   freedom: ``vecwb_act``'s Q and ``vecwb_grad``'s flat gradient equal the fp64 result bit for bit.
2. A learner step against fp64 PyTorch with ``.to(bfloat16)`` at the contract's rounding points (x, weights,
   f, h; dA | dV, dh, weights; both contraction operands): kernel error <= K_E32 * e32b, e32b the error of
   fp32 PyTorch with the same rounding points against the same fp64 reference, floored at one fp32 rounding
   (profiles/vector_wide_bf16.md).
3. Reruns and the captured learner graph are bit-equal; the fused evaluator act equals its step form.
"""
import numpy as np
import pytest
import torch

from apex_amd import ops
from apex_amd.algo.losses import _td_terms, huber_weighted, priorities_from_td

from . import actor_oracle as ao
from .test_gpu_vector_wide import _bias, _check, _host_engine, _np
from .test_gpu_vector_wide_eval import _act, _evaluator, _tape
from .vector_host_fixtures import TapeVectorEnv

pytestmark = pytest.mark.gpu

_bf = lambda t: t.to(torch.bfloat16).to(t.dtype)  # noqa: E731


def _forward(P, x):
    """Q and the stored (rounded) x, f, ha, hv of the contract, in the dtype of ``x``."""
    w0, b0, wa1, ba1, wa2, ba2, wv1, bv1, wv2, bv2 = P
    pre = [x, torch.relu(_bf(x) @ _bf(w0).T + b0)]
    f = _bf(pre[1])
    pre += [torch.relu(f @ _bf(wa1).T + ba1), torch.relu(f @ _bf(wv1).T + bv1)]
    ha, hv = _bf(pre[2]), _bf(pre[3])
    adv, val = ha @ _bf(wa2).T + ba2, hv @ _bf(wv2).T + bv2
    return val + adv - adv.mean(1, keepdim=True), (_bf(x), f, ha, hv), pre


def _sparse(gen, rows, cols, nnz, values):
    w = torch.zeros(rows, cols, dtype=torch.float64)
    for r in range(rows):
        c = torch.randperm(cols, generator=gen)[:nnz]
        w[r, c] = values[torch.randint(len(values), (len(c),), generator=gen)]
    return w


@pytest.mark.parametrize("obs,A,E", [(9, 8, 1), (33, 16, 33), (128, 32, 70)])
def test_bf16_act_is_exact_on_exact_inputs(cuda, obs, A, E):
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.vector_host import VectorHostShard
    from apex_amd.models.dqn import DuelingDQN

    gen = torch.Generator().manual_seed(obs)
    eighths = lambda *shape: torch.randint(-4, 5, shape, generator=gen).double() / 8  # noqa: E731
    x = torch.randint(-1, 2, (E, obs), generator=gen).double()
    v0, v1 = torch.tensor([-.5, -.25, -.125, .125, .25, .5]).double(), torch.tensor([-1., -.5, .5, 1.]).double()
    P = [_sparse(gen, 128, obs, 3, v0), eighths(128), _sparse(gen, 128, 128, 2, v1), eighths(128),
         _sparse(gen, A, 128, 2, v1), eighths(A), _sparse(gen, 128, 128, 2, v1), eighths(128),
         _sparse(gen, 1, 128, 2, v1), eighths(1)]
    q64, _, pre = _forward(P, x)
    # the precondition, on the fp64 reference alone: every operand has <= 8 significant bits before it is
    # rounded, and Q (never rounded to bf16) is an fp32 number
    assert all(torch.equal(_bf(t), t) for t in pre + P[0::2]) and torch.equal(q64.float().double(), q64)
    assert min(float(t.abs().max()) for t in pre) > 0
    m = DuelingDQN.from_shapes((obs,), A)
    with torch.no_grad():
        for p, v in zip(m.parameters(), P):
            p.copy_(v)
    rp = HBMReplay(4096, n_envs=E, n_step=3, device=cuda, frame_bytes=4 * obs)
    sh = VectorHostShard(rp, TapeVectorEnv(x.float().numpy(), [], A), seed=5, wide=True, wide_dtype="bf16")
    sh.set_policy(m.to(cuda))
    sh.act()
    torch.cuda.synchronize()
    assert np.array_equal(_np(sh.q).astype(np.float64), q64.numpy())
    want = ao.select_actions_ref(_np(sh.q), _np(sh.eps), sh.act_seed, int(sh.step_counter.item()))
    assert np.array_equal(_np(sh.actions), want)
    sh.close()


@pytest.mark.parametrize("B", [33, 96])
def test_bf16_grad_is_exact_on_integer_rows(cuda, B, obs=33, A=18):
    h, lay = ops.hip(), ops.hip().vecw_layout()
    gen = torch.Generator().manual_seed(B)
    vec = torch.randint(-3, 4, (B, lay["STRIDE"]), generator=gen).float()   # padding columns too: never read
    n, nblk = h.vec_param_count(obs, A), h.vecw_grad_blocks(obs, A)
    grad, part = torch.full((n,), 7.0, device=cuda), torch.zeros(nblk, dtype=torch.float64, device=cuda)
    dvec = vec.to(cuda)
    h.vecwb_grad(h.make_vecw_grad(dvec.data_ptr(), B, obs, A, n, grad.data_ptr(), part.data_ptr()),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    v = vec.double()
    cut = lambda k, w: v[:, lay[k]:lay[k] + w]  # noqa: E731
    x, f, dF, dA, dV = cut("X", obs), cut("F", 128), cut("DF", 128), cut("DA", A), cut("DV", 1)
    ha, dha = cut("H", 128), cut("DH", 128)
    hv, dhv = v[:, lay["H"] + 128:lay["H"] + 256], v[:, lay["DH"] + 128:lay["DH"] + 256]
    want = torch.cat([t.reshape(-1) for t in (dF.T @ x, dF.sum(0), dha.T @ f, dha.sum(0), dA.T @ ha, dA.sum(0),
                                              dhv.T @ f, dhv.sum(0), dV.T @ hv, dV.sum(0))])
    assert want.numel() == n and torch.equal(grad.cpu().double(), want)
    assert float(part.sum()) == float(want.pow(2).sum())


def _reference(P, T, batch, cfg, dt):
    """Q rows, loss, priorities and the ten gradient tensors with the contract's rounding points in ``dt``."""
    P, T = [p.detach().cpu().to(dt) for p in P], [p.detach().cpu().to(dt) for p in T]
    s, a, rew, s2, done, w = (t if t.dtype == torch.int64 else t.to(dt) for t in batch)
    with torch.no_grad():
        q0, (xb, f, ha, hv), _ = _forward(P, s)
        q2, qt = _forward(P, s2)[0], _forward(T, s2)[0]
    q = q0.clone().requires_grad_(True)
    td = _td_terms(q, q2, qt, a, rew, done, cfg.n_step, cfg.gamma)
    loss = huber_weighted(td, w)
    loss.backward()
    with torch.no_grad():
        dV = q.grad.sum(1, keepdim=True)
        dA = q.grad - dV / q.shape[1]
        dha = _bf((_bf(dA) @ _bf(P[4])) * (ha > 0))
        dhv = _bf((_bf(dV) @ _bf(P[8])) * (hv > 0))
        dF = (dha @ _bf(P[2]) + dhv @ _bf(P[6])) * (f > 0)
        g = [_bf(dF).T @ xb, dF.sum(0), dha.T @ f, dha.sum(0), _bf(dA).T @ ha, dA.sum(0), dhv.T @ f, dhv.sum(0),
             _bf(dV).T @ hv, dV.sum(0)]
    return (torch.cat([q0, q2, qt]).numpy(), float(loss.detach()), priorities_from_td(td).detach().numpy(),
            [t.reshape(-1).numpy() for t in g])


@pytest.mark.parametrize("obs,A,B", [(8, 7, 64), (33, 18, 33), (128, 32, 96)])
def test_bf16_learner_step_matches_fp64_with_the_same_rounding(cuda, obs, A, B):
    """Three SGD steps on a replay filled by 40 acting steps of 16 scripted host envs."""
    eng = _host_engine(cuda, obs, A, B, lr=1e-4, lr_step_size=2, lr_gamma=0.5, wide_dtype="bf16")
    L, rp, cfg = eng.learner, eng.replay, eng.cfg
    gen = torch.Generator().manual_seed(100 + B)
    _bias(L.model, gen)
    with torch.no_grad():
        L.tflat.add_(torch.randn(L.tflat.shape, generator=gen).to(cuda) * 0.05)
    eng.publish_params()
    for _ in range(40):
        eng.actor_step()
    knee = [0, 0]
    for it, shift in enumerate((0.0, -3.0, 2.5)):   # Q(s, a) near 0, -3, -0.5 straddles the Huber knee
        with torch.no_grad():
            L.model.value[2].bias.add_(shift)
        L.sample()
        L.forward_backward()
        torch.cuda.synchronize()
        assert float(L.part.sum()) == pytest.approx(float(L.flat_grad.double().pow(2).sum()), rel=1e-12)
        idx = L.idx.long()
        s, s2 = L.ring[rp.s_ids[idx, 3].long()].cpu(), L.ring[rp.s2_ids[idx, 3].long()].cpu()
        batch = (s, rp.action[idx].long().cpu(), rp.reward[idx].cpu(), s2, rp.done[idx].cpu(), L.w.cpu())
        params, tparams = list(L.model.parameters()), list(L.target.parameters())
        (q64, l64, p64, g64), (q32, l32, p32, g32) = (_reference(params, tparams, batch, cfg, dt)
                                                      for dt in (torch.float64, torch.float32))
        tag = f"bf16 learn obs={obs} A={A} B={B} it={it} "
        _check(tag + "q", np.concatenate([_np(L.q_s), _np(L.q_s2), _np(L.qt_s2)]), q32, q64)
        for (name, o, k), a64, a32 in zip(L.segments, g64, g32):
            assert np.linalg.norm(a64) > 0, name
            _check(tag + "d" + name, _np(L.flat_grad[o:o + k]), a32, a64, l2=True)
        knee = [knee[0] + int((L.delta < 1).sum()), knee[1] + int((L.delta >= 1).sum())]
        L.optimize()
        L.write_priorities()
        torch.cuda.synchronize()
        _check(tag + "loss", float(L.loss.item()), l32, l64)
        _check(tag + "prio", _np(L.prio), p32, p64)
    assert knee[0] > 0 and knee[1] > 0  # both branches of the Huber loss were taken
    eng.close()


def test_bf16_engine_reruns_and_graph_are_bit_equal(cuda):
    out = []
    for capture in (False, False, True):
        eng = _host_engine(cuda, 33, 18, seed=3, lr=1e-3, wide_dtype="bf16")
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
    assert all(torch.equal(a, b) for other in out[1:] for a, b in zip(out[0], other))


def test_bf16_fused_evaluator_act_equals_its_step_form(cuda, obs=33, A=18, N=33):
    eng = _host_engine(cuda, obs, A, seed=obs, wide_dtype="bf16")
    gen = torch.Generator().manual_seed(obs)
    _bias(eng.learner.model, gen)
    rows, tape = _tape(obs, N, 3, gen)
    fused, step = _evaluator(eng, rows, tape), _evaluator(eng, rows, tape, "step")
    for k in range(3):
        (q, act), (qs, acts) = _act(fused), _act(step)
        assert np.array_equal(q.view(np.uint32), qs.view(np.uint32)) and np.array_equal(act, acts), k
    fused.close(), step.close(), eng.close()
