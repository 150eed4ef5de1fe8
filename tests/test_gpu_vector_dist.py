"""The categorical (C51) kernels (ops/csrc/vector_dist_kernels.hip) against fp64 PyTorch through
``DuelingDQN.dist()`` and the projection written in plain torch.  The wide kernels' convention
(tests/test_gpu_vector_wide.py): kernel error <= K_E32 * e32, e32 = fp32 PyTorch's (CPU) error against
the same fp64 reference (max-normalised; gradients: relative L2 per tensor), floored at one fp32
rounding.  The measured ratios are in profiles/vector_dist.md."""
import numpy as np
import pytest
import torch

from apex_amd import ops
from apex_amd.algo.schedules import step_scheduler_early
from apex_amd.engine.vector import VectorApexEngine, VectorEngineConfig, vec_net
from apex_amd.models.dqn import DuelingDQN

from .vector_host_fixtures import ScriptedEnv

pytestmark = pytest.mark.gpu

K_E32 = 8.0
U32 = 2.0 ** -24
VMIN, VMAX = -2.0, 3.0
GAMMA_N = 0.99 ** 3
# obs, A, atoms, rows: CartPole's shape with a ragged second tile | unaligned weight rows, one atom into tile 2,
# a ragged second workgroup | every limit | a single action, exactly one tile, B = 1 | the smallest support
CASES = [(4, 2, 51, 64), (9, 3, 33, 33), (128, 8, 64, 33), (5, 1, 32, 1), (12, 4, 2, 40)]

_np = lambda t: t.detach().cpu().numpy()  # noqa: E731


def _err(x, ref, l2=False):
    d, ref = np.asarray(x, dtype=np.float64) - np.asarray(ref, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(d) / np.linalg.norm(ref)) if l2 else float(np.abs(d).max() / np.abs(ref).max())


def _check(what, got, ref32, ref64, l2=False):
    e, e32 = _err(got, ref64, l2), max(_err(ref32, ref64, l2), U32)
    print(f"{what}: kernel {e:.3e} fp32 {e32:.3e} ratio {e / e32:.2f}")
    assert e <= K_E32 * e32, what


def _cast(model, dtype):
    """A CPU copy of ``model`` in ``dtype`` (the fp64 reference and its fp32 twin)."""
    m = DuelingDQN.from_shapes(model.input_shape, model.num_actions, atoms=model.atoms, v_min=model.v_min,
                               v_max=model.v_max).to(dtype)
    m.load_state_dict({k: v.detach().to(dtype).cpu() for k, v in model.state_dict().items()})
    return m


def _model(cuda, obs, A, atoms, seed, v=(VMIN, VMAX)):
    torch.manual_seed(seed)
    m = DuelingDQN.from_shapes((obs,), A, atoms=atoms, v_min=v[0], v_max=v[1])
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.add_(torch.randn(p.shape) * 0.2)
    m = m.to(cuda)
    m.flatten_parameters()   # value.2's rows are unaligned in the flat vector when A * atoms % 4 != 0
    return m


def _ref_learn(on, tg, s, a, r, s2, d, w, astar):
    """C51 loss terms of the batch in the models' dtype -> (lw, delta, mean loss, per-tensor gradients)."""
    rows, N = torch.arange(len(a)), on.atoms
    z, dz = on.support(s), (on.v_max - on.v_min) / (N - 1)
    with torch.no_grad():
        pt = tg.dist(s2)[rows, astar]
        b = ((r[:, None] + GAMMA_N * (1 - d)[:, None] * z[None]).clamp(on.v_min, on.v_max) - on.v_min) / dz
        m = (pt[:, :, None] * (1 - (b[:, :, None] - torch.arange(N, dtype=s.dtype)).abs()).clamp(min=0)).sum(1)
    lw = w * -(m * torch.log_softmax(on.dist_logits(s)[rows, a], -1)).sum(-1)
    delta = ((m * z).sum(-1) - on(s)[rows, a]).abs()
    on.zero_grad()
    lw.mean().backward()
    return _np(lw), _np(delta), float(lw.detach().mean()), [_np(p.grad).reshape(-1) for p in on.parameters()]


@pytest.mark.parametrize("obs,A,atoms,rows", CASES)
def test_dist_act_matches_fp64_and_the_host_eval_act(cuda, obs, A, atoms, rows):
    h, s = ops.hip(), torch.cuda.current_stream().cuda_stream
    m = _model(cuda, obs, A, atoms, obs)
    gen = torch.Generator().manual_seed(obs)
    ring = torch.randn(rows + 3, obs, generator=gen).to(cuda)
    hist = torch.zeros(rows, 4, dtype=torch.int32, device=cuda)
    hist[:, 3] = (torch.randperm(rows, generator=gen) + 3).int().to(cuda)
    eps = torch.zeros(rows, device=cuda)
    counter = torch.full((1,), 7, dtype=torch.int64, device=cuda)
    q, act = torch.zeros(rows, A, device=cuda), torch.full((rows,), -1, dtype=torch.int32, device=cuda)
    net = vec_net(h, m)
    h.vecd_act(h.make_vecw_act(net, ring.data_ptr(), hist.data_ptr(), rows, eps.data_ptr(), 11, counter.data_ptr(),
                               q.data_ptr(), act.data_ptr()), s)
    x = ring[hist[:, 3].long()]
    stage = torch.zeros(rows * (2 * obs + 3), device=cuda)
    stage[rows * obs:2 * rows * obs] = x.reshape(-1)
    q2, act2 = torch.zeros_like(q), torch.full_like(act, -1)
    h.vecd_host_eval_act(h.make_vecw_host_eval_act(net, dict(N=rows, seed=11, stage=stage.data_ptr(),
                                                             q=q2.data_ptr(), actions=act2.data_ptr())), 7, s)
    torch.cuda.synchronize()
    with torch.no_grad():
        q64, q32 = _cast(m, torch.float64)(x.cpu().double()).numpy(), _cast(m, torch.float32)(x.cpu()).numpy()
    tag = f"act obs={obs} A={A} atoms={atoms} rows={rows}"
    _check(tag, _np(q), q32, q64)
    tol = K_E32 * max(_err(q32, q64), U32) * np.abs(q64).max()
    top = np.sort(q64, 1)
    clear = np.ones(rows, bool) if A == 1 else top[:, -1] - top[:, -2] > 2 * tol
    assert clear.any() and np.array_equal(_np(act)[clear], q64.argmax(1)[clear])
    assert torch.equal(q2, q) and torch.equal(act2, act)


@pytest.mark.parametrize("obs,A,atoms,rows", CASES)
def test_dist_learn_and_grad_match_fp64(cuda, obs, A, atoms, rows):
    """A constructed batch (row kind = slot % 5): done = 1 with r on an atom | done = 1 with r halfway between two
    atoms | Tz pushed past v_max | past v_min | plain.  (rows = 1: the on-atom row alone.)"""
    h, st = ops.hip(), torch.cuda.current_stream().cuda_stream
    on, tg = _model(cuda, obs, A, atoms, 10 + obs), _model(cuda, obs, A, atoms, 20 + obs)
    gen = torch.Generator().manual_seed(atoms)
    C, i = rows, torch.arange(rows)
    z = on.support(torch.zeros(1))
    kind = i % 5
    r = torch.randn(C, generator=gen) * 0.5
    r = torch.where(kind == 0, z[(3 * i) % atoms], r)
    r = torch.where(kind == 1, 0.5 * (z[i % (atoms - 1)] + z[i % (atoms - 1) + 1]), r)
    r = torch.where(kind == 2, torch.full_like(r, 2 * (VMAX - VMIN)), r)
    r = torch.where(kind == 3, torch.full_like(r, -2 * (VMAX - VMIN)), r)
    done = ((kind < 2) | (i % 10 == 9)).float()
    ring = torch.randn(2 * C, obs, generator=gen).to(cuda)
    ids = torch.zeros(2, C, 4, dtype=torch.int32, device=cuda)
    ids[0, :, 3], ids[1, :, 3] = i.int().to(cuda), (i + C).int().to(cuda)
    action = (i * 3 % A).int().to(cuda)
    rew, dn = r.to(cuda), done.to(cuda)
    idx = torch.randperm(C, generator=gen).int().to(cuda)
    w = (torch.rand(rows, generator=gen) + 0.5).to(cuda)
    f32 = dict(dtype=torch.float32, device=cuda)
    P, nblk = h.vecd_param_count(obs, A, atoms), h.vecd_grad_blocks(obs, A, atoms)
    assert P == on._flat.numel()
    qs, qs2, qts2 = (torch.zeros(rows, A, **f32) for _ in range(3))
    vec = torch.zeros(rows, h.vecd_layout()["STRIDE"], **f32)
    delta, lw, grad = torch.zeros(rows, **f32), torch.zeros(rows, **f32), torch.full((P,), 7.0, **f32)
    part = torch.zeros(nblk, dtype=torch.float64, device=cuda)
    L = h.make_vecw_learn(vec_net(h, on), vec_net(h, tg), dict(
        ring=ring.data_ptr(), s_ids=ids[0].data_ptr(), s2_ids=ids[1].data_ptr(), action=action.data_ptr(),
        reward=rew.data_ptr(), done=dn.data_ptr(), idx=idx.data_ptr(), w=w.data_ptr(), B=rows, gamma_n=GAMMA_N,
        q_s=qs.data_ptr(), q_s2=qs2.data_ptr(), qt_s2=qts2.data_ptr(), vec=vec.data_ptr(), delta=delta.data_ptr(),
        lw=lw.data_ptr()))
    h.vecd_learn(L, st)
    h.vecd_grad(h.make_vecd_grad(vec.data_ptr(), rows, obs, A, atoms, P, grad.data_ptr(), part.data_ptr()), st)
    torch.cuda.synchronize()
    j = idx.long().cpu()
    batch = (ring[:C].cpu()[j], action.long().cpu()[j], r[j], ring[C:].cpu()[j], done[j], w.cpu())
    ref = {}
    for dt in (torch.float64, torch.float32):
        o, t = _cast(on, dt), _cast(tg, dt)
        b = tuple(x if x.dtype == torch.int64 else x.to(dt) for x in batch)
        with torch.no_grad():
            ref[dt] = np.concatenate([o(b[0]).numpy(), o(b[3]).numpy(), t(b[3]).numpy()])
    tag = f"learn obs={obs} A={A} atoms={atoms} rows={rows} "
    _check(tag + "q", np.concatenate([_np(qs), _np(qs2), _np(qts2)]), ref[torch.float32], ref[torch.float64])
    astar = qs2.argmax(1).cpu()   # the kernel's own a*: no row is excluded for a near-tie
    out = {}
    for dt in (torch.float64, torch.float32):
        b = tuple(x if x.dtype == torch.int64 else x.to(dt) for x in batch)
        out[dt] = _ref_learn(_cast(on, dt), _cast(tg, dt), *b, astar)
    (lw64, d64, l64, g64), (lw32, d32, l32, g32) = out[torch.float64], out[torch.float32]
    _check(tag + "lw", _np(lw), lw32, lw64)
    _check(tag + "delta", _np(delta), d32, d64)
    _check(tag + "loss", float(lw.mean()), l32, l64)
    for (name, o, k), a64, a32 in zip(on.param_segments(), g64, g32):
        if A == 1 and name.startswith("advantage"):   # A - mean(A) = 0: exactly no gradient
            assert not a64.any() and not _np(grad[o:o + k]).any(), name
        else:
            _check(tag + "d" + name, _np(grad[o:o + k]), a32, a64, l2=True)
    assert float(part.sum()) == pytest.approx(float(grad.double().pow(2).sum()), rel=1e-12)


def _engine(cuda, host):
    from apex_amd.engine.vector_host import VectorHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    kw = dict(batch_size=64, replay_capacity=4096, wide_net=True, dist_atoms=51, v_min=-5.0, v_max=15.0, lr=1e-4,
              lr_step_size=2, lr_gamma=0.5)
    if not host:
        return VectorApexEngine(VectorEngineConfig(env_id="CartPole-v0", n_envs=64, **kw), cuda)
    vec = HostVectorEnv([lambda: ScriptedEnv(9, 3)] * 16, seed=0, max_obs=128)
    return VectorHostEngine(VectorEngineConfig(env_id="scripted", **kw), vec, cuda, eval_env=lambda: ScriptedEnv(9, 3))


@pytest.mark.parametrize("host", [False, True], ids=["device-envs", "host-envs"])
def test_dist_engine_tracks_fp64_training(cuda, host):
    """Three learner steps: the parameters against an fp64 (and an fp32) PyTorch loop fed the same sampled indices,
    weights and a*."""
    eng = _engine(cuda, host)
    L, rp, cfg = eng.learner, eng.replay, eng.cfg
    assert GAMMA_N == pytest.approx(cfg.gamma ** cfg.n_step)
    for _ in range(30):
        eng.actor_step()
    loops = {}
    for dt in (torch.float64, torch.float32):
        o, t = _cast(L.model, dt), _cast(L.target, dt)
        opt = torch.optim.RMSprop(o.parameters(), lr=cfg.lr, alpha=cfg.rms_alpha, eps=cfg.rms_eps, centered=True)
        loops[dt] = (o, t, opt, torch.optim.lr_scheduler.StepLR(opt, step_size=cfg.lr_step_size, gamma=cfg.lr_gamma))
    for _ in range(3):
        L.sample()
        L.forward_backward()
        torch.cuda.synchronize()
        idx = L.idx.long()
        s, s2 = L.ring[rp.s_ids[idx, 3].long()].cpu(), L.ring[rp.s2_ids[idx, 3].long()].cpu()
        batch = (s, rp.action[idx].long().cpu(), rp.reward[idx].cpu(), s2, rp.done[idx].cpu(), L.w.cpu())
        astar = L.q_s2.argmax(1).cpu()
        for dt, (o, t, opt, sched) in loops.items():
            _ref_learn(o, t, *(x if x.dtype == torch.int64 else x.to(dt) for x in batch), astar)
            torch.nn.utils.clip_grad_norm_(o.parameters(), cfg.max_norm)
            step_scheduler_early(sched)
            opt.step()
        L.optimize()
        L.write_priorities()
    torch.cuda.synchronize()
    flat = {dt: torch.cat([p.detach().reshape(-1) for p in o.parameters()]).numpy() for dt, (o, *_) in loops.items()}
    _check(f"engine host={host} parameters", _np(L.flat), flat[torch.float32], flat[torch.float64])
    assert bool(torch.isfinite(L.loss).all()) and bool(torch.isfinite(L.prio).all())
    ret = eng.evaluate(episodes=3)
    assert len(ret) == 3 and np.isfinite(ret).all()
    with pytest.raises(RuntimeError if host else ValueError, match="on the host" if host else "follow-up"):
        eng.rollout_evaluate(2)
    if host:
        eng.close()
