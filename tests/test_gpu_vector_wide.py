"""The wide MLP dueling DQN kernels (ops/csrc/vector_wide_kernels.hip) against fp64 PyTorch.  Each
quantity, each step: kernel error <= K_E32 * e32, e32 = fp32 PyTorch's (CPU) error against the same
fp64 reference (max-normalised; gradients: relative L2 per tensor), floored at one fp32 rounding
since an exact quantity (the clipped dL/dV) has e32 = 0.  At B = 1 loss, priority and gradients are
the one TD error times exact factors; there alone e32 is also floored at the Q rows' fp32 error
over |td| (twice for the loss: td^2, or |td| - 1/2 >= |td| / 2); profiles/vector_wide.md."""
import numpy as np
import pytest
import torch

from apex_amd.algo.losses import compute_loss_device
from apex_amd.algo.schedules import step_scheduler_early
from apex_amd.models.dqn import DuelingDQN

from . import actor_oracle as ao
from .vector_host_fixtures import ScriptedEnv, TapeVectorEnv

pytestmark = pytest.mark.gpu

# 2 x the worst per-step ratio measured on an MI355X over all cases, up to a power of two
# (profiles/vector_wide.md: 3.62, dL/d value.2.bias at B = 64, kernel 2.6e-7 against fp32 7.3e-8)
K_E32 = 8.0
U32 = 2.0 ** -24


_np = lambda t: t.detach().cpu().numpy()  # noqa: E731


def _err(x, ref, l2=False):
    d, ref = np.asarray(x, dtype=np.float64) - np.asarray(ref, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(d) / np.linalg.norm(ref)) if l2 else float(np.abs(d).max() / np.abs(ref).max())


def _cast(model, dtype):
    m = DuelingDQN.from_shapes(model.input_shape, model.num_actions).to(dtype)
    m.load_state_dict({k: v.detach().to(dtype).cpu() for k, v in model.state_dict().items()})
    return m


def _check(what, got, ref32, ref64, l2=False, floor=U32):
    e, e32 = _err(got, ref64, l2), max(_err(ref32, ref64, l2), floor)
    print(f"{what}: kernel {e:.3e} fp32 {e32:.3e} ratio {e / e32:.2f}")
    assert e <= K_E32 * e32, what


def _bias(model, gen):
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bias"):
                p.add_(torch.randn(p.shape, generator=gen).to(p.device) * 0.2)


@pytest.mark.parametrize("obs,A,E", [(9, 8, 1), (33, 18, 33), (128, 32, 70)])
def test_wide_act_matches_fp64_and_the_draw(cuda, obs, A, E):
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.vector_host import VectorHostShard

    gen = torch.Generator().manual_seed(obs)
    first = torch.randn(E, obs, generator=gen).numpy()
    rp = HBMReplay(4096, n_envs=E, n_step=3, device=cuda, frame_bytes=4 * obs)
    sh = VectorHostShard(rp, TapeVectorEnv(first, [], A), seed=5, wide=True)
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
    _check(f"act obs={obs} A={A} E={E}", _np(sh.q), q32, q64)
    want = ao.select_actions_ref(_np(sh.q), _np(sh.eps), sh.act_seed, int(sh.step_counter.item()))
    assert np.array_equal(_np(sh.actions), want)
    sh.close()


def _host_engine(cuda, obs, A, B=32, seed=0, **kw):
    from apex_amd.engine.vector import VectorEngineConfig
    from apex_amd.engine.vector_host import VectorHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    vec = HostVectorEnv([lambda: ScriptedEnv(obs, A)] * 16, seed=seed, max_obs=128)
    cfg = VectorEngineConfig(env_id="scripted", batch_size=B, replay_capacity=4096, wide_net=True, seed=seed, **kw)
    return VectorHostEngine(cfg, vec, cuda)


@pytest.mark.parametrize("obs,A,B", [(8, 7, 64), (9, 8, 1), (33, 18, 33), (128, 32, 96)])
def test_wide_learner_step_matches_fp64(cuda, obs, A, B):
    """Three SGD steps on a replay filled by 40 acting steps of 16 scripted host envs."""
    eng = _host_engine(cuda, obs, A, B, lr=1e-4, lr_step_size=2, lr_gamma=0.5)
    L, rp, cfg = eng.learner, eng.replay, eng.cfg
    gen = torch.Generator().manual_seed(100 + B)
    _bias(L.model, gen)
    with torch.no_grad():
        L.tflat.add_(torch.randn(L.tflat.shape, generator=gen).to(cuda) * 0.05)
    eng.publish_params()
    for _ in range(40):
        eng.actor_step()
    ref_p = [p.detach().clone().requires_grad_(True) for p in L.model.parameters()]
    opt = torch.optim.RMSprop(ref_p, lr=cfg.lr, alpha=cfg.rms_alpha, eps=cfg.rms_eps, centered=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=cfg.lr_step_size, gamma=cfg.lr_gamma)
    knee = [0, 0]
    # |n-step return| < 0.4 for nearly every row: Q(s, a) near 0, -3, -0.5 straddles the Huber knee
    for it, shift in enumerate((0.0, -3.0, 2.5)):
        with torch.no_grad():
            L.model.value[2].bias.add_(shift)
            ref_p[-1].add_(shift)
        L.sample()
        L.forward_backward()
        L.hip.grad_sumsq(L.flat_grad.data_ptr(), L.P, L.partials.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert float(L.part.sum()) == pytest.approx(float(L.partials.sum()), rel=1e-12)
        assert float(L.part.sum()) == pytest.approx(float(L.flat_grad.double().pow(2).sum()), rel=1e-12)
        idx = L.idx.long()
        s, s2 = L.ring[rp.s_ids[idx, 3].long()].cpu(), L.ring[rp.s2_ids[idx, 3].long()].cpu()
        batch = (s, rp.action[idx].long().cpu(), rp.reward[idx].cpu(), s2, rp.done[idx].cpu(), L.w.cpu())
        ref = {}
        for dt in (torch.float64, torch.float32):
            on, tg = _cast(L.model, dt), _cast(L.target, dt)
            b = tuple(t if t.dtype == torch.int64 else t.to(dt) for t in batch)
            loss, prio = compute_loss_device(on, tg, b, cfg.n_step, cfg.gamma)
            loss.backward()
            with torch.no_grad():
                q = np.concatenate([on(b[0]).numpy(), on(b[3]).numpy(), tg(b[3]).numpy()])
            ref[dt] = (q, float(loss.detach()), prio.numpy(), [p.grad.reshape(-1).numpy() for p in on.parameters()])
        (q64, l64, p64, g64), (q32, l32, p32, g32) = ref[torch.float64], ref[torch.float32]
        tag = f"learn obs={obs} A={A} B={B} it={it} "
        assert (e32q := _err(q32, q64)) > 0  # (below: prio = |td| + 1e-6 at B = 1)
        td_floor = max(U32, e32q * np.abs(q64).max() / (float(p64[0]) - 1e-6)) if B == 1 else U32
        _check(tag + "q", np.concatenate([_np(L.q_s), _np(L.q_s2), _np(L.qt_s2)]), q32, q64)
        grad = L.flat_grad.clone()
        for (name, o, k), a64, a32 in zip(L.segments, g64, g32):
            assert np.linalg.norm(a64) > 0, name
            _check(tag + "d" + name, _np(grad[o:o + k]), a32, a64, l2=True, floor=td_floor)
        knee = [knee[0] + int((L.delta < 1).sum()), knee[1] + int((L.delta >= 1).sum())]
        for p, (_, o, k) in zip(ref_p, L.segments):
            p.grad = grad[o:o + k].view_as(p).clone()
        l2 = torch.nn.utils.clip_grad_norm_(ref_p, cfg.max_norm)
        step_scheduler_early(sched)
        opt.step()
        L.optimize()
        L.write_priorities()
        torch.cuda.synchronize()
        _check(tag + "loss", float(L.loss.item()), l32, l64, floor=2 * td_floor if B == 1 else U32)
        _check(tag + "prio", _np(L.prio), p32, p64, floor=td_floor)
        torch.testing.assert_close(L.norms[0], l2, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(L.flat, torch.cat([p.detach().reshape(-1) for p in ref_p]), rtol=1e-5, atol=1e-6)
    assert knee[0] > 0 and knee[1] > 0  # both branches of the Huber loss were taken
    eng.close()


def test_wide_engine_reruns_and_graph_are_bit_equal(cuda):
    out = []
    for capture in (False, False, True):
        eng = _host_engine(cuda, 33, 18, seed=3, lr=1e-3)
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
