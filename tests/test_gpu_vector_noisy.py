"""NoisyNet heads (ops/csrc/vector_noisy_kernels.hip, ``noisy_heads``) against fp64 PyTorch fed the noise READ BACK
from the device; bounds and helpers are the modes' own: K x the error of fp32 PyTorch against the same fp64."""
import math

import numpy as np
import pytest
import torch

from apex_amd import ops
from apex_amd.algo.losses import compute_loss_device
from apex_amd.algo.schedules import step_scheduler_early
from apex_amd.engine.vector import MLPDQNLearner, VectorApexEngine, VectorEngineConfig
from apex_amd.models.dqn import DuelingDQN

from . import test_gpu_vector_wide as wide
from . import test_gpu_vector_wide_bf16 as wbf
from .test_gpu_vector_tall import K_TALL
from .test_gpu_vector_wide import _check, _np
from .vector_host_fixtures import ScriptedEnv

pytestmark = pytest.mark.gpu

MODES = {"narrow": {}, "wide": dict(wide_net=True), "wide_bf16": dict(wide_net=True, wide_dtype="bf16"),
         "tall": dict(wide_net=True, tall_obs=True), "tall_bf16": dict(wide_net=True, tall_obs=True, tall_dtype="bf16")}
CASES = [("narrow", 4, 2, 5), ("wide", 9, 3, 5), ("wide", 128, 32, 33), ("wide_bf16", 9, 3, 5),
         ("wide_bf16", 128, 32, 33), ("tall", 260, 3, 33), ("tall_bf16", 260, 3, 33)]


def _ulps(a, b):
    return int((a.contiguous().view(torch.int32) - b.contiguous().view(torch.int32)).abs().max())


def _eff(m):
    """The ten effective tensors of noisy model ``m`` in its dtype: mu + sigma * eps of the buffers it holds."""
    out = [m.features[0].weight, m.features[0].bias]
    for l in m.noisy_layers():
        out += [torch.addcmul(l.weight_mu, l.weight_sigma, l.weight_epsilon),
                torch.addcmul(l.bias_mu, l.bias_sigma, l.bias_epsilon)]
    return [t.detach() for t in out]


def _cast(m, dt):
    c = DuelingDQN.from_shapes(m.input_shape, m.num_actions, noisy=True).to(dt)
    c.load_state_dict({k: v.detach().to(dt).cpu() for k, v in m.state_dict().items()})
    return c.train()


@pytest.mark.parametrize("obs,A", [(2, 2), (9, 3), (128, 32)])
def test_compose_three_nets_in_one_launch_and_the_noise_statistics(cuda, obs, A):
    h, s = ops.hip(), torch.cuda.current_stream().cuda_stream
    ms = [DuelingDQN.from_shapes((obs,), A, noisy=True).to(cuda) for _ in range(3)]
    hs = [DuelingDQN.from_shapes((obs,), A).to(cuda) for _ in range(3)]
    step = torch.full((1,), 5, dtype=torch.int64, device=cuda)
    sets = [dict(master=m.flatten_parameters().data_ptr(), eff=p.flatten_parameters().data_ptr(), net=i,
                 **MLPDQNLearner._eps_ptrs(m)) for i, (m, p) in enumerate(zip(ms, hs))]
    draw = lambda: h.vecn_compose(h.make_vecn_compose(sets, obs, A, 1, 12, step.data_ptr(), 0), s)  # noqa: E731
    noise = lambda m: [t.clone() for l in m.noisy_layers() for t in (l.weight_epsilon, l.bias_epsilon)]  # noqa: E731
    draw()
    for m, p in zip(ms, hs):
        for l, (wk, bk) in zip(m.noisy_layers(), zip(list(p.parameters())[2::2], list(p.parameters())[3::2])):
            E = l.weight_epsilon.double()
            i, j = divmod(int(E.abs().argmax()), E.shape[1])   # rank 1: every 2 x 2 minor through the pivot vanishes
            torch.testing.assert_close(E * E[i, j], torch.outer(E[:, j], E[i, :]), rtol=3e-7, atol=0)
            assert _ulps(wk, torch.addcmul(l.weight_mu.double(), l.weight_sigma.double(), E).float()) <= 1
            assert _ulps(bk, torch.addcmul(l.bias_mu.double(), l.bias_sigma.double(), l.bias_epsilon.double()).float()) <= 1
        assert torch.equal(p._flat[:128 * obs + 128], m._flat[:128 * obs + 128])   # features.0, bit for bit
    seen = [noise(m) for m in ms]
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[1][0], seen[2][0])   # the nets differ
    draw()   # the same seed, net and step: the same noise
    assert all(torch.equal(a, b) for sn, m in zip(seen, ms) for a, b in zip(sn, noise(m)))
    h.vecn_compose(h.make_vecn_compose(sets[:1], obs, A, 0), s)   # noise = 0: mu, bit for bit
    want = [ms[0].features[0].weight, ms[0].features[0].bias] + [t for l in ms[0].noisy_layers() for t in (l.weight_mu, l.bias_mu)]
    assert all(torch.equal(a, b) for a, b in zip(hs[0].parameters(), want))
    if obs < 128:
        return
    # eps_in / eps_out are fixed by weight_epsilon only up to a common scale, so the marginals are taken over the bias
    # draws, single draws of the same generator (4335: 289 per net, 3 nets, 5 steps; 0.05 is 5.4 standard errors of
    # mean e^2, 3.7 of mean e), and the product's over 30 draws of a 128 x 128 weight_epsilon (2 / pi +- 0.011)
    e, w2 = [], []
    for _ in range(5):
        step += 1
        draw()
        e += [l.bias_epsilon.double().cpu() for m in ms for l in m.noisy_layers()]
        w2 += [float(l.weight_epsilon.double().pow(2).mean()) for m in ms for l in (m.advantage[0], m.value[0])]
    e = torch.cat(e)
    print(f"n {e.numel()} mean e {float(e.mean()):.4f} mean e^2 {float(e.pow(2).mean()):.4f} weights {np.mean(w2):.4f}")
    # distinct keys give distinct draws up to fp32 birthday collisions (4335^2 / 2 / 2^24 = 0.6 expected)
    assert e.numel() >= 4096 and e.unique().numel() >= e.numel() - 8 and abs(np.mean(w2) - 2 / math.pi) < 0.05
    assert abs(float(e.pow(2).mean()) - math.sqrt(2 / math.pi)) < 0.05 and abs(float(e.mean())) < 0.05


def _engine(cuda, mode, obs, A, B, **kw):
    from apex_amd.engine.vector_host import VectorHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    big = dict(max_obs=1024 if "tall" in mode else 128) if mode != "narrow" else {}
    vec = HostVectorEnv([lambda: ScriptedEnv(obs, A)] * 16, seed=0, **big)
    cfg = VectorEngineConfig(env_id="scripted", batch_size=B, replay_capacity=4096, noisy_heads=True, **MODES[mode], **kw)
    eng = VectorHostEngine(cfg, vec, cuda)
    with torch.no_grad():   # a target that differs from the online net
        eng.learner.tflat.add_(torch.randn(eng.learner.tflat.shape, generator=torch.Generator().manual_seed(B)).to(cuda) * 0.05)
    eng.learner.refresh_effective()
    [eng.actor_step() for _ in range(10)]
    return eng


def _reference(on, tg, L, rp, cfg, bf16):
    """Q rows, loss, priorities, the 18 master gradients in the dtype of ``on``, the device's noise loaded first."""
    dt = next(on.parameters()).dtype
    for dst, src in ((on, L.model), (tg, L.target)):
        for a, b in zip(dst.noisy_layers(), src.noisy_layers()):
            a.weight_epsilon.copy_(b.weight_epsilon)
            a.bias_epsilon.copy_(b.bias_epsilon)
    idx = L.idx.long()
    s, s2 = L.ring[rp.s_ids[idx, 3].long()].float().cpu(), L.ring[rp.s2_ids[idx, 3].long()].float().cpu()
    b = (s, rp.action[idx].long().cpu(), rp.reward[idx].cpu(), s2, rp.done[idx].cpu(), L.w.cpu())
    b = tuple(t if t.dtype == torch.int64 else t.to(dt) for t in b)
    if bf16:
        q, loss, prio, g = wbf._reference(_eff(on), _eff(tg), b, cfg, dt)
        gm = g[:2]
        for k, l in enumerate(on.noisy_layers()):   # d mu = g, d sigma = g * eps
            gm += [g[2 + 2 * k], g[2 + 2 * k] * l.weight_epsilon.reshape(-1).numpy(), g[3 + 2 * k], g[3 + 2 * k] * l.bias_epsilon.numpy()]
        return q, loss, prio, gm
    on.zero_grad()   # (the caller's learner sets p.grad: backward must not add to it)
    loss, prio = compute_loss_device(on, tg, b, cfg.n_step, cfg.gamma)
    loss.backward()
    q = np.concatenate([m(x).detach().numpy() for m, x in ((on, b[0]), (on, b[3]), (tg, b[3]))])
    return q, float(loss.detach()), prio.numpy(), [p.grad.reshape(-1).numpy().copy() for p in on.parameters()]


@pytest.mark.parametrize("mode,obs,A,B", CASES)
def test_noisy_three_sgd_steps_match_fp64_with_a_target_sync(cuda, mode, obs, A, B, monkeypatch):
    """An fp64 learner (and the fp32 one that sets the bound) fed the read-back noise; step 0: every quantity."""
    monkeypatch.setattr(wide, "K_E32", K_TALL if mode == "tall" else wide.K_E32)
    eng = _engine(cuda, mode, obs, A, B, lr=1e-4, max_norm=1e-3)   # (the clip is active)
    L, rp, cfg = eng.learner, eng.replay, eng.cfg
    refs, tag = {}, f"noisy {mode} obs={obs} A={A} B={B} "
    for dt in (torch.float64, torch.float32):
        on, tg = _cast(L.model, dt), _cast(L.target, dt)
        opt = torch.optim.RMSprop(on.parameters(), lr=cfg.lr, alpha=cfg.rms_alpha, eps=cfg.rms_eps, centered=True)
        refs[dt] = (on, tg, opt, torch.optim.lr_scheduler.StepLR(opt, step_size=cfg.lr_step_size, gamma=cfg.lr_gamma))
    for it in range(3):
        L.sample()
        L.forward_backward()
        torch.cuda.synchronize()
        (q64, l64, p64, g64), (q32, l32, p32, g32) = (_reference(on, tg, L, rp, cfg, "bf16" in mode)
                                                      for on, tg, _, _ in refs.values())
        if it == 0:
            _check(tag + "q", np.concatenate([_np(L.q_s), _np(L.q_s2), _np(L.qt_s2)]), q32, q64)
            for (name, o, k), a64, a32 in zip(L.segments, g64, g32):
                assert np.linalg.norm(a64) > 0, name
                _check(tag + "d" + name, _np(L.flat_grad[o:o + k]), a32, a64, l2=True)
            n_master = math.sqrt(sum(float((g ** 2).sum()) for g in g64))
            n_eff = math.sqrt(sum(float((g ** 2).sum()) for (name, _, _), g in zip(L.segments, g64) if "sigma" not in name))
            assert n_master > 1.1 * n_eff   # (on the reference alone: the optimizer must get the master's norm)
            assert float(L.npart.sum()) == pytest.approx(float(L.flat_grad.double().pow(2).sum()), rel=1e-12)
            assert math.sqrt(float(L.npart.sum())) == pytest.approx(n_master, rel=0.05)
        for (on, tg, opt, sched), g in zip(refs.values(), (g64, g32)):
            for p, a in zip(on.parameters(), g):
                p.grad = torch.as_tensor(a).view_as(p).clone()
            torch.nn.utils.clip_grad_norm_(on.parameters(), cfg.max_norm)
            step_scheduler_early(sched)
            opt.step()
        L.optimize()
        L.compose()
        L.write_priorities()
        torch.cuda.synchronize()
        if it == 0:
            l2 = math.sqrt(float(L.npart.sum()))
            assert float(L.norms[0]) == pytest.approx(l2, rel=1e-6)
            assert float(L.norms[2]) == pytest.approx(cfg.max_norm / (l2 + 1e-6), rel=1e-5) and float(L.norms[2]) < 1
            _check(tag + "loss", float(L.loss.item()), l32, l64)
            _check(tag + "prio", _np(L.prio), p32, p64)
        if it == 1:
            L.sync_target()
            for on, tg, _, _ in refs.values():
                tg.load_state_dict(on.state_dict())
            torch.cuda.synchronize()
            assert torch.equal(L.tflat, L.flat)
            for m, p in ((L.target, L.tnet_model), (L.model, L.net_model)):   # the invariant, both nets
                assert all(_ulps(a, b.float()) <= 1 for a, b in zip(p.parameters(), _eff(_cast(m, torch.float64).to(cuda))))
    flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()  # noqa: E731
    _check(tag + "master after 3 steps", _np(L.flat), flat(refs[torch.float32][0]), flat(refs[torch.float64][0]))
    eng.close()


def test_noisy_evaluation_is_greedy_on_mu_and_graph_replays_redraw(cuda):
    cfg = VectorEngineConfig(env_id="CartPole-v0", n_envs=16, replay_capacity=4096, noisy_heads=True, seed=3)
    eng, plain = VectorApexEngine(cfg, cuda), VectorApexEngine(VectorEngineConfig(env_id="CartPole-v0", n_envs=16, replay_capacity=4096), cuda)
    eng.fill()
    eng.capture(warmup_iters=2)
    L, seen = eng.learner, []
    for _ in range(3):
        eng.train_step()
        torch.cuda.synchronize()
        seen.append(L.model.advantage[0].weight_epsilon.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])   # replays draw by the device counter
    eng.publish_params()
    nets = [m.advantage[0].weight_epsilon for m in (L.model, L.target, L.actor_noise)]
    assert not torch.equal(nets[0], nets[1]) and not torch.equal(nets[0], nets[2]) and not torch.equal(nets[1], nets[2])
    mu = [L.model.features[0].weight, L.model.features[0].bias] + [t for l in L.model.noisy_layers() for t in (l.weight_mu, l.bias_mu)]
    plain.learner.flat.copy_(torch.cat([t.detach().reshape(-1) for t in mu]))
    for fn in ("evaluate", "rollout_evaluate"):
        assert getattr(eng, fn)(3, seed=7) == getattr(plain, fn)(3, seed=7)
