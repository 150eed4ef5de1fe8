"""GPU DQN.py engine (engine/dqn.py, dqn_frame in ops/csrc/vector_kernels.hip): the device
schedules, the fused frame kernel against the launches it fuses, the max-priority insert and
its tree walk, the PER's running max, one SGD step against fp64 PyTorch, the loop's cadences,
graph = eager, determinism and the CLI.

Bit-equal means ``torch.equal``.  fp64 comparisons use test_gpu_vector_engine.py's figures
(max|x - ref| / max|ref|; gradients: relative L2 norm, worst tensor) and its bounds: the learner
kernels are the same, unchanged."""
import functools
import json

import numpy as np
import pytest
import torch

from apex_amd.algo.losses import compute_loss_device
from apex_amd.algo.schedules import beta_by_frame, epsilon_by_frame, step_scheduler_early
from apex_amd.models.dqn import DuelingDQN

pytestmark = pytest.mark.gpu

Q_BOUND, LOSS_BOUND, PRIO_BOUND, GRAD_BOUND = 3e-6, 8e-7, 2e-6, 2e-6   # test_gpu_vector_engine.py
FRAMES = 300
ENVS = ["CartPole-v0", "MountainCar-v0"]


def _np(t):
    return t.detach().cpu().numpy()


def _rel(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-30))


def _engine(cuda, env_id, E, C, biased=True, **kw):
    from apex_amd.engine.dqn import DQNEngineConfig, DQNFrameEngine

    if env_id.startswith("MountainCar"):
        kw.setdefault("max_episode_steps", 20)   # so that resets occur
    eng = DQNFrameEngine(DQNEngineConfig(env_id=env_id, n_envs=E, replay_capacity=C, **kw), cuda)
    if biased:  # non-zero biases (the init's are zero)
        torch.manual_seed(7 + E)
        with torch.no_grad():
            for name, p in eng.model.named_parameters():
                if name.endswith("bias"):
                    p.add_(torch.randn_like(p) * 0.2)
    return eng


# ------------------------------------------------------------------ schedules
def test_device_schedules_match_host_within_one_ulp(cuda):
    """eps(t) and beta(t) of frames 0..2000 against algo/schedules.py rounded to fp32: at most
    1 fp32 ulp apart (the device's fp64 exp may differ from libm's in the last place)."""
    n = 2001
    eng = _engine(cuda, "CartPole-v0", 1, 4160)
    eng.learning = False
    eps = torch.zeros(n, device=cuda)
    beta = torch.zeros(n, device=cuda)
    for t in range(n):
        eng.frame()
        eps[t:t + 1].copy_(eng.eps)
        beta[t:t + 1].copy_(eng.beta)
    torch.cuda.synchronize()
    c = eng.cfg
    ref_e = np.array([epsilon_by_frame(t, c.eps_start, c.eps_final, c.eps_decay) for t in range(n)], np.float32)
    ref_b = np.array([beta_by_frame(t, c.beta, c.beta_horizon) for t in range(n)], np.float32)
    ulp_e = np.abs(_np(eps).view(np.int32).astype(np.int64) - ref_e.view(np.int32))
    ulp_b = np.abs(_np(beta).view(np.int32).astype(np.int64) - ref_b.view(np.int32))
    print(f"schedules: eps max ulp {ulp_e.max()} ({int((ulp_e > 0).sum())} differ), beta max ulp {ulp_b.max()}")
    assert ulp_e.max() <= 1 and ulp_b.max() <= 1
    assert ref_b[1000] == 1.0 and float(beta[2000]) == 1.0 and float(eps[0]) == 1.0
    assert int(eng.t.item()) == n


# ------------------------------------------------------------------ fused frame vs the launches it fuses
@functools.lru_cache(maxsize=None)
def _twin_run(cuda, env_id, E, C):
    """FRAMES frames of the fused kernel (learning off) beside a twin VectorActorShard driven with
    vec_act + vec_classic_step + frame_hist_step on the same weights, keys and ring size, and a twin
    replay that takes ``write_priorities(slot, None)`` at the same max_prio.  Everything is recorded
    on the device per frame and read back once."""
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.vector import VectorActorShard

    eng = _engine(cuda, env_id, E, C, eps_decay=60.0)   # greedy draws dominate the later frames
    eng.learning = False
    rp = eng.replay
    rp2 = HBMReplay(C, E, 1, eng.cfg.alpha, cuda, frame_bytes=4 * eng.obs_dim)
    assert rp2.frame_capacity == rp.frame_capacity
    sh = VectorActorShard(rp2, E, env_id, n_step=1, seed=eng.env_seed, max_episode_steps=eng.limit)
    sh.set_policy(eng.model)
    hist2 = sh.st["hist"]
    assert torch.equal(hist2, eng.hist) and torch.equal(sh.env_state, eng.env_state)
    assert torch.equal(sh.ring, eng.ring)
    A, obs = eng.A, eng.obs_dim
    z = lambda *s, dt=torch.float32: torch.zeros(FRAMES, *s, dtype=dt, device=cuda)  # noqa: E731
    keys_f = {"q": (E, A), "reward": (E,), "done": (E,), "env_state": (E, 16), "row": (E, obs), "ep_log": (E, 3)}
    keys_i = {"actions": (E,), "hist": (E, 4), "new_frame": (E,)}
    rec = {w: {**{k: z(*s) for k, s in keys_f.items()}, **{k: z(*s, dt=torch.int32) for k, s in keys_i.items()}}
           for w in ("fused", "twin")}
    ins = {"slot": z(E, dt=torch.int32), "acted": z(E, dt=torch.int32), "s3": z(E, dt=torch.int32),
           "s23": z(E, dt=torch.int32), "a": z(E, dt=torch.int32), "r": z(E), "d": z(E), "leaf": z(E), "leaf_min": z(E),
           "leaf2": z(E), "mp_before": z(1), "mp_after": z(1), "root": z(1, dt=torch.float64),
           "leaves": z(1, dt=torch.float64), "root_min": z(1), "leaves_min": z(1), "eps": z(1)}
    for t in range(FRAMES):
        if t % 40 == 0:   # a running max that moves, as the PER would move it
            rp.max_prio.fill_(1.0 + 0.37 * (t // 40))
        ins["mp_before"][t].copy_(rp.max_prio)
        ins["acted"][t].copy_(eng.hist[:, 3])
        eng.frame()
        ins["mp_after"][t].copy_(rp.max_prio)
        ins["eps"][t].copy_(eng.eps)
        # the twin: this frame's device epsilon, then the three launches
        sh.eps.copy_(eng.eps.expand(E))
        sh.act()
        sh.env_step()
        sh.hip.frame_hist_step(hist2.data_ptr(), sh.new_frame.data_ptr(), sh.done.data_ptr(), E,
                               sh.step_counter.data_ptr(), torch.cuda.current_stream().cuda_stream)
        for w, src, h in (("fused", eng, eng.hist), ("twin", sh, hist2)):
            r = rec[w]
            for k in ("q", "reward", "done", "env_state", "actions", "new_frame"):
                r[k][t].copy_(getattr(src, k))
            r["hist"][t].copy_(h)
            r["row"][t].copy_(src.ring[src.new_frame.long()])
            r["ep_log"][t].copy_(src.ep_log[:, :3])
        sl = eng.slot.long()
        ins["slot"][t].copy_(eng.slot)
        ins["s3"][t].copy_(rp.s_ids[sl, 3])
        ins["s23"][t].copy_(rp.s2_ids[sl, 3])
        ins["a"][t].copy_(rp.action[sl])
        ins["r"][t].copy_(rp.reward[sl])
        ins["d"][t].copy_(rp.done[sl])
        ins["leaf"][t].copy_(rp.leaf_sum[sl])
        ins["leaf_min"][t].copy_(rp.leaf_min[sl])
        rp2.max_prio.copy_(rp.max_prio)
        rp2.write_priorities(eng.slot, None, dedup=False)
        ins["leaf2"][t].copy_(rp2.leaf_sum[sl])
        if (t + 1) % 25 == 0:
            ins["root"][t].copy_(rp.node_sum[-1])
            ins["leaves"][t].copy_(rp.leaf_sum.double().sum())
            ins["root_min"][t].copy_(rp.node_min[-1])
            ins["leaves_min"][t].copy_(rp.leaf_min.min())
    torch.cuda.synchronize()
    return eng, sh, rp2, rec, ins


@pytest.mark.parametrize("C", [96, 4160])
@pytest.mark.parametrize("E", [1, 3, 8])
@pytest.mark.parametrize("env_id", ENVS)
def test_fused_frame_equals_act_step_hist(cuda, env_id, E, C):
    """Q, actions, reward, done, env_state, the new ring rows, hist and the episode log of the
    fused kernel are bit-equal to vec_act + vec_classic_step + frame_hist_step, frame by frame."""
    eng, sh, _, rec, ins = _twin_run(cuda, env_id, E, C)
    for k in rec["fused"]:
        assert torch.equal(rec["fused"][k], rec["twin"][k]), k
    assert torch.equal(eng.ring, sh.ring) and torch.equal(eng.hist, sh.st["hist"])
    assert int(eng.t.item()) == int(sh.step_counter.item()) == FRAMES
    # the run was not trivial: both draws, every action, episode ends with their resets
    a, d = _np(rec["fused"]["actions"]), _np(rec["fused"]["done"])
    greedy = _np(rec["fused"]["q"]).argmax(-1)
    assert set(np.unique(a)) == set(range(eng.A))
    assert (a != greedy).any() and (a == greedy)[150:].mean() > 0.5
    assert d.sum() >= 3 and float(eng.ep_log[:, 2].sum()) == d.sum()
    assert float(eng.ep_log[:, 3].sum()) == pytest.approx(float((_np(rec["fused"]["ep_log"])[..., 0] * d).sum()))
    eps = _np(ins["eps"])[:, 0]
    assert eps[0] == 1.0 and eps[-1] < 0.02 and (np.diff(eps) < 0).all()
    F = eng.replay.frame_capacity
    want = (np.arange(1, FRAMES + 1)[:, None] * E + np.arange(E)[None]) % F
    assert (_np(rec["fused"]["new_frame"]) == want).all()   # the ring-row convention
    assert C > 96 or FRAMES * E > 2 * F                       # ... through several wraps of the ring


@pytest.mark.parametrize("C", [96, 4160])
@pytest.mark.parametrize("E", [1, 3, 8])
@pytest.mark.parametrize("env_id", ENVS)
def test_insert_semantics(cuda, env_id, E, C):
    eng, _, rp2, rec, ins = _twin_run(cuda, env_id, E, C)
    rp, f = eng.replay, rec["fused"]
    # slots advance as (filled + e) mod C, through the wrap
    want = (np.arange(FRAMES)[:, None] * E + np.arange(E)[None]) % C
    assert (_np(ins["slot"]) == want).all()
    assert int(rp.filled.item()) == FRAMES * E and (C > 96 or FRAMES * E > 3 * C)
    # the row: (ring row acted on, action, reward, new ring row, done) of that frame
    assert torch.equal(ins["s3"], ins["acted"]) and torch.equal(ins["s23"], f["new_frame"])
    assert torch.equal(ins["s23"], f["hist"][:, :, 3])
    assert torch.equal(ins["a"], f["actions"]) and torch.equal(ins["r"], f["reward"])
    assert torch.equal(ins["d"], f["done"])
    # the row acted on is the previous frame's new row
    assert torch.equal(ins["acted"][1:], f["new_frame"][:-1])
    # leaves: what write_priorities(idx, None) writes at the same max_prio; max_prio untouched
    assert torch.equal(ins["leaf"], ins["leaf2"]) and torch.equal(ins["leaf"], ins["leaf_min"])
    assert torch.equal(ins["mp_before"], ins["mp_after"])
    mp = _np(ins["mp_before"])[:, 0]
    assert len(np.unique(mp)) == 8
    np.testing.assert_allclose(_np(ins["leaf"]), np.broadcast_to((mp.astype(np.float64) ** 0.6)[:, None], (FRAMES, E)),
                               rtol=1e-6)
    assert torch.equal(rp.leaf_sum, rp2.leaf_sum) and torch.equal(rp.leaf_min, rp2.leaf_min)
    # the tree: root sum = fp64 sum of the leaves, root min = the leaves' min, every 25th frame
    at = np.arange(24, FRAMES, 25)
    root, leaves = _np(ins["root"])[at, 0], _np(ins["leaves"])[at, 0]
    assert (leaves > 0).all() and (np.abs(root - leaves) <= 1e-12 * leaves).all()
    assert (_np(ins["root_min"])[at] == _np(ins["leaves_min"])[at]).all()
    # and every level at the end, against the twin's tree (per_write_leaves' own walk)
    assert len(rp.node_sum) == (3 if C == 4160 else 2)
    for lv in range(len(rp.node_sum)):
        assert torch.equal(rp.node_sum[lv], rp2.node_sum[lv]) and torch.equal(rp.node_min[lv], rp2.node_min[lv]), lv


# ------------------------------------------------------------------ the running max follows the PER
@pytest.mark.parametrize("E", [1, 3])
def test_max_priority_follows_the_per(cuda, E):
    """Full frames on C = 96, driven launch by launch: after each SGD step max_prio is the larger of
    its previous value and max(prio_out); the next frame's leaves use it; the sequence equals
    PrioritizedReplayBuffer._max_priority fed the same priorities."""
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.replay.buffers import PrioritizedReplayBuffer

    C, B = 96, 8
    eng = _engine(cuda, "CartPole-v0", E, C, batch_size=B, lr=1e-2)
    rp = eng.replay
    rp2 = HBMReplay(C, E, 1, eng.cfg.alpha, cuda, frame_bytes=4 * eng.obs_dim)
    host = PrioritizedReplayBuffer(C, alpha=eng.cfg.alpha)
    dummy = np.zeros(eng.obs_dim, np.float32)
    # the max starts below any TD error (|r| = 1, Q ~ 0) and Q is pushed away from its target twice, so the
    # first SGD step and the steps after frames 40 and 80 must each raise it
    rp.max_prio.fill_(0.05)
    host._max_priority = float(np.float32(0.05))
    raised = 0
    for t in range(120):
        if t in (40, 80):
            with torch.no_grad():
                eng.model.value[2].bias.add_(2.0 * t / 40)
        mp0 = rp.max_prio.clone()
        eng.act_insert()
        for _ in range(E):
            host.add(dummy, 0, 0.0, dummy, 0.0)
        rp2.max_prio.copy_(mp0)
        rp2.write_priorities(eng.slot, None, dedup=False)
        sl = eng.slot.long()
        assert torch.equal(rp.leaf_sum[sl], rp2.leaf_sum[sl]) and torch.equal(rp.max_prio, mp0), t
        assert float(mp0) == float(np.float32(host._max_priority)), t
        if t >= eng.first_learning_frame:
            eng.sgd_step()
            pmax = eng.prio.max()
            assert torch.equal(rp.max_prio[0], torch.maximum(mp0[0], pmax)), t
            raised += int(float(pmax) > float(mp0))
            host.update_priorities(eng.idx.tolist(), _np(eng.prio).astype(np.float64))
            assert float(rp.max_prio) == float(np.float32(host._max_priority)), t
        else:
            assert int(eng.step_counter.item()) == 0
    assert raised >= 3 and float(rp.max_prio) > 1.0   # the max did move
    assert float(rp.node_sum[-1][0]) == pytest.approx(float(rp.leaf_sum.double().sum()), rel=1e-12)


# ------------------------------------------------------------------ one SGD step vs fp64 PyTorch
def _double(model):
    m = DuelingDQN.from_shapes(model.input_shape, model.num_actions).double()
    m.load_state_dict({k: v.detach().double().cpu() for k, v in model.state_dict().items()})
    return m


@pytest.mark.parametrize("env_id", ENVS)
def test_sgd_step_matches_fp64(cuda, env_id):
    """Three SGD steps at n = 1 on the engine's own idx / w.  Q, loss, priorities and gradient
    against fp64 PyTorch within test_gpu_vector_engine.py's bounds.  The parameter update: the
    device's, torch's fp32 Adam's and an fp64 Adam's on the device's gradients (early StepLR each);
    the device update's max error against fp64 may be at most twice the fp32 torch update's
    (update = parameters after - before the step; the measured pair is in profiles/dqn_engine.md)."""
    eng = _engine(cuda, env_id, 8, 4160, lr_step_size=2, lr_gamma=0.5)
    cfg, rp = eng.cfg, eng.replay
    eng.learning = False
    for _ in range(40):
        eng.frame()
    with torch.no_grad():   # a target that differs from the online net
        eng.tflat.add_(torch.randn_like(eng.tflat) * 0.05)
    p32 = [p.detach().clone().requires_grad_(True) for p in eng.model.parameters()]
    p64 = [p.detach().double().cpu().requires_grad_(True) for p in eng.model.parameters()]
    adam = dict(lr=cfg.lr, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_eps, weight_decay=0.0)
    o32, o64 = torch.optim.Adam(p32, **adam), torch.optim.Adam(p64, **adam)
    s32, s64 = (torch.optim.lr_scheduler.StepLR(o, step_size=cfg.lr_step_size, gamma=cfg.lr_gamma) for o in (o32, o64))
    worst = {"q": 0.0, "loss": 0.0, "prio": 0.0, "grad": 0.0, "upd_dev": 0.0, "upd_t32": 0.0}
    knee = [0, 0]
    # Q(s, a) is moved to about 0.4, 2.0 and 1.0 from the 1-step target (|r| = 1, Q ~ 0), step by step,
    # so the TD errors fall on both sides of the Huber knee
    sign = 1.0 if env_id.startswith("CartPole") else -1.0
    for it in range(3):
        shift = sign * (0.6, 2.4, -1.0)[it]
        with torch.no_grad():
            eng.model.value[2].bias.add_(shift)
            p32[-1].add_(shift)
            p64[-1].add_(shift)
        assert float(eng.beta.item()) == pytest.approx(beta_by_frame(39, cfg.beta, cfg.beta_horizon), rel=2e-7)
        eng.sample()
        eng.forward_backward()
        torch.cuda.synchronize()
        idx = eng.idx.long()
        assert int(idx.min()) >= 0 and int(idx.max()) < len(rp)
        s = eng.ring[rp.s_ids[idx, 3].long()].double().cpu()
        s2 = eng.ring[rp.s2_ids[idx, 3].long()].double().cpu()
        batch = (s, rp.action[idx].long().cpu(), rp.reward[idx].double().cpu(), s2, rp.done[idx].double().cpu(),
                 eng.w.double().cpu())
        on, tg = _double(eng.model), _double(eng.target)
        loss64, prio64 = compute_loss_device(on, tg, batch, 1, cfg.gamma)
        loss64.backward()
        with torch.no_grad():
            worst["q"] = max(worst["q"], _rel(_np(eng.q_s), on(s).numpy()), _rel(_np(eng.q_s2), on(s2).numpy()),
                             _rel(_np(eng.qt_s2), tg(s2).numpy()))
        grad = eng.flat_grad.clone()
        knee[0] += int((eng.delta < 1).sum())
        knee[1] += int((eng.delta >= 1).sum())
        for (name, o, k), q64 in zip(eng.segments, on.parameters()):
            g64 = q64.grad.reshape(-1).numpy()
            gk = _np(grad[o:o + k]).astype(np.float64)
            assert np.linalg.norm(g64) > 0, name
            worst["grad"] = max(worst["grad"], float(np.linalg.norm(gk - g64) / np.linalg.norm(g64)))
        # the three optimizers on the device's gradient
        off = 0
        for a, b in zip(p32, p64):
            a.grad = grad[off:off + a.numel()].view_as(a).clone()
            b.grad = a.grad.double().cpu()
            off += a.numel()
        before = [torch.cat([p.detach().reshape(-1).double().cpu() for p in ps])
                  for ps in (p32, p64, list(eng.model.parameters()))]
        for sched, opt in ((s32, o32), (s64, o64)):
            step_scheduler_early(sched)
            opt.step()
        eng.optimize()
        eng.write_priorities()
        torch.cuda.synchronize()
        after = [torch.cat([p.detach().reshape(-1).double().cpu() for p in ps])
                 for ps in (p32, p64, list(eng.model.parameters()))]
        d32, d64, ddev = (a - b for a, b in zip(after, before))
        assert float(d64.abs().max()) > 1e-4   # (an update of about lr)
        worst["upd_t32"] = max(worst["upd_t32"], float((d32 - d64).abs().max()))
        worst["upd_dev"] = max(worst["upd_dev"], float((ddev - d64).abs().max()))
        l64 = float(loss64.detach())
        worst["loss"] = max(worst["loss"], abs(float(eng.loss.item()) - l64) / abs(l64))
        worst["prio"] = max(worst["prio"], _rel(_np(eng.prio), prio64.numpy()))
        assert float(eng.norms[3].item()) == pytest.approx(o32.param_groups[0]["lr"], rel=1e-6)
        assert float(eng.norms[2].item()) == 1.0   # no clipping
        assert int(eng.step_counter.item()) == it + 1
    print(f"sgd {env_id}: |td| < 1 / >= 1: {knee}; " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert knee[0] > 0 and knee[1] > 0
    assert o32.param_groups[0]["lr"] == pytest.approx(cfg.lr * 0.5)   # the StepLR boundary was crossed, early
    assert worst["q"] <= Q_BOUND and worst["loss"] <= LOSS_BOUND and worst["prio"] <= PRIO_BOUND
    assert worst["grad"] <= GRAD_BOUND
    assert worst["upd_dev"] <= 2 * worst["upd_t32"]


# ------------------------------------------------------------------ cadence
def test_cadence(cuda):
    """target_update_interval = 7, 16 eager frames, learning from frame 2 (E = 3, batch 8)."""
    eng = _engine(cuda, "CartPole-v0", 3, 96, batch_size=8, target_update_interval=7, lr_step_size=5, lr_gamma=0.5)
    assert eng.first_learning_frame == 2
    init = eng.flat.clone()
    with torch.no_grad():
        eng.tflat.add_(1.0)   # (so that the sync of frame 0 shows)
    dummy = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=eng.cfg.lr)
    sched = torch.optim.lr_scheduler.StepLR(dummy, step_size=5, gamma=0.5)
    lrs = []
    for t in range(16):
        eng.frame()
        torch.cuda.synchronize()
        same = torch.equal(eng.flat, eng.tflat)
        if t < 2:   # no SGD launch has written anything
            assert torch.equal(eng.flat, init) and int(eng.step_counter.item()) == 0
            assert not eng.opt_m.any() and not eng.opt_v.any() and not eng.flat_grad.any() and not eng.norms.any()
            assert same   # synced at frame 0, nothing has moved since
        else:
            step_scheduler_early(sched)
            lrs.append(dummy.param_groups[0]["lr"])
            assert float(eng.norms[3]) == pytest.approx(lrs[-1], rel=1e-6), t
            assert int(eng.step_counter.item()) == t - 1 == eng.learn_steps
            assert same == (t in (7, 14)), t
        assert int(eng.t.item()) == t + 1 == eng.frames
        assert int(eng.replay.filled.item()) == 3 * (t + 1)
    assert not torch.equal(eng.flat, init)
    assert lrs[0] == lrs[3] == eng.cfg.lr and lrs[4] == pytest.approx(eng.cfg.lr * 0.5) and len(set(lrs)) == 3
    st = eng.stats()
    assert st["frames"] == 16 and st["learn_steps"] == 14 and all(v == v for v in st.values())


# ------------------------------------------------------------------ graph = eager, determinism
@pytest.fixture(scope="module")
def runs(cuda):
    """Engines ``a`` and ``a2`` eager, ``b`` through the hipGraph; one seed, 200 frames each, C = 96."""
    out = {}
    for name in ("a", "a2", "b"):
        eng = _engine(cuda, "CartPole-v0", 3, 96, biased=False, batch_size=16, target_update_interval=50, seed=3)
        if name == "b":
            eng.capture(warmup_iters=3)
        while eng.frames < 200:
            eng.frame()
        torch.cuda.synchronize()
        out[name] = eng
    return out


def test_graph_equals_eager_and_same_seed_is_bit_identical(runs):
    a = runs["a"]
    assert runs["b"]._graph is not None and a._graph is None and runs["a2"]._graph is None
    assert a.learn_steps == 200 - a.first_learning_frame == int(a.step_counter.item())
    for other in (runs["a2"], runs["b"]):
        ra, rb = a.replay, other.replay
        assert torch.equal(a.flat, other.flat) and torch.equal(a.tflat, other.tflat)
        for k in ("s_ids", "s2_ids", "action", "reward", "done", "leaf_sum", "leaf_min", "max_prio", "filled",
                  "frames"):
            assert torch.equal(getattr(ra, k), getattr(rb, k)), k
        for x, y in zip(ra.node_sum + ra.node_min, rb.node_sum + rb.node_min):
            assert torch.equal(x, y)
        assert torch.equal(a.ep_log, other.ep_log) and torch.equal(a.env_state, other.env_state)
        assert torch.equal(a.opt_m, other.opt_m) and torch.equal(a.opt_v, other.opt_v)
        assert int(other.t.item()) == 200 and other.learn_steps == a.learn_steps
    assert float(a.ep_log[:, 2].sum()) > 0 and float(a.replay.max_prio) > 1.0
    assert float(a.replay.node_sum[-1][0]) == pytest.approx(float(a.replay.leaf_sum.double().sum()), rel=1e-12)


def test_save_and_evaluate(runs, tmp_path):
    eng = runs["b"]
    filled = int(eng.replay.filled.item())
    path = eng.save(str(tmp_path / "model199.pth"))
    m = DuelingDQN.from_shapes((4,), 2)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert list(sd) == list(m.state_dict())
    m.load_state_dict(sd)
    assert torch.equal(torch.cat([p.reshape(-1) for p in m.parameters()]), eng.flat.cpu())
    ret = eng.rollout_evaluate(5)
    assert len(ret) == 5 and all(1 <= r <= 200 and r == int(r) for r in ret)
    assert eng.evaluate(5, seed=1) == eng.rollout_evaluate(5, seed=1)
    assert int(eng.replay.filled.item()) == filled   # evaluation writes nothing to the replay


# ------------------------------------------------------------------ CLI
def test_cli_gpu_engine(cuda, tmp_path, capsys):
    from apex_amd.trainers import dqn as trainer
    from apex_amd.utils.checkpoint import load_model

    recs = trainer.main(["--engine", "gpu", "--max-step", "300", "--save-dir", str(tmp_path), "--log-interval", "100",
                         "--eval-interval", "150", "--seed", "1"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["model0.pth", "model299.pth"]
    init = load_model(DuelingDQN.from_shapes((4,), 2), str(tmp_path / "model0.pth"))
    last = load_model(DuelingDQN.from_shapes((4,), 2), str(tmp_path / "model299.pth"))
    flat = lambda m: torch.cat([p.reshape(-1) for p in m.parameters()])  # noqa: E731
    assert torch.isfinite(flat(last)).all() and not torch.equal(flat(init), flat(last))
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert lines == recs and [r["frame"] for r in lines] == [99, 149, 199, 299]
    for r in lines:
        assert set(r) >= {"loss", "lr", "eps", "frames_per_s", "episodes", "mean_return"}
        assert np.isfinite(r["loss"]) and r["lr"] == pytest.approx(1e-3) and r["frames_per_s"] > 0
        assert r["eps"] == pytest.approx(epsilon_by_frame(r["frame"]), rel=1e-6)
    assert lines[-1]["episodes"] > lines[0]["episodes"] > 0 and 8 <= lines[-1]["mean_return"] <= 200
    assert 1 <= lines[1]["eval_return"] <= 200 and "eval_return" in lines[3] and "eval_return" not in lines[0]
