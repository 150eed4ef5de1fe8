"""GPU AQL.py engine (engine/aql_frame.py, aql_frame in ops/csrc/aql_frame_kernels.hip, the AQL.py
mode of aql_update): the fused acting frame against the launches it fuses, acting with the
train-mode online net, the per-frame epsilon stream, the device schedules, one SGD step against
fp64 PyTorch, the fused step sequence against the launch-by-launch one, the loop's cadences,
graph = eager, determinism, checkpoints, evaluation and the CLI.

Bit-equal means ``torch.equal``.  The fp64 bounds are test_gpu_aql_engine.py's
(``test_learner_step_matches_reference``: the same critic and learner kernels)."""
import copy
import functools
import json

import numpy as np
import pytest
import torch

from apex_amd.algo.schedules import cosine_lr

from . import aql_rollout_fixtures as fx
from .actor_oracle import uniform4
from .test_aql_frame_host import EPS_FRAMES, EPS_SEED, torch_cosine

pytestmark = pytest.mark.gpu

FRAMES = 300
# (env, candidate-set options): T = 16 and T = 13 (not a multiple of the 8 waves) on Pendulum, the
# discrete T = 5, the AQL engine's default T = 51 with 4 action dims, the reference's T = 200
SHAPES = {
    "pend16": ("Pendulum-v0", dict(propose_sample=7, uniform_sample=9)),
    "pend13": ("Pendulum-v0", dict(propose_sample=6, uniform_sample=7)),
    "cart5": ("CartPole-v0", dict(propose_sample=3)),
    "biped51": ("BipedalWalker-v3", dict(propose_sample=1, uniform_sample=50)),
    "pend200": ("Pendulum-v0", dict(propose_sample=100, uniform_sample=100)),
}
T_OF = {"pend16": 16, "pend13": 13, "cart5": 5, "biped51": 51, "pend200": 200}


def _np(t):
    return t.detach().cpu().numpy()


def _engine(cuda, shape, C=96, **kw):
    from apex_amd.engine.aql_frame import AQLFrameConfig, AQLFrameEngine

    env_id, cand = SHAPES[shape]
    if not env_id.startswith("CartPole"):
        kw.setdefault("max_episode_steps", 20)   # so that resets occur
    kw.setdefault("batch_size", 8)
    eng = AQLFrameEngine(AQLFrameConfig(env_id=env_id, capacity=C, **cand, **kw), cuda)
    assert eng.T == T_OF[shape]
    fx.set_params(eng.model)   # non-zero biases, sigma and epsilon
    eng.sync_target()          # (the target follows; both nets' effective weights are recomputed)
    return eng


# ------------------------------------------------------------------ fused frame vs the launches it fuses
REC_F = ("cand", "q", "eps", "env_act", "reward", "done", "obs_next", "row_st", "row_st2", "row_rew", "row_done",
         "row_amu", "leaf", "leaf_min", "ep_ret", "beta", "ep_log")
REC_I = ("act_idx", "slot", "row_act", "ep_len", "ep_count")


@functools.lru_cache(maxsize=None)
def _twin_run(cuda, shape, C):
    """FRAMES acting frames (learning off) of the fused kernel beside a twin engine with
    ``fused=False`` on the same weights and seeds.  Everything is recorded on the device per frame
    and read back once."""
    engs = {"fused": _engine(cuda, shape, C, trace_q=True), "twin": _engine(cuda, shape, C, fused=False)}
    rec = {w: {} for w in engs}
    tree = {k: torch.zeros(FRAMES, dtype=torch.float64, device=cuda) for k in ("root", "leaves", "root_min", "leaves_min")}
    mp = torch.zeros(FRAMES, 2, device=cuda)
    for w, eng in engs.items():
        eng.learning = False
        assert torch.equal(eng.learner.flat, engs["fused"].learner.flat)
        assert torch.equal(eng.obs_buf, engs["fused"].obs_buf)
    for t in range(FRAMES):
        for w, eng in engs.items():
            rp = eng.replay
            if t % 40 == 0:   # a running max that moves, as the PER would move it
                rp.max_prio.fill_(1.0 + 0.37 * (t // 40))
            if w == "fused":
                mp[t, 0:1].copy_(rp.max_prio)
            eng.frame()
            if w == "fused":
                mp[t, 1:2].copy_(rp.max_prio)
            sl = eng.slot.long()
            cur = {"cand": rp.a_mu[sl] if w == "fused" else eng.amu, "q": eng.qbuf, "eps": eng.eps,
                   "env_act": eng.env_act, "reward": eng.reward, "done": eng.done, "obs_next": eng.obs_buf,
                   "row_st": rp.st[sl], "row_st2": rp.st2[sl], "row_rew": rp.reward[sl], "row_done": rp.done[sl],
                   "row_amu": rp.a_mu[sl], "leaf": rp.leaf_sum[sl], "leaf_min": rp.leaf_min[sl], "ep_ret": eng.ep_ret,
                   "beta": eng.beta, "ep_log": eng.ep_log[:8], "act_idx": eng.act_idx, "slot": eng.slot,
                   "row_act": rp.action[sl], "ep_len": eng.ep_len, "ep_count": eng.ep_count}
            r = rec[w]
            for k, v in cur.items():
                if k not in r:
                    r[k] = torch.zeros(FRAMES, *v.shape, dtype=v.dtype, device=cuda)
                r[k][t].copy_(v)
        if (t + 1) % 25 == 0:
            rp = engs["fused"].replay
            tree["root"][t].copy_(rp.node_sum[-1][0])
            tree["leaves"][t].copy_(rp.leaf_sum.double().sum())
            tree["root_min"][t].copy_(rp.node_min[-1][0])
            tree["leaves_min"][t].copy_(rp.leaf_min.min())
    torch.cuda.synchronize()
    assert set(rec["fused"]) == set(REC_F) | set(REC_I)
    return engs, rec, tree, mp


TWIN_CASES = [(s, C) for s in ("pend16", "pend13", "cart5", "biped51") for C in (96, 4160)] + [("pend200", 96)]


@pytest.mark.parametrize("shape,C", TWIN_CASES)
def test_fused_frame_equals_the_launches_it_fuses(cuda, shape, C):
    """Per frame: the candidate set, the Q row, epsilon, the selected index, the action, reward,
    done, the next observation, the slot, the inserted row (all six tables) and the leaf sum / min
    of ``aql_frame`` are bit-equal to aql_propose -> aql_candidate_q -> aql_frame_eps + aql_select
    -> aql_env_step -> per_write_leaves; every 25 frames the root is the sum / min of the leaves."""
    engs, rec, tree, mp = _twin_run(cuda, shape, C)
    f, tw = rec["fused"], rec["twin"]
    for k in f:
        assert torch.equal(f[k], tw[k]), k
    a, b = engs["fused"], engs["twin"]
    ra, rb = a.replay, b.replay
    for k in ("st", "st2", "action", "reward", "done", "a_mu", "leaf_sum", "leaf_min", "filled", "max_prio"):
        assert torch.equal(getattr(ra, k), getattr(rb, k)), k
    assert len(ra.node_sum) == (3 if C == 4160 else 2)
    for lv in range(len(ra.node_sum)):
        assert torch.equal(ra.node_sum[lv], rb.node_sum[lv]) and torch.equal(ra.node_min[lv], rb.node_min[lv]), lv
    for k in ("t", "obs_buf", "phys", "ep_len", "ep_ret", "ep_count", "ep_log"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert int(a.t.item()) == int(ra.filled.item()) == FRAMES
    # the insert: slot = filled mod C through the wrap; the row is this frame's transition
    assert (_np(f["slot"])[:, 0] == np.arange(FRAMES) % C).all() and (C > 96 or FRAMES > 3 * C)
    assert torch.equal(f["row_amu"], f["cand"]) and torch.equal(f["row_act"], f["act_idx"])
    assert torch.equal(f["row_rew"], f["reward"]) and torch.equal(f["row_done"], f["done"])
    idx = f["act_idx"][:, 0].long()
    assert torch.equal(f["cand"][torch.arange(FRAMES, device=cuda), 0, idx], f["env_act"][:, 0])
    d = _np(f["done"])[:, 0] > 0
    nxt, st, st2 = _np(f["obs_next"])[:, 0], _np(f["row_st"])[:, 0], _np(f["row_st2"])[:, 0]
    assert (nxt[~d] == st2[~d]).all() and (st[1:] == nxt[:-1]).all()
    assert d.sum() >= 3 and int(a.ep_count.item()) == d.sum()   # episodes ended (TimeLimit stored as done)
    # the leaf: max_prio^alpha at the running max, which the insert leaves alone
    assert torch.equal(mp[:, 0], mp[:, 1]) and len(np.unique(_np(mp)[:, 0])) == 8
    assert torch.equal(f["leaf"], f["leaf_min"])
    np.testing.assert_allclose(_np(f["leaf"])[:, 0], _np(mp)[:, 0].astype(np.float64) ** 0.6, rtol=1e-6)
    at = np.arange(24, FRAMES, 25)
    root, leaves = _np(tree["root"])[at], _np(tree["leaves"])[at]
    assert (leaves > 0).all() and (np.abs(root - leaves) <= 1e-12 * leaves).all()
    assert (_np(tree["root_min"])[at] == _np(tree["leaves_min"])[at]).all()
    # the run was not trivial: both epsilons, greedy and random picks
    eps, q = _np(f["eps"])[:, 0], _np(f["q"])[:, 0]
    assert set(np.unique(eps)) == {np.float32(0.5), np.float32(0.05)}
    greedy = _np(idx) == q.argmax(-1)
    assert greedy.any() and (~greedy).any()


@pytest.mark.parametrize("shape", ["pend16", "cart5", "biped51"])
def test_acting_is_the_train_mode_online_net(cuda, shape):
    """The frame's Q row against an fp64 ``AQL`` copy in train mode (noise applied) on the same
    observation and candidates: within 1e-4 of the row's max |Q|; against the eval-mode copy
    (the means) it differs by more than that."""
    engs, rec, _, _ = _twin_run(cuda, shape, 96)
    eng, f = engs["fused"], rec["fused"]
    # the discrete critic casts its candidate input with .float(): CartPole runs the reference in fp32
    dt = torch.float64 if eng.cont else torch.float32
    ref = copy.deepcopy(eng.model).to(dt)
    s = f["row_st"][:, 0].to(dt)
    am = f["cand"][:, 0].to(dt)
    if not eng.cont:
        am = am.reshape(FRAMES, -1)
    q = f["q"][:, 0].double()
    with torch.no_grad():
        ref.q.train()
        q_train = ref.q.candidate_q(s, am).double()
        ref.q.eval()
        q_eval = ref.q.candidate_q(s, am).double()
    scale = q_train.abs().amax(1) + 1e-6
    err_t = ((q - q_train).abs().amax(1) / scale).max().item()
    err_e = ((q - q_eval).abs().amax(1) / scale).min().item()
    print(f"{shape}: |Q - train fp64| / max|Q| = {err_t:.3g}; min over frames |Q - eval| / max|Q| = {err_e:.3g}")
    assert err_t <= 1e-4
    assert err_e > 1e-4


# ------------------------------------------------------------------ epsilon
def test_epsilon_stream(cuda):
    """4000 frames: every epsilon is exactly 0.5 or 0.05, the 0.05 share is inside +-4 sigma of
    Binomial(4000, 0.1), and the sequence equals the host model of the documented Philox stream."""
    from apex_amd.engine.aql_frame import host_epsilons

    eng = _engine(cuda, "pend16", seed=EPS_SEED)
    eng.learning = False
    eps = torch.zeros(EPS_FRAMES, device=cuda)
    for t in range(EPS_FRAMES):
        eng.frame()
        eps[t:t + 1].copy_(eng.eps)
    torch.cuda.synchronize()
    e = _np(eps)
    assert ((e == np.float32(0.5)) | (e == np.float32(0.05))).all()
    share = float((e == np.float32(0.05)).mean())
    print(f"epsilon: share of 0.05 = {share:.4f}")
    assert 0.08 <= share <= 0.12
    want = np.asarray(host_epsilons(EPS_SEED, EPS_FRAMES, uniform4=uniform4), dtype=np.float32)
    assert (e == want).all()


# ------------------------------------------------------------------ schedules
def test_device_beta_matches_host_within_one_ulp(cuda):
    """beta(t) of frames 0..2000 with max_step = 1000 against the host formula rounded to fp32."""
    n = 2001
    eng = _engine(cuda, "pend16", max_step=1000)
    eng.learning = False
    beta = torch.zeros(n, device=cuda)
    for t in range(n):
        eng.frame()
        beta[t:t + 1].copy_(eng.beta)
    torch.cuda.synchronize()
    c = eng.cfg
    ref = np.array([min(1.0, c.beta_start + t * (1.0 - c.beta_start) / c.max_step) for t in range(n)], np.float32)
    ulp = np.abs(_np(beta).view(np.int32).astype(np.int64) - ref.view(np.int32))
    print(f"beta: max ulp {ulp.max()} ({int((ulp > 0).sum())} differ)")
    assert ulp.max() <= 1
    assert float(beta[0]) == np.float32(0.4) and ref[1000] == 1.0 and float(beta[1000]) == 1.0
    assert float(beta[2000]) == 1.0 and int(eng.t.item()) == n


@pytest.mark.parametrize("T_max", [10, 1000])
def test_device_cosine_lr_matches_the_torch_scheduler(cuda, T_max):
    """``lr_used`` at SGD step k (set through the step counter) against CosineAnnealingLR stepped
    k times: within 2e-7 relative (half an ulp of the fp32 rounding + one ulp for the device's
    cos)."""
    eng = _engine(cuda, "pend16", max_step=T_max)
    eng.learning = False
    for _ in range(12):
        eng.frame()
    c = eng.cfg
    for k in (0, 1, T_max // 2, T_max - 1, T_max):
        eng.set_learn_steps(k)
        eng.sgd_step()
        torch.cuda.synchronize()
        got = float(eng.lr_used.item())
        ref = torch_cosine(k, c.lr, T_max, c.eta_min())
        print(f"T_max {T_max} k {k}: lr_used {got:.9g} scheduler {ref:.9g} rel {abs(got - ref) / ref:.3g}")
        assert abs(got - ref) <= 2e-7 * ref
        assert float(eng.learner.norms_p[3].item()) == got   # both Adams
        assert int(eng.learner.step_ctr.item()) == k + 1


# ------------------------------------------------------------------ one SGD step vs fp64
def _grads(model, names):
    return {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
            for n, p in model.named_parameters() if n in names}


def _adam_at(params, lr, k):
    """A fresh Adam whose step count is k (zero moments, as the engine's are)."""
    opt = torch.optim.Adam(params, lr)
    for g in opt.param_groups:
        for p in g["params"]:
            opt.state[p] = {"step": torch.tensor(float(k)), "exp_avg": torch.zeros_like(p),
                            "exp_avg_sq": torch.zeros_like(p)}
    return opt


@pytest.mark.parametrize("shape", ["biped51", "cart5", "pend16"])
def test_sgd_step_matches_fp64_in_aql_py_mode(cuda, shape):
    from apex_amd.algo.losses import compute_loss_AQL

    T_max = 1000
    eng = _engine(cuda, shape, max_step=T_max)
    L, cfg = eng.learner, eng.cfg
    eng.learning = False
    for _ in range(64):
        eng.frame()
    k = T_max // 2
    eng.set_learn_steps(k)
    lr_k = cosine_lr(k, cfg.lr, T_max, cfg.eta_min())
    assert abs(lr_k - cfg.lr / 2) < 1e-3 * cfg.lr
    dt = torch.float64 if eng.cont else torch.float32
    mr, tr = copy.deepcopy(eng.model).to(dt), copy.deepcopy(eng.target).to(dt)
    for m in (mr, tr):
        m.proposal.action_var = m.proposal.action_var.to(device=eng.device, dtype=dt)
        m.q.train()
    p_before, eps0, teps0, tflat0 = L.flat.clone(), L.eps.clone(), L.teps.clone(), L.tflat.clone()
    assert torch.equal(L.tflat, L.flat)
    eng.sgd_step()
    torch.cuda.synchronize()
    r = eng.replay
    idx = L.idx.long()
    s, s2 = r.st[idx].to(dt), r.st2[idx].to(dt)
    a, rew, d, am, w = r.action[idx].long(), r.reward[idx].to(dt), r.done[idx].to(dt), r.a_mu[idx].to(dt), L.w.to(dt)
    if not eng.cont:
        am = am.reshape(am.shape[0], -1)
    B = s.shape[0]
    assert B == 8 and float(eng.beta.item()) > cfg.beta_start

    # --- the reference step (AQL.py compute_td_loss): proposal first, then the critic, both at lr_k
    q_values = mr(s, am)
    with torch.no_grad():
        q2_ref = mr.q.candidate_q(s2, am)
        qt2_ref = tr.q.candidate_q(s2, am)
    scale = q_values.detach().abs().max().item() + 1e-6
    assert (L.q_s.double() - q_values.detach()).abs().max().item() <= 1e-4 * scale
    assert (L.q_s2.double() - q2_ref).abs().max().item() <= 1e-4 * scale
    assert (L.qt_s2.double() - qt2_ref).abs().max().item() <= 1e-4 * scale
    dist = mr.proposal.evaluate(mr.q.embedding_feature(s))
    best = am[torch.arange(B, device=am.device), q_values.max(1)[1]].reshape(B, -1)
    loss_p = torch.mean(-dist.log_prob(best) - cfg.ent_lam * dist.entropy())
    opt_p = _adam_at(list(mr.proposal.parameters()), lr_k, k)
    opt_p.zero_grad()
    loss_p.backward()
    g_ref = _grads(mr, {n for n, _ in mr.named_parameters() if n.startswith("proposal.")})
    torch.nn.utils.clip_grad_norm_(mr.proposal.parameters(), cfg.max_norm)
    opt_p.step()
    loss_q, prios = compute_loss_AQL(mr, tr, (s, a, rew, s2, d, am, w), n_steps=1, gamma=cfg.gamma)
    opt_q = _adam_at(list(mr.q.parameters()), lr_k, k)
    opt_q.zero_grad()
    loss_q.backward()
    g_ref.update(_grads(mr, {n for n, _ in mr.named_parameters() if n.startswith("q.")}))
    torch.nn.utils.clip_grad_norm_(mr.q.parameters(), cfg.max_norm)
    opt_q.step()

    # --- losses, priorities, gradients (pre-clip): test_learner_step_matches_reference's bounds
    assert abs(L.loss_q.item() - loss_q.item()) <= 1e-4 * max(1.0, abs(loss_q.item()))
    assert abs(L.loss_p.item() - loss_p.item()) <= 1e-4 * max(1.0, abs(loss_p.item()))
    pr = torch.as_tensor(prios, dtype=torch.float64)
    assert (L.prio.double().cpu() - pr).abs().max().item() <= 1e-4 * pr.abs().max().item()
    offs = eng.model._flat_offsets
    for name, p in eng.model.named_parameters():
        n, off = p.numel(), offs[name]
        g = L.grad[off:off + n].double().reshape(p.shape)
        ref = g_ref[name]
        err = (g - ref).norm().item()
        assert err <= 1e-4 * ref.norm().item() + 1e-9, (name, err, ref.norm().item())
    # --- parameters after both clipped Adam steps at cosine_lr(k)
    sel = torch.cat([torch.arange(offs[n], offs[n] + p.numel()) for n, p in eng.model.named_parameters()])
    sel = sel.to(L.flat.device)
    p_ref = torch.cat([p.detach().reshape(-1) for p in mr.parameters()])
    diff = (L.flat[sel].double() - p_ref).abs()
    moved = (p_ref - p_before[sel].double()).abs()
    print(f"{shape}: lr_k {lr_k:.4g} max|dp - ref| / lr_k {diff.max().item() / lr_k:.3g} "
          f"share > 1e-3 lr_k {(diff > 1e-3 * lr_k).float().mean().item():.3g} moved / lr_k {moved.max().item() / lr_k:.3g}")
    assert diff.max().item() <= 2.01 * lr_k
    assert (diff > 1e-3 * lr_k).float().mean().item() < 1e-3, "more than 0.1% of updates differ"
    assert moved.max().item() > 0.5 * lr_k
    assert abs(float(eng.lr_used.item()) - lr_k) <= 2e-7 * lr_k
    # --- AQL.py: the noise stays, no proposal copy, the target is untouched
    assert torch.equal(L.eps, eps0) and torch.equal(L.teps, teps0)
    assert torch.equal(L.tflat, tflat0)
    assert not torch.equal(L.tflat[L.P_q:], L.flat[L.P_q:])
    # --- the online effective weights: what aql_post(regen = 0) yields from the updated parameters
    eff_on, eff_tg = L.eff_on.clone(), L.eff_tg.clone()
    L.eff_on.zero_()
    L.refresh()
    torch.cuda.synchronize()
    assert torch.equal(L.eff_on, eff_on) and torch.equal(L.eff_tg, eff_tg)
    a1 = eng.model.q.advantage1
    want = torch.addcmul(a1.weight_mu.double(), a1.weight_sigma.double(), a1.weight_epsilon.double()).reshape(-1)
    assert (eff_on[:want.numel()].double() - want).abs().max().item() <= 1e-6
    assert L.step_ctr.item() == k + 1


# ------------------------------------------------------------------ fused sequence vs the launch-by-launch one
@pytest.mark.parametrize("shape", ["pend13", "cart5", "biped51"])
def test_fused_sequence_equals_reference_sequence(cuda, shape):
    """48 frames (40 learning) with a constant schedule (``lr_eta_min == lr``: a host-rounded lr
    cannot differ): parameters, Adam moments, the tree, max_prio, the replay and the env are
    bit-identical between ``fused=True`` and ``fused=False``."""
    out = []
    for fused in (True, False):
        eng = _engine(cuda, shape, lr=3e-4, lr_eta_min=3e-4, target_update_interval=17, fused=fused)
        for _ in range(8 + 40):
            eng.frame()
        torch.cuda.synchronize()
        L, r = eng.learner, eng.replay
        assert int(L.step_ctr.item()) == 40 == eng.learn_steps
        assert float(eng.lr_used.item()) == np.float32(3e-4)
        out.append({"flat": L.flat, "m": L.m, "v": L.v, "tflat": L.tflat, "eps": L.eps, "teps": L.teps,
                    "eff_on": L.eff_on, "eff_tg": L.eff_tg, "idx": L.idx, "w": L.w, "prio": L.prio,
                    "loss_q": L.loss_q, "loss_p": L.loss_p, "leaf_sum": r.leaf_sum, "leaf_min": r.leaf_min,
                    "root": r.node_sum[-1], "root_min": r.node_min[-1], "max_prio": r.max_prio, "st": r.st,
                    "a_mu": r.a_mu, "action": r.action, "reward": r.reward, "obs": eng.obs_buf, "t": eng.t,
                    "beta": eng.beta, "ep_log": eng.ep_log})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), (k, (out[0][k].double() - out[1][k].double()).abs().max().item())
    assert float(out[0]["max_prio"].item()) != 1.0 and bool((out[0]["m"] != 0).any())


# ------------------------------------------------------------------ cadence
@pytest.mark.parametrize("C", [96, 32])
def test_cadence(cuda, C):
    """Batch 8, target_update_interval 7, 40 frames: no SGD step before frame 8, one per frame
    from it on; target syncs exactly on frames 0, 7, 14, ... and after one the target equals the
    online net, noise included; ``len(replay) == min(40, C)``."""
    eng = _engine(cuda, "pend16", C, target_update_interval=7)
    L = eng.learner
    assert eng.first_learning_frame == 8
    L.teps.add_(1.0)   # (a target noise that differs until the first sync)
    for t in range(40):
        eng.frame()
        torch.cuda.synchronize()
        assert int(L.step_ctr.item()) == max(0, t + 1 - 8), t
        assert len(eng.replay) == min(t + 1, C)
        synced = torch.equal(L.tflat, L.flat) and torch.equal(L.teps, L.eps) and torch.equal(L.eff_tg, L.eff_on)
        if t % 7 == 0:
            assert synced, t
        elif t > 8:
            assert not torch.equal(L.tflat, L.flat), t
    assert eng.target_syncs == [0, 7, 14, 21, 28, 35]
    assert int(L.step_ctr.item()) == 40 - 8 == eng.learn_steps
    assert len(eng.replay) == min(40, C) and int(eng.t.item()) == 40 == eng.frames
    assert np.isfinite(eng.stats()["loss_q"])


# ------------------------------------------------------------------ graph = eager, determinism
_STATE = ("flat", "m", "v", "tflat", "eps", "teps", "eff_on", "step_ctr", "idx")
_REPLAY = ("st", "st2", "action", "reward", "done", "a_mu", "leaf_sum", "leaf_min", "max_prio", "filled")


@functools.lru_cache(maxsize=None)
def _run120(cuda, mode):
    eng = _engine(cuda, "pend13", 96, target_update_interval=50, seed=5)
    if mode == "eager":
        for _ in range(120):
            eng.frame()
    else:
        eng.run(70)
        assert eng._g_act is not None and eng._g_full is not None
        eng.run(50)
    torch.cuda.synchronize()
    return eng


def test_graph_equals_eager_and_same_seed_is_bit_identical(cuda):
    a, b, c = _run120(cuda, "graph"), _run120(cuda, "eager"), _run120(cuda, "graph2")
    for other in (b, c):
        for k in _STATE:
            assert torch.equal(getattr(a.learner, k), getattr(other.learner, k)), k
        for k in _REPLAY:
            assert torch.equal(getattr(a.replay, k), getattr(other.replay, k)), k
        assert torch.equal(a.replay.node_sum[-1], other.replay.node_sum[-1])
        for k in ("t", "obs_buf", "ep_log", "ep_count", "beta"):
            assert torch.equal(getattr(a, k), getattr(other, k)), k
        assert a.target_syncs == other.target_syncs == [0, 50, 100]
    assert a.frames == 120 and a.learn_steps == 112 == int(a.learner.step_ctr.item())
    assert int(a.ep_count.item()) >= 5 and float(a.replay.max_prio) != 1.0
    assert a.launches_per_frame == 5


# ------------------------------------------------------------------ save, evaluate, CLI
def test_save_and_evaluate(cuda, tmp_path):
    from apex_amd import envs
    from apex_amd.models.aql import AQL
    from apex_amd.utils.checkpoint import load_model

    eng = _engine(cuda, "cart5")
    for _ in range(20):
        eng.frame()
    path = eng.save(19, str(tmp_path))
    assert path == str(tmp_path / "model19.pth") and (tmp_path / "model19.pth.train.pt").exists()
    fresh = AQL(envs.make("CartPole-v0"), device="cpu", **SHAPES["cart5"][1])
    load_model(fresh, path, strict=True)
    sd, ref = fresh.state_dict(), eng.model.state_dict()
    assert "q.advantage1.weight_epsilon" in sd and set(sd) == set(ref)
    for k in sd:
        assert torch.equal(sd[k], ref[k].cpu()), k
    st = torch.load(str(tmp_path / "model19.pth.train.pt"), weights_only=True)
    assert st["counters"] == {"frame": 19, "learner_steps": 12}
    assert torch.equal(st["extra"]["adam_m"], eng.learner.m.cpu())
    filled = int(eng.replay.filled.item())
    a = eng.evaluate(3, seed=1234, max_episode_steps=60)
    b = eng.rollout_evaluate(3, seed=1234, max_episode_steps=60)
    assert a == b and all(1.0 <= x <= 60.0 for x in a)
    assert eng.rollout_evaluate(3, seed=1234, max_episode_steps=60) == b
    assert int(eng.replay.filled.item()) == filled   # evaluation writes nothing to the replay


def test_cli_gpu_engine(cuda, tmp_path, capsys):
    from apex_amd import envs
    from apex_amd.models.aql import AQL
    from apex_amd.trainers import aql as trainer
    from apex_amd.utils.checkpoint import load_model

    recs = trainer.main(["--engine", "gpu", "--env", "Pendulum-v0", "--max-step", "200", "--save-dir", str(tmp_path),
                         "--log-interval", "100", "--eval-interval", "150", "--seed", "1"])
    names = sorted(p.name for p in tmp_path.iterdir() if p.name.endswith(".pth"))
    assert names == ["model0.pth", "model199.pth"]
    env = envs.make("Pendulum-v0")
    init = load_model(AQL(env, propose_sample=100, uniform_sample=100, device="cpu"), str(tmp_path / "model0.pth"))
    last = load_model(AQL(env, propose_sample=100, uniform_sample=100, device="cpu"), str(tmp_path / "model199.pth"))
    flat = lambda m: torch.cat([p.reshape(-1) for p in m.parameters()])  # noqa: E731
    assert torch.isfinite(flat(last)).all() and not torch.equal(flat(init), flat(last))
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert lines == recs and [r["frame"] for r in lines] == [99, 149, 199]
    assert lines[0]["loss_q"] is not None and 0.4 < lines[-1]["beta"] < 1.0 and lines[-1]["lr"] <= 1e-4
    assert "eval_return" in lines[1] and "eval_return" not in lines[0]
