"""The step-tail references (tests/step_tail_ref.py) checked on the host: they agree with torch
in fp64, a correct fp32 evaluation of every formula (numpy float32, two summation orders /
algebraic forms) stays under every conditioned bound at every shape of the GPU suite, the same
evaluation with one mistake in it is rejected, and Adam's bound needs its bias-correction term
against the ``1 - powf(beta, t)`` form.  Each maximum is printed as ``TAIL-CPU ...``
(profiles/step_tail_fp64.md records them)."""
import warnings

import numpy as np
import pytest
import torch

from . import goldens
from . import step_tail_ref as R

F = np.float32


# ---------------------------------------------------------------- fp32 evaluations
def eval32_loss(c, order=0, bug=None):
    """The loss / heads-backward formulas in numpy float32.  order 0: colsum and the batch sums in
    ascending order, W_adv2 as (sum_b 1[a_b = k] g_b h_b) - (sum_b g_b h_b) / A; order 1:
    descending, W_adv2 as sum_b dadv_b h_b with dadv = g (e_a - 1 / A)."""
    B, A = c["B"], c["A"]
    ix = c["idx"].astype(np.int64)
    a, r, d = c["act"][ix].astype(np.int64), c["rew"][ix], c["done"][ix]
    rows = np.arange(B)
    if bug == "tie_high":
        astar = A - 1 - np.argmax(c["q2"][:, ::-1], axis=1)
    else:
        astar = np.argmax(c["q2"], axis=1)
    if bug == "ignore_done":
        d = np.zeros_like(d)
    qt, qa, w, gn = c["q2t"][rows, astar], c["q"][rows, a], c["w"], F(c["gamma_n"])
    y = r + gn * qt * (F(1) - d)
    delta = np.abs(y - qa)
    lw = w * np.where(delta < 1, F(0.5) * delta * delta, delta - F(0.5))
    diff = qa - y
    g = w / F(B) * (diff if bug == "unclamped" else np.clip(diff, F(-1), F(1)))
    wa, wv, h = c["w_adv2"], c["w_val2"], c["h"]
    colsum = np.zeros(128, F)
    for k in (range(A) if order == 0 else reversed(range(A))):
        colsum = colsum + wa[k]
    if bug == "colsum_last_twice":
        colsum = colsum + wa[A - 1]
    ga = g if bug == "drop_inv_A" else g / F(A)
    dz = np.concatenate([g[:, None] * wa[a] - ga[:, None] * colsum[None, :], g[:, None] * wv[None, :]], 1)
    dz = np.where(h > 0, dz, F(0))
    acc = np.zeros((A, 128), F)
    S, gsum, gact, dsum = np.zeros(256, F), F(0), np.zeros(A, F), np.zeros(256, F)
    for b in (range(B) if order == 0 else reversed(range(B))):
        if order == 0:
            acc[a[b]] = acc[a[b]] + g[b] * h[b, :128]
        else:
            dadv = np.full(A, -(g[b] / F(A)), F)
            dadv[a[b]] = g[b] - g[b] / F(A)
            acc = acc + dadv[:, None] * h[b, None, :128]
        S = S + g[b] * h[b]
        gsum = gsum + g[b]
        gact[a[b]] = gact[a[b]] + g[b]
        dsum = dsum + dz[b]
    out = {"delta": delta, "lw": lw, "dz": dz, "w_val2": S[128:], "b_val2": np.array([gsum], F),
           "b_adv2": gact - gsum / F(A), "b_adv1": dsum[:128], "b_val1": dsum[128:],
           "w_adv2": acc - (S[:128] / F(A))[None, :] if order == 0 else acc}
    if order == 0:
        out["loss"] = np.array(np.sum(lw, dtype=F) / F(B))
    else:
        t = F(0)
        for v in lw:
            t = t + v
        out["loss"] = np.array(t / F(B))
    out["prio"] = (F(0.9) * delta.max() + F(0.1) * delta) + F(1e-6)
    assert all(v.dtype == F for v in out.values()), {k: v.dtype for k, v in out.items()}
    return out


def _clip_lr32(g, hp, step, bug=None):
    l2, _, _, _ = R.clip_and_lr(g, hp, step)
    l2f, gs = F(l2), F(hp["grad_scale"])
    coef = F(hp["max_norm"]) / (l2f + F(1e-6)) if hp["max_norm"] > 0 else F(1)
    clip = min(coef, F(1)) * gs
    hp2 = dict(hp, lr_step_offset=0) if bug == "ignore_offset" else hp
    gamma, size = hp["lr_gamma"], hp["lr_step_size"]
    if gamma == 1.0 or size <= 0:
        lr = F(hp["lr"])
    else:
        lr = F(hp["lr"]) * F(gamma ** ((step + hp2["lr_step_offset"]) // size))
    return F(clip), F(lr)


def eval32_rms(p, g, s1, s2, hp, step, order=0, bug=None):
    clip, lr = _clip_lr32(g, hp, step, bug)
    a, eps = F(hp["alpha"]), F(hp["eps"])
    oma = F(1) - a
    gi = g * clip
    gm = g if bug == "clip_after_moments" else gi
    n1 = s1 * a + oma * gm * gm if order == 0 else a * s1 + oma * (gm * gm)
    if hp["centered"]:
        n2 = s2 + oma * (gm - s2) if order == 0 else a * s2 + oma * gm
        var = np.maximum(n1 - n2 * n2, F(0))
    else:
        n2, var = s2, n1
    avg = np.sqrt(var + eps) if bug == "eps_in_sqrt" else np.sqrt(var) + eps
    pn = p - lr * (gi / avg) if order == 0 else p - (lr * gi) / avg
    assert pn.dtype == n1.dtype == n2.dtype == F
    return {"p": pn, "s1": n1, "s2": n2}


def eval32_adam(p, g, m, v, hp, step, order=0, bug=None, form="powf"):
    """form 'powf': bc = 1 - beta^t with a correctly rounded fp32 power; 'expm1':
    bc = -expm1f(t log1pf(beta - 1))."""
    clip, lr = _clip_lr32(g, hp, step, bug)
    b1, b2, eps, wd = F(hp["beta1"]), F(hp["beta2"]), F(hp["eps"]), F(hp["weight_decay"])
    t = step if bug == "t_is_step" else step + 1
    if form == "powf":
        bc1, bc2 = F(1) - F(float(b1) ** t), F(1) - F(float(b2) ** t)
    else:
        bc1, bc2 = -np.expm1(F(t) * np.log1p(b1 - F(1))), -np.expm1(F(t) * np.log1p(b2 - F(1)))
    gi = g if bug == "clip_after_moments" else g * clip
    if wd != 0:
        gi = gi + wd * p
    if bug == "clip_after_moments":
        lr = lr * clip
    with np.errstate(divide="ignore", invalid="ignore"):
        if order == 0:
            nm = m + (F(1) - b1) * (gi - m)
            nv = v * b2 + (F(1) - b2) * gi * gi
            pn = p - (lr / bc1) * (nm / (np.sqrt(nv) * (F(1) / np.sqrt(bc2)) + eps))
        else:
            nm = b1 * m + (F(1) - b1) * gi
            nv = b2 * v + (F(1) - b2) * (gi * gi)
            pn = p - (lr / bc1) * nm / (np.sqrt(nv) / np.sqrt(bc2) + eps)
    assert pn.dtype == nm.dtype == nv.dtype == F
    return {"p": pn, "s1": nm, "s2": nv}


def _loss_ratios(c, got, G=None):
    r = R.loss_heads_ref(c, G)
    return {k: R.ratio(got[k], r["ref"][k], r["scale"][k]) for k in r["ref"]}


def _opt_ratios(ref, got):
    return {k: R.ratio(got[k], ref["ref"][k], ref["scale"][k]) for k in ("p", "s1", "s2")}


# ---------------------------------------------------------------- 1. the references agree with torch
def _torch_steps(kind, hp, n_steps, seed):
    """(p, g, s1, s2) fp64 before and torch's fp64 parameter after each of n_steps steps."""
    rs = np.random.RandomState(seed)
    p0 = rs.randn(300)
    p = torch.from_numpy(p0.copy()).requires_grad_(True)
    if kind == "rms":
        opt = torch.optim.RMSprop([p], lr=hp["lr"], alpha=hp["alpha"], eps=hp["eps"], centered=hp["centered"])
    else:
        opt = torch.optim.Adam([p], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"],
                               weight_decay=hp["weight_decay"])
    sched = None
    if hp["lr_step_size"] > 0:
        sched = torch.optim.lr_scheduler.StepLR(opt, hp["lr_step_size"], hp["lr_gamma"])
    out = []
    for step in range(n_steps):
        g = rs.randn(300) * (20 if step % 2 else 0.01)
        p.grad = torch.from_numpy(g * hp["grad_scale"])
        if hp["max_norm"] > 0:
            torch.nn.utils.clip_grad_norm_([p], hp["max_norm"])
        if sched is not None and hp["lr_step_offset"]:
            with warnings.catch_warnings():  # the scheduler before the optimizer, on purpose: offset 1
                warnings.simplefilter("ignore", UserWarning)
                sched.step()
        opt.step()
        if sched is not None and not hp["lr_step_offset"]:
            sched.step()
        out.append((g, p.detach().numpy().copy()))
    return p0, out


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("centered", [False, True])
def test_rmsprop_reference_matches_torch_fp64(centered, offset):
    hp = R.rms_hp(6.25e-5, 0.95, 1.5e-7, max_norm=40.0, lr_gamma=0.5, lr_step_size=3, lr_step_offset=offset,
                  centered=centered, grad_scale=0.25)
    p, steps = _torch_steps("rms", hp, 8, 11)
    s1, s2 = np.zeros_like(p), np.zeros_like(p)
    clipped = set()
    for step, (g, want) in enumerate(steps):
        r = R.rmsprop_ref(p, g, s1, s2, hp, step)
        clipped.add(r["coef"] < 1)
        p, s1, s2 = r["ref"]["p"], r["ref"]["s1"], r["ref"]["s2"]
        np.testing.assert_allclose(p, want, rtol=1e-12, atol=0)
    assert clipped == {True, False}


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_reference_matches_torch_fp64(wd):
    hp = R.adam_hp(1e-3, weight_decay=wd, max_norm=10.0, lr_gamma=0.5, lr_step_size=3, lr_step_offset=1)
    p, steps = _torch_steps("adam", hp, 8, 12)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for step, (g, want) in enumerate(steps):
        r = R.adam_ref(p, g, m, v, hp, step)
        p, m, v = r["ref"]["p"], r["ref"]["s1"], r["ref"]["s2"]
        np.testing.assert_allclose(p, want, rtol=1e-12, atol=0)


def test_loss_reference_matches_golden():
    """delta -> loss and priorities of the reference on the Q-values of the recorded loss case
    (tests/golden/models_loss.npz: the reference implementation's compute_loss in fp64)."""
    from .test_models_host import _loss_case

    gold = goldens.load("models_loss")
    env, model, tgt, batch = _loss_case()
    model.load_state_dict(goldens.get_state(gold, "model"))
    tgt.load_state_dict(goldens.get_state(gold, "target"))
    s, a, r, s2, d, w = batch
    with torch.no_grad():
        q, q2, q2t = model(s).numpy(), model(s2).numpy(), tgt(s2).numpy()
    B, A = q.shape
    rs = np.random.RandomState(0)
    c = {"B": B, "A": A, "gamma_n": 0.99 ** 3, "q": q, "q2": q2, "q2t": q2t, "act": a.numpy(), "rew": r.numpy(),
         "done": d.numpy(), "idx": np.arange(B), "w": w.numpy(), "z": rs.randn(B, 256) + 3,
         "w_adv2": rs.randn(A, 128), "w_val2": rs.randn(128)}
    ref = R.loss_heads_ref(c)["ref"]
    np.testing.assert_allclose(ref["loss"], gold["loss"], rtol=1e-12)
    np.testing.assert_allclose(ref["prio"], gold["prios"], rtol=1e-12)


def test_crafted_rows_are_what_they_claim():
    for B, A in R.LOSS_SHAPES:
        if B < 8:
            continue
        for use_idx in (True, False):
            c = R.make_loss_case(B, A, use_idx=use_idx)
            r = R.loss_heads_ref(c)
            ix = c["idx"]
            d, a = c["done"][ix], r["a"]
            y_minus_q = -r["g"] * B / c["w"]  # clamp(y - Q(s, a))
            assert d[0] == 1 and d[3] == 1
            assert r["ref"]["delta"][1] > 1 and r["ref"]["delta"][2] > 1 and np.isclose(y_minus_q[1], 1) and np.isclose(y_minus_q[2], -1)
            assert r["ref"]["delta"][3] == 0 and not r["ref"]["dz"][3].any()
            assert a[4] == 0 and a[5] == A - 1
            tied = np.flatnonzero(c["q2"][6] == c["q2"][6].max())
            assert len(tied) == 2 and r["astar"][6] == tied[0] and c["q2t"][6, tied[0]] != c["q2t"][6, tied[1]]
            assert not c["h"][7].any() and not r["ref"]["dz"][7].any()
            assert (c["z"] != 0).all()
            assert use_idx == (len(np.unique(ix)) < B)


# ---------------------------------------------------------------- 2. a correct fp32 evaluation fits
@pytest.mark.parametrize("B,A", R.LOSS_SHAPES)
def test_fp32_loss_evaluation_fits(B, A):
    for use_idx in (True, False):
        c = R.make_loss_case(B, A, use_idx=use_idx)
        for order in (0, 1):
            rat = _loss_ratios(c, eval32_loss(c, order))
            print(f"TAIL-CPU B={B} A={A} idx={int(use_idx)} order={order} "
                  + " ".join(f"{k} {v:.3f}" for k, v in rat.items()))
            assert max(rat.values()) < 1, rat


def _opt_cases():
    """(name, kind, hp, step, state, gscale): every setting of the GPU suite at one small size."""
    out = []
    for centered in (False, True):
        for state in ("zero", "random"):
            for gscale, max_norm, gs in ((1e-2, 0.0, 1.0), (1e-2, 40.0, 1.0), (20.0, 40.0, 1.0), (20.0, 40.0, 0.25)):
                hp = R.rms_hp(6.25e-5, 0.95, 1.5e-7, max_norm, centered=centered, grad_scale=gs)
                out.append((f"rms c{int(centered)} {state} g{gscale} mn{max_norm} gs{gs}", "rms", hp, 0, state, gscale))
    for offset in (0, 1):
        for step in (2, 3, 5, 6):
            hp = R.rms_hp(6.25e-5, 0.95, 1.5e-7, 40.0, 0.5, 3, offset, True)
            out.append((f"rms steplr off{offset} step{step}", "rms", hp, step, "random", 20.0))
    for wd in (0.0, 1e-2):
        for step in (0, 1, 2, 9, 999):
            for gscale, max_norm in ((1e-2, 0.0), (20.0, 10.0)):
                hp = R.adam_hp(1e-3, weight_decay=wd, max_norm=max_norm)
                out.append((f"adam wd{wd} step{step} g{gscale} mn{max_norm}", "adam", hp, step,
                            "zero" if step == 0 else "random", gscale))
    return out


def _run_opt(kind, hp, step, state, gscale, order=0, bug=None, form="powf", n=1000, seed=5, bias_term=True,
             pscale=1e-2):
    p, g, s1, s2 = R.make_opt_state(n, seed, state, gscale, pscale)
    if kind == "rms":
        return R.rmsprop_ref(p, g, s1, s2, hp, step), eval32_rms(p, g, s1, s2, hp, step, order, bug)
    return (R.adam_ref(p, g, s2, s1, hp, step, bias_term=bias_term),
            eval32_adam(p, g, s2, s1, hp, step, order, bug, form))


def test_fp32_optimizer_evaluation_fits():
    for name, kind, hp, step, state, gscale in _opt_cases():
        for order in (0, 1):
            for form in (("powf", "expm1") if kind == "adam" else ("powf",)):
                ref, got = _run_opt(kind, hp, step, state, gscale, order, form=form)
                rat = _opt_ratios(ref, got)
                upd = R.ratio(got["p"], ref["ref"]["p"], R.U * np.abs(ref["update"]))
                print(f"TAIL-CPU {name} order={order} form={form} p {rat['p']:.3f} s1 {rat['s1']:.3f} "
                      f"s2 {rat['s2']:.3f} (p error {upd:.1f} u|update|, c <= {float(np.max(ref['c'])):.0f})")
                assert max(rat.values()) < 1, (name, order, form, rat)


# ---------------------------------------------------------------- 3. wrong arithmetic is rejected
@pytest.mark.parametrize("bug", ["tie_high", "drop_inv_A", "colsum_last_twice", "ignore_done", "unclamped"])
def test_loss_mistakes_are_rejected(bug):
    for B, A in R.LOSS_SHAPES:
        if B < 8:  # the crafted rows carry the tie, done and |td| > 1; A = 1 has no 1 / A to drop
            continue
        for order in (0, 1):
            c = R.make_loss_case(B, A)
            assert max(_loss_ratios(c, eval32_loss(c, order, bug)).values()) > 1, (bug, B, A, order)
    if bug == "colsum_last_twice":  # at A = 1 the whole advantage gradient must cancel
        c = R.make_loss_case(1, 1)
        assert _loss_ratios(c, eval32_loss(c, 0, bug))["dz"] > 1


def _mistake_configs(bug, kind):
    """(hp, step, state, gradient scale) at which the mistake changes the arithmetic."""
    sl = dict(lr_gamma=0.5, lr_step_size=3, lr_step_offset=1)
    out = []
    for centered in ((False, True) if kind == "rms" else (False,)):
        mk = (lambda **kw: R.rms_hp(6.25e-5, 0.95, 1.5e-7, centered=centered, **kw)) if kind == "rms" else \
             (lambda **kw: R.adam_hp(1e-3, **kw))
        if bug == "clip_after_moments":  # a clip well below 1
            out += [(mk(max_norm=10.0), 0, st, 20.0) for st in ("zero", "random")]
        elif bug == "eps_in_sqrt":  # sqrt(s1') ~ 2e-5 against eps = 1.5e-7, sqrt(eps) = 4e-4
            out += [(mk(), 0, st, 1e-4) for st in ("zero", "random")]
        elif bug == "t_is_step":
            out += [(mk(), step, "random", 1e-2) for step in (1, 2, 9)]
        else:  # (step + 1) // 3 != step // 3
            out += [(mk(max_norm=10.0, **sl), step, "random", 20.0) for step in (2, 5)]
    return out


@pytest.mark.parametrize("bug,kind", [("clip_after_moments", "rms"), ("clip_after_moments", "adam"),
                                      ("eps_in_sqrt", "rms"), ("t_is_step", "adam"), ("ignore_offset", "rms"),
                                      ("ignore_offset", "adam")])
def test_optimizer_mistakes_are_rejected(bug, kind):
    for hp, step, state, gscale in _mistake_configs(bug, kind):
        for order in (0, 1):
            ref, good = _run_opt(kind, hp, step, state, gscale, order, pscale=1e-2)
            assert max(_opt_ratios(ref, good).values()) < 1
            _, bad = _run_opt(kind, hp, step, state, gscale, order, bug=bug, pscale=1e-2)
            assert max(_opt_ratios(ref, bad).values()) > 1, (bug, kind, hp, step, state, order)


# ---------------------------------------------------------------- 4. Adam's bias-correction term
def test_adam_bound_needs_its_bias_correction_term():
    """beta2 = 0.999, t = 2: 1 - powf(beta2, t) is off by ~110 u (499 times the rounding of the
    power; ~60 u of the update, through the square root), -expm1f(t log1pf(beta2 - 1)) is not.  Parameters at the scale of the update, so that
    u |p'| does not hide it.  Without the term the bound rejects the powf form and still holds
    the expm1 form; with it both fit."""
    hp = R.adam_hp(1e-3)
    worst = {}
    for form in ("powf", "expm1"):
        for term in (True, False):
            ref, got = _run_opt("adam", hp, 1, "zero", 1e-2, form=form, bias_term=term, pscale=1e-3)
            worst[form, term] = _opt_ratios(ref, got)["p"]
            if not term:
                err = R.ratio(got["p"], ref["ref"]["p"], R.U * np.abs(ref["update"]))
                print(f"TAIL-CPU adam t=2 form={form}: p error {err:.1f} u|update|, bound without the term "
                      f"{float(np.max(ref['c'])):.0f} u|update| + u|p|, ratio {worst[form, term]:.2f}")
    assert worst["powf", True] < 1 and worst["expm1", True] < 1
    assert worst["powf", False] > 1, worst
    assert worst["expm1", False] < 1, worst
