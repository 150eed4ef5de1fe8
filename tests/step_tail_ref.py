"""fp64 references and conditioned error scales for the last launches of a learner step:
dqn_heads_bwd (loss + dueling-heads backward + head-gradient partials), the heads job of
grad_finalize, and rmsprop_step / adam_step / adam_step2.  Host only (numpy + CPU torch): the
GPU suite (test_gpu_step_tail_fp64.py) and the host suite (test_step_tail_ref_host.py) share it.

Every check is ``|got - ref| / scale < 1`` per element, with ``u = 2^-24`` the fp32 unit roundoff
and the scale counted from the kernels' code:

Loss + heads.  ``g_b = w_b/B clamp(Q(s,a) - y)`` is a difference, so its fp32 error is a few ulp
of the operands, not of ``|g_b|``.  With ``S_b = |Q(s,a)| + |r| + gamma^n |Q_t (1 - d)|``:

  delta     4 u S_b: the product gamma^n Q_t, the sum r + ., the difference y - Q(s,a) round at
            most (|gamma^n Q_t| + |y| + |delta|) u <= 3 u S_b; one spare, for an evaluation that
            rounds (1 - d) gamma^n Q_t in another order.
  lw        4 u S_b w_b max(delta, 1): d huber / d delta = min(delta, 1) <= max(delta, 1), the
            roundings of 0.5 delta^2 | delta - 0.5 and of w * . are below u S_b max(delta, 1).
  g_b       e_b = 4 s_b + n |g_b| in units of u, s_b = (w_b / B) S_b (the error of the
            difference carried through w / B) and n the number of further fp32 roundings on the
            longest chain behind the output:
  dz        n = A + 4: colsum_j is A - 1 sequential adds in action order, then w / B, g / A,
            the two products and the subtraction.  Scale u e_b (|W[a][j]| + sum_k |W[k][j]| / A)
            for j < 128, u e_b |W_val2[j - 128]| for j >= 128, 0 (exact zero) where h = 0.
  heads     n = 13 + (ceil(G / 4) + 2): w / B and the product g h (2), the chain of 8 rows
            inside a workgroup (8), S / A and the subtraction of it (2), one spare for the
            fused multiply-adds the compiler may or may not form (1); ceil(G / 4) + 2 for the
            finalize (a chain of ceil(G / 4) slices and the 4-way combine) when the finalized
            gradient is checked, 0 for the fp64 sum of the partials.  Scales:
            W_adv2[k][j] u sum_b e_b h_bj (1[a_b = k] + 1 / A), W_val2[j] u sum_b e_b h_b(128+j),
            b_adv2[k] u sum_b e_b (1[a_b = k] + 1 / A), b_val2 u sum_b e_b.
  FC1 bias  b_adv1 / b_val1 are column sums of dz: n = (A + 4) + 8 (+ finalize), scale the sum
            over the batch of dz's scale.
  loss      mean of lw's scale + 13 u mean |lw| (the 1024-wide tree reduction: <= 12 adds on a
            chain, and the division by B).
  priority  0.9 max_b(delta scale) + 0.1 (delta scale)_b + 5 u |prio| (two fp32 constants, two
            products, two sums; prio_mix is not contracted).

Optimizers, per element, in units of u (divide counted at 2.5 ulp = 5 u and sqrt at 3 ulp = 6 u:
the limits the compiler may lower fp32 ``/`` and ``sqrtf`` to when they are not correctly
rounded; a correctly rounded build fits a fortiori):

  clip      c_clip = 8 when the clip is active (l2 to fp32 1, + 1e-6 1, max_norm / . 5,
            * grad_scale 1), else 0 (coef = 1, clip = grad_scale exactly).
  lr        c_lr = 4 under StepLR (powf + product; norms_out[3] is held to the same 4 u), else 0.
  g_i       relative c_g = c_clip + 1 (the product g clip).
  RMSprop   s1' = s1 a + oma g_i g_i: relative 2 c_g + 4 (three products and the sum; the
            kernel's fma saves one).  s2' = s2 + oma (g_i - s2) or a s2 + oma g_i: absolute
            u (oma (c_g + 1) |g_i| + |s2| + |s2'|).  avg = sqrt(var) + eps with var = s1' (half
            of s1's, + 6 + 1) or var = s1' - s2'^2 (centered: the error of s1' and
            2 |s2'| err(s2') <= (2 c_g + 6) u s1' -- |s2'| <= sqrt(s1'), oma g_i^2 <= s1',
            |s2| <= 0.5 sqrt(s1' / a) -- all times the condition s1' / (s1' - s2'^2), + 1 for
            the difference, halved, + 6 + 1).  update = lr g_i / avg: c_g + 5 (divide) + c_lr +
            that.  New parameter: u |p'| + c u |update|.
  Adam      error propagated in absolute terms through g_i (+ wd p), m' = m + (1 - b1)(g_i - m)
            or b1 m + (1 - b1) g_i, v' = b2 v + (1 - b2) g_i g_i (each product and sum one
            rounding), sqrt(v') (6), rbc2 = 1 / sqrt(bc2) (11 + half the
            relative error of bc2), the fma with eps (1), the divide (5), step_size = lr / bc1
            (c_lr + 5 + the relative error of bc1).  bc = 1 - beta^t has relative error
            u + beta^t / (1 - beta^t) e_pow: the bias-correction term
            [beta1^t / (1 - beta1^t) + beta2^t / (2 (1 - beta2^t))] e_pow, with e_pow = 4 u
            (powf at its documented 1 ulp = 2 u, doubled).  ``bias_term=False`` drops it for the
            form bc = -expm1f(t log1pf(beta - 1)), whose relative error is 6 u at every t:
            log1pf and expm1f at 1 ulp = 2 u each, the product 1, x e^x / (e^x - 1) <= 1 for
            x < 0 carries the argument's error through, 1 spare.

Hyperparameters are the fp32 values the parameter structs hold, widened (``f32``)."""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24
E_POW = 4 * U  # relative error allowed to powf(beta, t)
E_BC_EXPM1 = 6 * U  # relative error of -expm1f(t log1pf(beta - 1)): log1pf 2, the product 1, expm1f 2, 1 spare
HEAD_KEYS = ("w_adv2", "b_adv2", "w_val2", "b_val2", "b_adv1", "b_val1")
# (B, A) of the dqn_heads_bwd cases (the issue's table: what each reaches is in the GPU suite)
LOSS_SHAPES = ((1, 1), (8, 6), (9, 3), (37, 18), (120, 17), (121, 63), (128, 16))
OPT_SIZES = (1, 255, 256, 257, 262144, 262145)


def f32(x) -> float:
    """The fp32 value a parameter struct holds for ``x``, as a Python double."""
    return float(np.float32(x))


def ratio(got, ref, scale) -> float:
    """max |got - ref| / scale; an exact match passes where the scale is 0 (masked outputs)."""
    got, ref, scale = (np.asarray(t, dtype=np.float64) for t in (got, ref, scale))
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    err = np.abs(got - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    r = np.where(err == 0, 0.0, err / np.maximum(scale, 1e-300))
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------- loss + heads: inputs
def make_loss_case(B: int, A: int, seed: int = 0, use_idx: bool = True) -> dict:
    """fp32 inputs of one dqn_heads_bwd launch.  (a, r, d) live in a transition table of C rows
    read through ``idx`` (use_idx: C = 4 B slots with a repeat; else C = B, row b).  B >= 8: rows
    0..7 are crafted -- 0 done = 1; 1, 2 |td| > 1 of either sign; 3 y == Q(s, a) exactly;
    4 a = 0; 5 a = A - 1; 6 an argmax tie whose tied actions differ in Q_t; 7 h all zero."""
    rs = np.random.RandomState(1000 * B + A + 7919 * seed)
    f = np.float32
    C = 4 * B if use_idx else B
    q = (rs.randn(B, A) * 3).astype(f)
    q2 = rs.randn(B, A).astype(f)
    q2t = rs.randn(B, A).astype(f)
    act = rs.randint(0, A, C).astype(np.int32)
    rew = rs.randn(C).astype(f)
    done = (rs.rand(C) < 0.2).astype(f)
    w = (rs.rand(B) + 0.2).astype(f)
    z = rs.randn(B, 256).astype(f)
    z[z == 0] = f(0.5)
    wa = (rs.randn(A, 128) * 0.1).astype(f)
    wv = (rs.randn(128) * 0.1).astype(f)
    if use_idx:
        idx = rs.permutation(C)[:B].astype(np.int32)
        if B > 8:
            idx[B - 1] = idx[4]  # a repeated slot (the last row reads row 4's transition)
        elif B == 8:
            idx[4] = idx[0]  # rows 0 and 4 share a slot (done = 1 and a = 0)
    else:
        idx = np.arange(B, dtype=np.int32)
    gn = f(0.99 ** 3)
    if B >= 8:
        s = idx[:8]
        done[s[0]] = 1
        rew[s[1]], done[s[1]] = 6, 0
        rew[s[2]], done[s[2]] = -6, 0
        done[s[3]] = 1
        act[s[4]] = 0
        act[s[5]] = A - 1
        done[s[6]] = 0
        z[7] = -np.abs(z[7])
        for b in (1, 2):
            q[b, act[s[b]]] = 0.5
        q[3, act[s[3]]] = rew[s[3]]  # done = 1: y = r exactly in fp32 and in fp64
        i, j = A // 3, A - 1
        assert i < j
        q2[6, i] = q2[6, j] = np.abs(q2[6]).max() + 1
        q2t[6, j] = q2t[6, i] + 2
    return {"B": B, "A": A, "C": C, "gamma_n": gn, "q": q, "q2": q2, "q2t": q2t, "act": act, "rew": rew,
            "done": done, "idx": idx, "use_idx": use_idx, "w": w, "z": z, "h": np.maximum(z, 0).astype(f),
            "w_adv2": wa, "w_val2": wv}


# ---------------------------------------------------------------- loss + heads: fp64 reference
def loss_heads_ref(c: dict, G: int | None = None) -> dict:
    """fp64 autograd through the real formulas from the fp32 inputs widened: ``ref`` (delta, lw,
    loss, prio, dz and the six gradients), ``scale`` (per output, see the module docstring;
    ``scale_part``: the head gradients without the finalize's roundings).  G: partial count
    (default ceil(B / 8))."""
    from apex_amd.algo.losses import huber_weighted

    B, A = c["B"], c["A"]
    G = -(-B // 8) if G is None else G
    D = torch.float64
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
    ix = c["idx"].astype(np.int64)
    a_np, r, d = c["act"][ix].astype(np.int64), t(c["rew"][ix]), t(c["done"][ix])
    a = torch.from_numpy(a_np)
    gn, w = float(c["gamma_n"]), t(c["w"])
    q = t(c["q"]).requires_grad_(True)
    astar = torch.from_numpy(np.argmax(c["q2"], axis=1))  # first maximum
    qt = t(c["q2t"]).gather(1, astar[:, None])[:, 0]
    y = r + gn * qt * (1 - d)
    qa = q.gather(1, a[:, None])[:, 0]
    td = torch.abs(y - qa)
    loss = huber_weighted(td, w)
    loss.backward()
    dq = q.grad  # dL/dQ: w / B clamp(Q(s, a) - y, -1, 1) at the action taken
    # the dueling heads, every parameter a leaf; the FC1 biases enter through zero leaves
    z = t(c["z"]).requires_grad_(True)
    b1 = torch.zeros(256, dtype=D, requires_grad=True)
    wa, wv = t(c["w_adv2"]).requires_grad_(True), t(c["w_val2"]).view(1, 128).requires_grad_(True)
    ba, bv = torch.zeros(A, dtype=D, requires_grad=True), torch.zeros(1, dtype=D, requires_grad=True)
    h = torch.relu(z + b1)
    adv, val = h[:, :128] @ wa.t() + ba, h[:, 128:] @ wv.t() + bv
    (val + adv - adv.mean(1, keepdim=True)).backward(dq)
    delta = td.detach().numpy()
    hub = np.where(delta < 1, 0.5 * delta ** 2, delta - 0.5)
    ref = {"delta": delta, "lw": c["w"].astype(np.float64) * hub, "loss": np.array(float(loss.detach())),
           "prio": 0.9 * delta.max() + 0.1 * delta + 1e-6, "dz": z.grad.numpy(),
           "w_adv2": wa.grad.numpy(), "b_adv2": ba.grad.numpy(), "w_val2": wv.grad.numpy().reshape(128),
           "b_val2": bv.grad.numpy(), "b_adv1": b1.grad.numpy()[:128], "b_val1": b1.grad.numpy()[128:]}
    assert abs(float(ref["lw"].mean()) - float(ref["loss"])) <= 1e-14 * max(1.0, abs(float(ref["loss"])))
    # ---- scales
    g = dq.gather(1, a[:, None])[:, 0].numpy()
    S = np.abs(qa.detach().numpy()) + np.abs(r.numpy()) + gn * np.abs((qt * (1 - d)).numpy())
    sb = c["w"].astype(np.float64) / B * S
    hh = np.maximum(c["z"].astype(np.float64), 0)
    mask = hh > 0
    Wa, Wv = np.abs(c["w_adv2"].astype(np.float64)), np.abs(c["w_val2"].astype(np.float64))
    fac = np.concatenate([Wa[a_np] + Wa.sum(0)[None, :] / A, np.broadcast_to(Wv, (B, 128))], 1) * mask  # [B][256]
    onehot = np.zeros((B, A))
    onehot[np.arange(B), a_np] = 1
    sel = onehot + 1.0 / A  # |1[a_b = k]| + 1 / A
    e = lambda n: (4 * sb + n * np.abs(g)) * U  # noqa: E731
    sd = 4 * U * S
    scale = {"delta": sd, "lw": sd * c["w"].astype(np.float64) * np.maximum(delta, 1),
             "dz": e(A + 4)[:, None] * fac}
    scale["loss"] = np.array(scale["lw"].mean() + 13 * U * np.abs(ref["lw"]).mean())
    scale["prio"] = 0.9 * sd.max() + 0.1 * sd + 5 * U * np.abs(ref["prio"])
    for name, fin in (("scale", math.ceil(G / 4) + 2), ("scale_part", 0)):
        eh, eb = e(13 + fin), e(A + 4 + 8 + fin)
        cs = (eb[:, None] * fac).sum(0)
        out = {"w_adv2": np.einsum("b,bk,bj->kj", eh, sel, hh[:, :128]), "b_adv2": (eh[:, None] * sel).sum(0),
               "w_val2": (eh[:, None] * hh[:, 128:]).sum(0), "b_val2": np.array([eh.sum()]),
               "b_adv1": cs[:128], "b_val1": cs[128:]}
        if name == "scale":
            scale.update(out)
        else:
            scale_part = out
    return {"ref": ref, "scale": scale, "scale_part": scale_part, "a": a_np, "g": g, "astar": astar.numpy(), "G": G}


# ---------------------------------------------------------------- optimizers
def clip_and_lr(g, hp: dict, step: int):
    """(l2 * grad_scale, coefficient min(max_norm / (l2 + 1e-6), 1), clip = coefficient *
    grad_scale, StepLR rate) in fp64 from the fp32 gradient; hp holds widened fp32 values."""
    gs = hp.get("grad_scale", 1.0)
    l2 = math.sqrt(float((np.asarray(g, dtype=np.float64) ** 2).sum())) * gs
    coef = min(hp["max_norm"] / (l2 + f32(1e-6)), 1.0) if hp["max_norm"] > 0 else 1.0
    return l2, coef, coef * gs, step_lr(hp, step)


def step_lr(hp: dict, step: int) -> float:
    gamma, size = hp.get("lr_gamma", 1.0), hp.get("lr_step_size", 0)
    if gamma == 1.0 or size <= 0:
        return hp["lr"]
    return hp["lr"] * gamma ** ((step + hp.get("lr_step_offset", 0)) // size)


def rms_hp(lr, alpha=0.99, eps=1e-8, max_norm=0.0, lr_gamma=1.0, lr_step_size=0, lr_step_offset=0, centered=False,
           grad_scale=1.0) -> dict:
    return {"lr": f32(lr), "alpha": f32(alpha), "eps": f32(eps), "max_norm": f32(max_norm), "lr_gamma": f32(lr_gamma),
            "lr_step_size": int(lr_step_size), "lr_step_offset": int(lr_step_offset), "centered": bool(centered),
            "grad_scale": f32(grad_scale)}


def adam_hp(lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0, lr_gamma=1.0, lr_step_size=0,
            lr_step_offset=0, grad_scale=1.0) -> dict:
    return {"lr": f32(lr), "beta1": f32(beta1), "beta2": f32(beta2), "eps": f32(eps), "weight_decay": f32(weight_decay),
            "max_norm": f32(max_norm), "lr_gamma": f32(lr_gamma), "lr_step_size": int(lr_step_size),
            "lr_step_offset": int(lr_step_offset), "grad_scale": f32(grad_scale)}


def _c_clip_lr(hp: dict, coef: float):
    c_clip = 8.0 if coef < 1.0 else 0.0
    c_lr = 4.0 if (hp.get("lr_gamma", 1.0) != 1.0 and hp.get("lr_step_size", 0) > 0) else 0.0
    return c_clip, c_lr


def rmsprop_ref(p, g, s1, s2, hp: dict, step: int) -> dict:
    """One RMSprop step in fp64 from the fp32 state: ``ref`` (p, s1, s2), ``scale`` of each,
    the update, and (l2, coef, lr)."""
    p, g, s1, s2 = (np.asarray(t, dtype=np.float64) for t in (p, g, s1, s2))
    l2, coef, clip, lr = clip_and_lr(g, hp, step)
    a, eps = hp["alpha"], hp["eps"]
    oma = 1.0 - a
    gi = g * clip
    n1 = a * s1 + oma * gi * gi
    if hp["centered"]:
        n2 = s2 + oma * (gi - s2)
        var = n1 - n2 * n2
        assert (var > 0).all()
    else:
        n2, var = s2.copy(), n1
    upd = lr * gi / (np.sqrt(var) + eps)
    pn = p - upd
    c_clip, c_lr = _c_clip_lr(hp, coef)
    cg = c_clip + 1
    if hp["centered"]:
        cond = n1 / var
        c_avg = ((2 * cg + 4) + (2 * cg + 6)) * cond / 2 + 0.5 + 7
        sc2 = U * (oma * (cg + 1) * np.abs(gi) + np.abs(s2) + np.abs(n2))
    else:
        c_avg = (2 * cg + 4) / 2 + 7 + np.zeros_like(p)
        sc2 = np.zeros_like(p)  # untouched: bit for bit
    c = cg + 5 + c_lr + c_avg
    return {"ref": {"p": pn, "s1": n1, "s2": n2}, "update": upd, "c": c, "l2": l2, "coef": coef, "lr": lr,
            "scale": {"p": U * np.abs(pn) + c * U * np.abs(upd), "s1": (2 * cg + 4) * U * n1, "s2": sc2}}


def adam_ref(p, g, m, v, hp: dict, step: int, bias_term: bool = True) -> dict:
    """One Adam step (t = step + 1) in fp64 from the fp32 state, as rmsprop_ref."""
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    l2, coef, clip, lr = clip_and_lr(g, hp, step)
    b1, b2, eps, wd = hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"]
    t = step + 1
    gc = g * clip
    gi = gc + wd * p
    nm = m + (1 - b1) * (gi - m)
    nv = b2 * v + (1 - b2) * gi * gi
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    den = np.sqrt(nv) / math.sqrt(bc2) + eps
    upd = (lr / bc1) * nm / den
    pn = p - upd
    # ---- absolute error propagation (module docstring)
    c_clip, c_lr = _c_clip_lr(hp, coef)
    e_g = (c_clip + 1) * U * np.abs(gc) + (U * np.abs(gi) if wd != 0 else 0.0)
    e_m = (1 - b1) * (e_g + U * np.abs(gi - m)) + U * np.abs(m) + U * np.abs(nm)
    e_v = (1 - b2) * (2 * np.abs(gi) * e_g + 2 * U * gi * gi) + U * b2 * v + U * nv
    sv = np.sqrt(nv)
    e_sv = np.where(sv > 0, e_v / (2 * np.maximum(sv, 1e-300)), 0.0) + 6 * U * sv
    # relative error of bc1 and half that of bc2: 1 - powf(beta, t) | -expm1f(t log1pf(beta - 1))
    pw1 = U + b1 ** t / bc1 * E_POW if bias_term else E_BC_EXPM1
    pw2 = (U + b2 ** t / bc2 * E_POW) / 2 if bias_term else E_BC_EXPM1 / 2
    rbc2 = 1 / math.sqrt(bc2)
    e_den = e_sv * rbc2 + sv * rbc2 * (11 * U + pw2) + U * den
    rel = e_m / np.maximum(np.abs(nm), 1e-300) + e_den / den + 5 * U + (c_lr + 5) * U + pw1
    rel = np.where(nm == 0, 0.0, rel)
    return {"ref": {"p": pn, "s1": nm, "s2": nv}, "update": upd, "c": rel / U, "l2": l2, "coef": coef, "lr": lr,
            "bias_term": pw1 + pw2,
            "scale": {"p": U * np.abs(pn) + rel * np.abs(upd), "s1": e_m, "s2": e_v}}


def make_opt_state(n: int, seed: int, state: str, gscale: float, pscale: float = 1.0):
    """fp32 (p, g, s1, s2): ``state`` 'zero' or 'random' (s1 > 0, |s2| <= 0.5 sqrt(s1): a centered
    condition of at most 4/3); gradients at ``gscale``."""
    rs = np.random.RandomState(seed)
    f = np.float32
    p = (rs.randn(n) * pscale).astype(f)
    g = (rs.randn(n) * gscale).astype(f)
    if state == "zero":
        return p, g, np.zeros(n, f), np.zeros(n, f)
    s1 = ((rs.rand(n) + 0.1) * gscale ** 2).astype(f)
    s2 = ((rs.rand(n) - 0.5) * np.sqrt(s1.astype(np.float64))).astype(f)
    assert (np.abs(s2.astype(np.float64)) <= 0.5 * np.sqrt(s1.astype(np.float64)) * (1 + 1e-6)).all()
    return p, g, s1, s2
