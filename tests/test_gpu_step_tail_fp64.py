"""The last launches of a learner step against fp64 (tests/step_tail_ref.py: torch fp64 autograd
through the real formulas, conditioned error scales counted from the kernels' code; the host
suite test_step_tail_ref_host.py shows that a correct fp32 evaluation fits them and a wrong one
does not): dqn_heads_bwd, the heads job of grad_finalize, the priority mix of the tree write,
rmsprop_step / adam_step / adam_step2 with reduce_norms, grad_sumsq, and the fp32 packed copies.

Everything is driven through the bindings.  Every float operand sits between 1024 NaN guard rows,
every output in a NaN-filled tensor with 1024 guard rows on both sides: no output element may
stay NaN, no guard may be written (for dz that includes the rows at and after B).  Each maximum
is printed as ``TAIL <case> <what> <value> (bound ...)``; profiles/step_tail_fp64.md records them.

dqn_heads_bwd cases (B, A) and what each reaches:

  (1, 1)     one live row, seven idle; the dueling mean cancels the whole advantage gradient
  (8, 6)     one exact workgroup, G = 1
  (9, 3)     a second workgroup with one row, G = 2
  (37, 18)   G = 5: a narrow finalize with a tail of 1
  (120, 17)  G = 15: the last narrow plan, tail 3; the second action batch holds one live action
  (121, 63)  G = 16: the first wide plan; a last workgroup with one row; the largest A; lane 63
             idle in the argmax
  (128, 16)  exactly one action batch

each with ``idx`` (slots with a repeat into a table of C = 4 B rows) and without, with the fp32
``dz`` output and with ``dz_bf``; B >= 8 carries the crafted rows of step_tail_ref.make_loss_case.

Optimizers: single steps from a given state at n in {1, 255, 256, 257, 262144, 262145} (262144 =
1024 workgroups x 256: the one-pass limit; 262145: the first grid-stride case), RMSprop centered
and not, Adam with weight_decay 0 and 1e-2, zero and random states, gradient scales 1e-2 and 20,
max_norm 0 / above the norm / below it, grad_scale 0.25, StepLR, Adam steps 0 .. 999, adam_step2,
n_partials 1 .. 1300, and the full fp32 net with its packed copies."""
import math

import numpy as np
import pytest
import torch

from . import step_tail_ref as R

pytestmark = pytest.mark.gpu

GUARD = 1024
U = R.U
BOUND_SUMSQ = 1e-6  # test_gpu_f32_backward_edges.BOUND_SUMSQ
# Adam's bias corrections are -expm1f(t log1pf(beta - 1)) (opt_dev.h make_rule): the bound carries no
# bias-correction term (with 1 - powf(beta, t) the device was 60 u |update| off at steps 1 and 2)
ADAM_BIAS_TERM = False


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _report(case: str, what: str, value: float, bound: float = 1.0) -> None:
    print(f"TAIL {case} {what} {value:.3g} (bound {bound:g})")
    assert value < bound, (case, what, value, bound)


class _Buf:
    """``shape`` floats inside a NaN-filled tensor with GUARD rows of ``width`` (>= 4) floats on
    both sides; an operand when ``data`` is given (copied in), else an output."""

    def __init__(self, dev, shape, width: int, data=None, dtype=torch.float32):
        n, pad = math.prod(shape), GUARD * max(int(width), 4)
        self.big = torch.full((n + 2 * pad,), float("nan"), device=dev, dtype=dtype)
        self.t = self.big[pad:pad + n].view(shape)
        self.guards = (self.big[:pad], self.big[pad + n:])
        if data is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(data)).to(dtype).view(shape))

    def ptr(self) -> int:
        return self.t.data_ptr()

    def check(self, name, written: bool = True) -> None:
        if written:
            bad = torch.isnan(self.t).flatten()
            assert not bool(bad.any()), (name, "unwritten elements", int(bad.sum()), bad.nonzero()[:4].flatten().tolist())
        for side, g in zip(("before", "after"), self.guards):
            hit = ~torch.isnan(g)
            assert not bool(hit.any()), (name, "store into the guard", side, int(hit.sum()),
                                         hit.nonzero()[:4].flatten().tolist())

    def np(self):
        return self.t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def hip(cuda):
    from apex_amd import ops

    return ops.hip()


_REFS = {}


def _loss_case(B, A, use_idx):
    """(inputs, fp64 reference), computed once per case and left unchanged."""
    if (B, A, use_idx) not in _REFS:
        c = R.make_loss_case(B, A, use_idx=use_idx)
        _REFS[B, A, use_idx] = (c, R.loss_heads_ref(c))
    return _REFS[B, A, use_idx]


@pytest.fixture(scope="module", autouse=True)
def _free_refs():
    yield
    _REFS.clear()


# ---------------------------------------------------------------- dqn_heads_bwd + heads finalize
class _LossRun:
    """One dqn_heads_bwd launch of case ``c`` (bf: the dz_bf output instead of dz)."""

    def __init__(self, dev, hip, c, bf: bool, step_value: int = 41):
        B, A = c["B"], c["A"]
        self.B, self.A, self.G = B, A, hip.dqn_heads_bwd_blocks(B)
        assert self.G == -(-B // 8)
        self.stride = (A + 1) * 128 + (A + 1) + 256
        op = lambda k, width: _Buf(dev, c[k].shape, width, c[k])  # noqa: E731
        self.ops = {k: op(k, A) for k in ("q", "q2", "q2t")}
        self.ops.update({k: op(k, 1) for k in ("rew", "done", "w")})
        self.ops.update(h=op("h", 256), w_adv2=op("w_adv2", 128), w_val2=op("w_val2", 128))
        self.act = torch.from_numpy(c["act"]).to(dev)
        self.idx = torch.from_numpy(c["idx"]).to(dev) if c["use_idx"] else None
        self.delta, self.lw = _Buf(dev, (B,), 1), _Buf(dev, (B,), 1)
        self.dz = _Buf(dev, (B, 256), 256, dtype=torch.bfloat16 if bf else torch.float32)
        self.part = _Buf(dev, (self.G, self.stride), self.stride)
        self.step = torch.full((1,), step_value, dtype=torch.int64, device=dev)
        self.snap = torch.full((2 * GUARD + 1,), -7, dtype=torch.int64, device=dev)
        self.args = {**{k: v.ptr() for k, v in self.ops.items()}, "act": self.act.data_ptr(),
                     "idx": 0 if self.idx is None else self.idx.data_ptr(), "delta": self.delta.ptr(),
                     "lw": self.lw.ptr(), ("dz_bf" if bf else "dz"): self.dz.ptr(), "part": self.part.ptr(),
                     "step": self.step.data_ptr(), "step_snap": self.snap[GUARD:].data_ptr()}
        hip.dqn_heads_bwd(self.args, B, A, float(c["gamma_n"]), _stream())
        torch.cuda.synchronize()
        for k, v in self.ops.items():
            v.check(k, written=True)  # operands: intact guards, unchanged contents
            assert torch.equal(v.t.cpu(), torch.from_numpy(c[k]).view(v.t.shape)), k
        for k in ("delta", "lw", "dz", "part"):
            getattr(self, k).check(k)
        assert int(self.snap[GUARD]) == step_value and int((self.snap != -7).sum()) == 1

    def partials(self):
        """The workspace as fp64: name -> [G][...] in the layout of the finalized gradient."""
        A, p = self.A, self.part.np()
        o = (A + 1) * 128
        return {"w_adv2": p[:, :A * 128].reshape(self.G, A, 128), "w_val2": p[:, A * 128:o],
                "b_adv2": p[:, o:o + A], "b_val2": p[:, o + A:o + A + 1], "b_adv1": p[:, o + A + 1:o + A + 129],
                "b_val1": p[:, o + A + 129:]}


def _bf16_ok(got: np.ndarray, ref: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """Within one bf16 ulp of the fp64 value rounded to bf16, or within the fp32 bound."""
    rounded = torch.from_numpy(ref).float().bfloat16().double().numpy()
    with np.errstate(divide="ignore"):
        ulp = np.where(ref == 0, 0.0, 2.0 ** (np.floor(np.log2(np.abs(np.where(ref == 0, 1.0, ref)))) - 7))
    return (np.abs(got - rounded) <= ulp) | (np.abs(got - ref) <= scale)


@pytest.mark.parametrize("use_idx", [True, False], ids=["idx", "rows"])
@pytest.mark.parametrize("B,A", R.LOSS_SHAPES)
def test_dqn_heads_bwd_and_finalize_match_fp64(cuda, hip, B, A, use_idx):
    from apex_amd.engine.hbm_replay import HBMReplay

    dev = cuda
    c, r = _loss_case(B, A, use_idx)
    ref, scale = r["ref"], r["scale"]
    case = f"B={B} A={A} {'idx' if use_idx else 'rows'}"
    run = _LossRun(dev, hip, c, bf=False)
    G = run.G
    assert (G >= 16) == (B >= 121)  # the narrow / wide switch of the finalize sits between 120 and 121
    for k in ("delta", "lw", "dz"):
        _report(case, k, R.ratio(getattr(run, k).np(), ref[k], scale[k]))
    # the rows of h = 0 and of g = 0 are exact zeros
    assert not run.dz.np()[~(c["h"] > 0)].any()
    # ---- the fp64 sum of the kernel's own partials
    part = run.partials()
    for k in R.HEAD_KEYS:
        _report(case, f"partials {k}", R.ratio(part[k].sum(0), ref[k], r["scale_part"][k]))
    # ---- the finalize: against the partials at the project's bound, against autograd end to end
    outs = {k: _Buf(dev, ref[k].shape, max(ref[k].shape[-1], 4)) for k in R.HEAD_KEYS}
    job = hip.heads_finalize_job(G, A, run.part.ptr(), *(outs[k].ptr() for k in R.HEAD_KEYS))
    sumsq = torch.full((256,), float("nan"), dtype=torch.float64, device=dev)
    n = hip.grad_finalize([job], _stream(), sumsq.data_ptr())
    torch.cuda.synchronize()
    assert n == -(-run.stride // (64 if G >= 16 else 256)) < 256
    assert bool(torch.isfinite(sumsq[:n]).all()) and bool(torch.isnan(sumsq[n:]).all())
    run.part.check("partials after the finalize")
    fin_bound = math.ceil(G / 4) + 2
    want_sq = 0.0
    for k in R.HEAD_KEYS:
        outs[k].check(k)
        got = outs[k].np()
        want_sq += float((got ** 2).sum())
        mass = np.abs(part[k]).sum(0)
        _report(case, f"finalize {k} x u sum|part|", R.ratio(got, part[k].sum(0), U * mass), fin_bound)
        _report(case, f"finalized {k}", R.ratio(got, ref[k], scale[k]))
    got_sq = float(sumsq[:n].sum())
    if want_sq > 0:
        _report(case, "sumsq", abs(got_sq - want_sq) / want_sq, BOUND_SUMSQ)
    else:
        assert got_sq == 0
    # ---- the priority mix of the tree write: loss mean and mixed priorities
    rp = HBMReplay(4096, 64, 3, 0.6, dev)
    slots = torch.arange(B, dtype=torch.int32, device=dev) * 3
    prio, loss = _Buf(dev, (B,), 1), _Buf(dev, (1,), 1)
    rp.write_priorities(slots, None, dedup=True, mix=(run.delta.t, run.lw.t, prio.t, loss.t))
    torch.cuda.synchronize()
    prio.check("prio")
    loss.check("loss")
    _report(case, "loss", R.ratio(loss.np().reshape(()), ref["loss"], scale["loss"]))
    _report(case, "prio", R.ratio(prio.np(), ref["prio"], scale["prio"]))
    # ---- the bf16 output: same launch otherwise, bit for bit
    runb = _LossRun(dev, hip, c, bf=True)
    for k in ("delta", "lw", "part"):
        assert torch.equal(getattr(run, k).t, getattr(runb, k).t), k
    ok = _bf16_ok(runb.dz.np(), ref["dz"], scale["dz"])
    assert ok.all(), (case, "dz_bf", int((~ok).sum()), np.argwhere(~ok)[:4].tolist())
    assert torch.equal(runb.dz.t, run.dz.t.bfloat16())  # the same d, rounded to nearest even


def test_dqn_heads_bwd_refuses_64_actions(cuda, hip):
    """A = 64 does not fit the argmax wave / the LDS tables: refused on the host, nothing launched."""
    B, A = 8, 64
    t = torch.full((B * 256 + (A + 1) * 129 + 256,), float("nan"), device=cuda)
    i = torch.zeros(B, dtype=torch.int32, device=cuda)
    step = torch.zeros(2, dtype=torch.int64, device=cuda)
    args = {k: t.data_ptr() for k in ("q", "q2", "q2t", "rew", "done", "w", "h", "w_adv2", "w_val2", "delta", "lw",
                                      "dz", "part")}
    args.update(act=i.data_ptr(), idx=0, step=step.data_ptr(), step_snap=step[1:].data_ptr())
    with pytest.raises(ValueError, match="1 <= A <= 63"):
        hip.dqn_heads_bwd(args, B, A, 0.97, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all()) and int(step[1]) == 0


# ---------------------------------------------------------------- optimizers
def _hp_obj(hip, kind, hp):
    if kind == "rms":
        o = hip.RMSpropParams(hp["lr"], hp["alpha"], hp["eps"], hp["max_norm"], hp["lr_gamma"], hp["lr_step_size"],
                              hp["lr_step_offset"], hp["centered"])
    else:
        o = hip.AdamParams(hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], hp["max_norm"],
                           hp["lr_gamma"], hp["lr_step_size"], hp["lr_step_offset"])
    o.grad_scale = hp["grad_scale"]
    return o


class _OptState:
    """(p, g, s1, s2) of n floats between guards, the gradient's sum-of-squares partials from
    grad_sumsq (checked against fp64 at 1e-12), norms_out between guards."""

    def __init__(self, dev, hip, p, g, s1, s2):
        self.n = n = len(p)
        self.host = (p, g, s1, s2)
        self.p, self.g, self.s1, self.s2 = (_Buf(dev, (n,), 4, t) for t in (p, g, s1, s2))
        self.partials = torch.full((hip.grad_norm_partials() + 2 * GUARD,), float("nan"), dtype=torch.float64,
                                   device=dev)
        self.parts = self.partials[GUARD:GUARD + hip.grad_norm_partials()]
        hip.grad_sumsq(self.g.ptr(), n, self.parts.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(self.parts).all()) and int(torch.isnan(self.partials).sum()) == 2 * GUARD
        want = float((g.astype(np.float64) ** 2).sum())
        assert abs(float(self.parts.sum()) - want) <= 1e-12 * want, (n, float(self.parts.sum()), want)
        self.norms = _Buf(dev, (4,), 4)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)

    def set(self, step: int):
        self.step.fill_(step)
        return self

    def check(self, case, ref):
        for k in ("p", "g", "s1", "s2"):
            getattr(self, k).check(k)
        self.norms.check("norms", written=False)
        assert torch.equal(self.g.t.cpu(), torch.from_numpy(self.host[1])), "the gradient is read-only"
        nv = self.norms.np()
        assert np.isfinite(nv[[0, 2, 3]]).all() and np.isnan(nv[1]), nv  # norms_out[1]: the host's statistic
        got = {"p": self.p.np(), "s1": self.s1.np(), "s2": self.s2.np()}
        worst = {k: R.ratio(got[k], ref["ref"][k], ref["scale"][k]) for k in got}
        for k, v in worst.items():
            _report(case, k, v)
        _report(case, "norms_out[0] / 2u", abs(nv[0] - ref["l2"]) / (2 * U * max(ref["l2"], 1e-300)))
        _report(case, "norms_out[2] / 8u", abs(nv[2] - ref["coef"]) / (8 * U * ref["coef"]))
        if ref["coef"] == 1.0:
            assert nv[2] == 1.0
        _report(case, "norms_out[3] / 4u", abs(nv[3] - ref["lr"]) / (4 * U * ref["lr"]))
        return got


def _step_gpu(hip, kind, st: _OptState, hp, n_partials=None, parts=None, **pk):
    fn = hip.rmsprop_step if kind == "rms" else hip.adam_step
    a, b = (st.s1, st.s2) if kind == "rms" else (st.s2, st.s1)  # Adam: (m, v) = (signed, positive)
    parts = st.parts if parts is None else parts
    fn(st.p.ptr(), st.g.ptr(), a.ptr(), b.ptr(), st.n, parts.data_ptr(), n_partials or parts.numel(),
       _hp_obj(hip, kind, hp), st.step.data_ptr(), st.norms.ptr(), _stream(), **pk)
    torch.cuda.synchronize()


def _ref(kind, state, hp, step):
    p, g, s1, s2 = state
    if kind == "rms":
        return R.rmsprop_ref(p, g, s1, s2, hp, step)
    r = R.adam_ref(p, g, s2, s1, hp, step, bias_term=ADAM_BIAS_TERM)
    # back to the (s1, s2) = (positive, signed) slots of _OptState
    r["ref"]["s1"], r["ref"]["s2"] = r["ref"]["s2"], r["ref"]["s1"]
    r["scale"]["s1"], r["scale"]["s2"] = r["scale"]["s2"], r["scale"]["s1"]
    return r


RULES = {"rms": ("rms", dict(centered=False)), "rms-centered": ("rms", dict(centered=True)),
         "adam": ("adam", dict(weight_decay=0.0)), "adam-wd": ("adam", dict(weight_decay=1e-2))}
# (state, gradient scale, max_norm, grad_scale)
CONFIGS = (("zero", 1e-2, 0.0, 1.0), ("random", 1e-2, 40.0, 1.0), ("random", 20.0, 40.0, 1.0), ("zero", 20.0, 40.0, 0.25))


def _mk_hp(kind, kw, **more):
    if kind == "rms":
        return R.rms_hp(6.25e-5, 0.95, 1.5e-7, **kw, **more)
    return R.adam_hp(1e-3, **kw, **more)


@pytest.mark.parametrize("n", R.OPT_SIZES)
@pytest.mark.parametrize("rule", list(RULES))
def test_optimizer_single_step_matches_fp64(cuda, hip, rule, n):
    kind, kw = RULES[rule]
    for ci, (state, gscale, max_norm, gs) in enumerate(CONFIGS):
        hp = _mk_hp(kind, kw, max_norm=max_norm, grad_scale=gs)
        host = R.make_opt_state(n, 100 * n % 9973 + ci, state, gscale, pscale=1e-2)
        step = 0 if state == "zero" else 4
        ref = _ref(kind, host, hp, step)
        if n >= 255:  # the clip is off, inactive (norm below max_norm) or active, as the config says
            assert (ref["coef"] < 1) == (gscale == 20.0), (ref["coef"], ref["l2"])
        st = _OptState(cuda, hip, *host).set(step)
        _step_gpu(hip, kind, st, hp)
        st.check(f"{rule} n={n} {state} g={gscale:g} max_norm={max_norm:g} gs={gs:g}", ref)


@pytest.mark.parametrize("rule", ["rms-centered", "adam"])
def test_step_lr(cuda, hip, rule):
    """StepLR gamma 0.5, step size 3, offset 0 and 1 at steps 2, 3, 5, 6; gamma 1 returns lr0 bit
    for bit whatever the step size."""
    kind, kw = RULES[rule]
    n = 257
    host = R.make_opt_state(n, 77, "random", 20.0, pscale=1e-2)
    rates = set()
    for offset in (0, 1):
        for step in (2, 3, 5, 6):
            hp = _mk_hp(kind, kw, max_norm=40.0, lr_gamma=0.5, lr_step_size=3, lr_step_offset=offset)
            ref = _ref(kind, host, hp, step)
            assert ref["lr"] == hp["lr"] * 0.5 ** ((step + offset) // 3)
            rates.add(ref["lr"])
            st = _OptState(cuda, hip, *host).set(step)
            _step_gpu(hip, kind, st, hp)
            st.check(f"{rule} steplr offset={offset} step={step}", ref)
    assert len(rates) == 3
    hp = _mk_hp(kind, kw, max_norm=40.0, lr_gamma=1.0, lr_step_size=3, lr_step_offset=1)
    st = _OptState(cuda, hip, *host).set(6)
    _step_gpu(hip, kind, st, hp)
    assert st.norms.t[3].item() == float(np.float32(hp["lr"]))


def _torch_adam_fp32(p, g, hp, step):
    """torch.optim.Adam in fp32 on the CPU: one step from the zero state at step count ``step``."""
    tp = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"],
                           weight_decay=hp["weight_decay"], foreach=False)
    opt.state[tp] = {"step": torch.tensor(float(step)), "exp_avg": torch.zeros_like(tp),
                     "exp_avg_sq": torch.zeros_like(tp)}
    tp.grad = torch.from_numpy(g.copy())
    opt.step()
    return tp.detach().double().numpy()


@pytest.mark.parametrize("rule", ["adam", "adam-wd"])
def test_adam_steps(cuda, hip, rule):
    """Adam at steps 0, 1, 2, 9, 999 (t = step + 1): from a random state against the bound; from
    the zero state (no cancellation in m': a uniform relative error) the update error in units of
    u |update|, printed beside torch.optim.Adam's in fp32 on the same inputs (parameters at the
    scale of the update, so that the rounding of p' is one of those units)."""
    kind, kw = RULES[rule]
    n = 1000
    for step in (0, 1, 2, 9, 999):
        hp = _mk_hp(kind, kw)
        host = R.make_opt_state(n, 31 + step, "random", 1e-2, pscale=1e-2)
        st = _OptState(cuda, hip, *host).set(step)
        _step_gpu(hip, kind, st, hp)
        st.check(f"{rule} step={step} random", _ref(kind, host, hp, step))
        host = R.make_opt_state(n, 57 + step, "zero", 1e-2, pscale=1e-3)
        ref = _ref(kind, host, hp, step)
        st = _OptState(cuda, hip, *host).set(step)
        _step_gpu(hip, kind, st, hp)
        got = st.check(f"{rule} step={step} zero", ref)
        unit = U * np.abs(ref["update"])
        ours = R.ratio(got["p"], ref["ref"]["p"], unit)
        theirs = R.ratio(_torch_adam_fp32(host[0], host[1], hp, step), ref["ref"]["p"], unit)
        print(f"TAIL adam-table {rule} step={step} kernel {ours:.1f} torch-fp32 {theirs:.1f} u|update| "
              f"(bound {float(np.max(ref['c'])):.0f} u|update| + u|p|)")


def test_adam_step2(cuda, hip):
    """Two sets in one launch, 1000 elements and 1, of different norms: the first clipped, the
    second not; each against its own fp64 step, each with its own norms."""
    hp = R.adam_hp(1e-3, max_norm=10.0)
    hosts = (R.make_opt_state(1000, 5, "random", 20.0, pscale=1e-2), R.make_opt_state(1, 6, "random", 0.5, pscale=1e-2))
    sts = [_OptState(cuda, hip, *h).set(3) for h in hosts]
    refs = [_ref("adam", h, hp, 3) for h in hosts]
    assert refs[0]["coef"] < 1 and refs[1]["coef"] == 1
    sets = [[st.p.ptr(), st.g.ptr(), st.s2.ptr(), st.s1.ptr(), st.n, st.parts.data_ptr(), st.parts.numel(),
             st.norms.ptr()] for st in sts]
    hip.adam_step2(sets[0], sets[1], _hp_obj(hip, "adam", hp), sts[0].step.data_ptr(), _stream())
    torch.cuda.synchronize()
    for i, (st, ref) in enumerate(zip(sts, refs)):
        st.check(f"adam_step2 set {i} n={st.n}", ref)


@pytest.mark.parametrize("n_partials", [1, 256, 577, 1024, 1025, 1300])
def test_reduce_norms(cuda, hip, n_partials):
    """Synthetic positive fp64 partials: norms_out[0] within 2 u of sqrt(sum) * grad_scale, the
    clip coefficient from it, nothing read past n_partials (NaN behind them)."""
    rs = np.random.RandomState(n_partials)
    vals = rs.rand(n_partials) * 3 + 0.01
    buf = torch.full((n_partials + 2 * GUARD,), float("nan"), dtype=torch.float64, device=cuda)
    buf[GUARD:GUARD + n_partials] = torch.from_numpy(vals).to(cuda)
    hp = R.rms_hp(6.25e-5, 0.95, 1.5e-7, max_norm=2.0, grad_scale=0.25)
    host = R.make_opt_state(1, 3, "random", 1.0)
    st = _OptState(cuda, hip, *host)
    _step_gpu(hip, "rms", st, hp, n_partials=n_partials, parts=buf[GUARD:])
    l2 = math.sqrt(float(vals.sum())) * hp["grad_scale"]
    nv = st.norms.np()
    _report(f"reduce_norms n_partials={n_partials}", "norms_out[0] / 2u", abs(nv[0] - l2) / (2 * U * l2))
    coef = min(hp["max_norm"] / (l2 + R.f32(1e-6)), 1.0)
    _report(f"reduce_norms n_partials={n_partials}", "norms_out[2] / 8u", abs(nv[2] - coef) / (8 * U * coef))
    assert np.isfinite(st.p.np()).all()


def test_five_step_carry_drift_report(cuda, hip):
    """Five carried steps: the drift of the kernels and of torch fp32 from the fp64 chain.  A
    report (printed, not asserted: rounding differences compound through the state); the
    single-step tests above are the check."""
    n = 1000
    for rule in ("rms-centered", "adam"):
        kind, kw = RULES[rule]
        hp = _mk_hp(kind, kw, max_norm=40.0)
        p0, g0, s1, s2 = R.make_opt_state(n, 9, "zero", 1.0, pscale=1e-2)
        st = _OptState(cuda, hip, p0, g0, s1, s2)
        tp = torch.from_numpy(p0.copy()).requires_grad_(True)
        if kind == "rms":
            opt = torch.optim.RMSprop([tp], lr=hp["lr"], alpha=hp["alpha"], eps=hp["eps"], centered=True)
        else:
            opt = torch.optim.Adam([tp], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
        state = (p0.astype(np.float64), None, s1.astype(np.float64), s2.astype(np.float64))
        rs = np.random.RandomState(10)
        for step in range(5):
            g = (rs.randn(n) * (20 if step % 2 else 0.01)).astype(np.float32)
            st.g.t.copy_(torch.from_numpy(g))
            hip.grad_sumsq(st.g.ptr(), n, st.parts.data_ptr(), _stream())
            st.set(step)
            _step_gpu(hip, kind, st, hp)
            tp.grad = torch.from_numpy(g.copy())
            torch.nn.utils.clip_grad_norm_([tp], hp["max_norm"])
            opt.step()
            r = _ref(kind, (state[0], g, state[2], state[3]), hp, step)
            state = (r["ref"]["p"], None, r["ref"]["s1"], r["ref"]["s2"])
        total = np.abs(state[0] - p0).max()
        print(f"TAIL carry {rule} 5 steps: kernel {np.abs(st.p.np() - state[0]).max() / total:.2e} torch-fp32 "
              f"{np.abs(tp.detach().double().numpy() - state[0]).max() / total:.2e} of the largest 5-step change")


@pytest.mark.parametrize("kind", ["rms", "adam"])
def test_full_fp32_net_step_and_packed_copies(cuda, hip, kind):
    """F32DuelingNet at A = 6 through opt_pack_args (PackMap.arena_f32 + FcPack.wp_f32: the default
    learner's optimizer launch): parameters and moments against fp64; the arena, NaN-filled before
    the step, equals repack() of the updated master bit for bit."""
    from apex_amd.models.fused_f32 import F32DuelingNet

    from .test_gpu_f32_net import _model

    m = _model(cuda, A=6, seed=4)
    flat = m.flatten_parameters()
    net = F32DuelingNet(m)
    P = flat.numel()
    assert P == sum(nn for _, _, nn in m.param_segments())
    p0 = flat.cpu().numpy().copy()
    _, g, s1, s2 = R.make_opt_state(P, 21, "random", 1e-2)
    dev_t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    gt, a1, a2 = dev_t(g), dev_t(s1), dev_t(s2)
    hp = (R.rms_hp(6.25e-5, 0.95, 1.5e-7, max_norm=0.5, centered=True) if kind == "rms"
          else R.adam_hp(1e-3, max_norm=0.5))
    step_v = 4
    ref = _ref(kind, (p0, g, s1, s2), hp, step_v)
    assert ref["coef"] < 1
    # the count the fused learner passes is the finalize's (for example 578), not 256
    n_partials = 578
    parts = torch.zeros(n_partials, dtype=torch.float64, device=cuda)
    chunks = np.array_split(g.astype(np.float64) ** 2, n_partials)
    parts.copy_(torch.tensor([float(ch.sum()) for ch in chunks], dtype=torch.float64))
    norms = torch.full((4,), float("nan"), device=cuda)
    step = torch.full((1,), step_v, dtype=torch.int64, device=cuda)
    pk = net.opt_pack_args()
    net.arena.fill_(float("nan"))
    fn = hip.rmsprop_step if kind == "rms" else hip.adam_step
    x1, x2 = (a1, a2) if kind == "rms" else (a2, a1)
    fn(flat.data_ptr(), gt.data_ptr(), x1.data_ptr(), x2.data_ptr(), P, parts.data_ptr(), n_partials,
       _hp_obj(hip, kind, hp), step.data_ptr(), norms.data_ptr(), _stream(), **pk)
    torch.cuda.synchronize()
    case = f"full net {kind}"
    for k, t in (("p", flat), ("s1", a1), ("s2", a2)):
        _report(case, k, R.ratio(t.double().cpu().numpy(), ref["ref"][k], ref["scale"][k]))
    _report(case, "norms_out[0] / 2u", abs(float(norms[0]) - ref["l2"]) / (2 * U * ref["l2"]))
    assert not bool(torch.isnan(net.arena).any()), ("arena positions nobody wrote", int(torch.isnan(net.arena).sum()))
    stepped = net.arena.clone()
    net.repack()
    torch.cuda.synchronize()
    assert torch.equal(stepped.view(torch.int32), net.arena.view(torch.int32))
