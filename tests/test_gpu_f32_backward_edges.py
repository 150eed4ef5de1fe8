"""The fp32 backward kernels (f32_kernels.hip: the gemm2_k pairs Fc1Wgrad / Fc1Dgrad and
ConvWgrad<3|2> / Conv3DgradPT / Conv2DgradPT, f32_conv1_wgrad_x3_k<S>; conv_bwd_kernels.hip:
grad_finalize_k) against fp64 references at ragged multi-block batches, driven through the
bindings with every operand and every output between NaN guard rows.

Shapes (the plans are asserted through the API: a retuned default fails test_plans_reach_the_edges
instead of silently losing an edge):

  E1  B = 33: two sample blocks of 32, the second with ONE sample (nbb = 2); every input
      gradient has one ragged M-tile; conv1 on 17 workgroups, the last with one live sample
      (G = 17 partials: the finalize's wide path); conv2 kbt = 162, kbps = 6, 27 splits; conv3
      kbt = 98, kbps = 4, 25 splits (24 x 4 = 96: the last split has 2 k-blocks).  With a
      ``target`` the conv2 / conv3 plans of 8 and 7 splits (kbps 21 / 24 and 13 / 14) take the
      finalize's narrow path, 7 with its tail loop; the 8-split plans start mid-position.
  E2  B = 135 = 128 + 7: nbb = 5, the last block with 7 samples; Fc1Dgrad on 3 M-tiles (64, 64,
      7), the conv input gradients on 2 (128, 7); conv1 on 68 workgroups, the last with one live
      sample; conv2 kbt = 405, kbps = 13, 32 splits (31 x 13 = 403); conv3 kbt = 245, kbps = 9,
      28 splits (27 x 9 = 243): kbps is no multiple of nbb, splits begin in the middle of an
      output position and span several, both layers end in a 2-k-block split.
  E3  B = 257 = 2 x 128 + 1, conv3's input gradient only: three M-tiles per position (128, 128,
      1).  Conv3DgradPT decodes block -> (position, M-tile) over 81 positions; with one or two
      M-tiles per position a decode that takes both as remainders of the block index (block % 81,
      block % tpp) still visits every pair once (81 is odd), with three it does not.

No B = 512 case: the backward launchers do not branch on the batch size beyond these plans
(gemm2_k uses neither xcd_chunk nor a learner-sized class; f32_conv_bwd and f32_fc1_bwd_split
pick their kernels from ``layer``, ``tile`` and ``target`` alone).  Fc1Dgrad has one tile, so
only the conv input gradients are run at ``tile`` 1 (BK 32) and 2 (BK 16).

Inputs are synthetic per layer (seeded device generator: activations randn().relu_(), dy
randn() / B, weights at the scale of the model's init) and every reference is computed in fp64
from the SAME tensors the kernel read.  Every float operand is a slice of a NaN-filled tensor
with 1024 NaN rows before and after it (a buffer range longer than the operand, or a clamped
load that is not zeroed at use, pulls a NaN into a sum); every output lives in a NaN-filled
tensor with >= 1024 guard rows of its own row width on both sides (input gradients: a whole
M-tile of 128 samples and one more): no output element may stay NaN, no guard element may be
written.

Bounds (tests/test_gpu_f32_net.py): per element |got - fp64| / sum_k |a_k b_k| < 1e-6 for every
gemm_body layer, < 4e-7 for conv1's weight and bias gradient.  The finalized gradient against
the fp64 sum of the kernel's OWN partials: (ceil(G / 4) + 2) 2^-24 sum_g |part_g| per element
(sequential fp32 adds along a chain of ceil(G / 4) slices plus the 4-way combine; the narrow
path's tail lengthens one chain to floor(G / 4) + G % 4 slices -- G = 7: 4 slices, worst case
5 roundings -- the measured maxima stay below 2.5).  The sum-of-squares partials: 1e-6 relative.
The measured maxima: profiles/f32_backward_edges_fp64.md."""
import math

import pytest
import torch
from torch.nn.grad import conv2d_input, conv2d_weight

from .test_gpu_f32_net import _model, _nchw

pytestmark = pytest.mark.gpu

GUARD = 1024  # guard rows before / after every operand and every output
U = 2.0 ** -24  # fp32 unit roundoff
SHAPES = {"E1": 33, "E2": 135, "E3": 257}
# (shape, layer) -> kbt, kbps, splits of the default plan
PLANS = {("E1", 2): (162, 6, 27), ("E1", 3): (98, 4, 25), ("E2", 2): (405, 13, 32), ("E2", 3): (245, 9, 28)}
CONV = {2: (32, 4, 2, 20, 9), 3: (64, 3, 1, 9, 7)}  # layer -> C in, K, stride, IH, OH
BOUND_GEMM, BOUND_CONV1, BOUND_SUMSQ = 1e-6, 4e-7, 1e-6
SUMSQ = 4096  # sum-of-squares partial slots (one per finalize workgroup: <= 577 + 1 here)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _operand(t: torch.Tensor, width: int) -> torch.Tensor:
    """A copy of ``t`` with GUARD NaN rows of ``width`` floats before and after it."""
    assert t.dtype == torch.float32 and width % 4 == 0 and t.numel() % width == 0
    pad, n = GUARD * width, t.numel()
    big = torch.full((n + 2 * pad,), float("nan"), device=t.device)
    v = big[pad:pad + n].view(t.shape)
    v.copy_(t)
    assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + n:]).all())
    return v


class _Out:
    """An output of ``shape`` inside one NaN-filled tensor, ``guard_rows`` rows of ``width``
    floats before and after it (the sibling of test_gpu_f32_learner_tiles._Out for one region of
    any shape)."""

    def __init__(self, dev, shape, width: int, guard_rows: int = GUARD):
        assert width % 4 == 0 and guard_rows >= GUARD
        pad, n = guard_rows * width, math.prod(shape)
        self.big = torch.full((n + 2 * pad,), float("nan"), device=dev)
        self.t = self.big[pad:pad + n].view(shape)
        self.guards = (self.big[:pad], self.big[pad + n:])

    def ptr(self) -> int:
        return self.t.data_ptr()

    def check(self, name):
        bad = torch.isnan(self.t).flatten()
        assert not bool(bad.any()), (name, "unwritten elements", int(bad.sum()), bad.nonzero()[:4].flatten().tolist())
        for side, g in zip(("before", "after"), self.guards):
            hit = ~torch.isnan(g)
            assert not bool(hit.any()), (name, "store into the guard", side, int(hit.sum()),
                                         hit.nonzero()[:4].flatten().tolist())


def _scaled(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor) -> float:
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    return float(((got.double() - ref).abs() / scale.clamp_min(1e-30)).max())


def _report(shape: str, what: str, value: float, bound: float) -> None:
    print(f"EDGE {shape} {what} {value:.2e} (bound {bound:.0e})")
    assert value < bound, (shape, what, value, bound)


# ---------------------------------------------------------------- inputs and fp64 references
class _ConvCase:
    """conv2 / conv3 backward at batch B: layer input x (= the ReLU mask of the input
    gradient), output gradient dy, weights W (reference layout) and their w2t / w3t packing."""

    def __init__(self, dev, L: int, B: int):
        C, K, S, IH, OH = CONV[L]
        self.L, self.B, self.dev = L, B, dev
        g = torch.Generator(device=dev).manual_seed(1000 * L + B)
        self.x = _operand(torch.randn(B, IH * IH, C, device=dev, generator=g).relu_(), C)
        self.dy = _operand(torch.randn(B, OH * OH, 64, device=dev, generator=g) / B, 64)
        self.W = torch.randn(64, C, K, K, device=dev, generator=g) * 0.03
        self.wt = _operand(self.W.permute(2, 3, 1, 0).contiguous(), 64)  # [ky][kx][ci][co]
        share = float((self.x > 0).float().mean())
        assert 0.3 <= share <= 0.7, share
        self._w = self._d = None

    def launch(self, hip, target: int = 0, tile: int = 0):
        """One f32_conv_bwd launch; returns (input gradient, partial workspace) as _Out."""
        C, K, S, IH, OH = CONV[self.L]
        N, B = K * K * C, self.B
        splits, nws = hip.f32_wgrad_splits(self.L, B, target), hip.f32_wgrad_workspace_floats(self.L, B, target)
        assert nws == splits * (64 * N + 64)
        ws = _Out(self.dev, (nws,), N)
        dx = _Out(self.dev, (B, IH * IH, C), C, guard_rows=max(GUARD, 129 * IH * IH))
        hip.f32_conv_bwd(self.L, self.x.data_ptr(), 0, 0, self.dy.data_ptr(), self.wt.data_ptr(), self.x.data_ptr(),
                         dx.ptr(), ws.ptr(), B, _stream(), target=target, tile=tile)
        torch.cuda.synchronize()
        return dx, ws

    def nchw(self):
        C, K, S, IH, OH = CONV[self.L]
        return _nchw(self.x, self.B, C, IH), _nchw(self.dy, self.B, 64, OH)

    def wgrad_ref(self):
        """(dW, its error scale, db, its error scale) in fp64, reference layout (shared, read-only)."""
        if self._w is None:
            S = CONV[self.L][2]
            x, dy = self.nchw()
            self._w = (conv2d_weight(x, self.W.shape, dy, stride=S),
                       conv2d_weight(x.abs(), self.W.shape, dy.abs(), stride=S),
                       dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)))
        return self._w

    def dgrad_ref(self):
        """(dx before the mask, its error scale, mask) in fp64, NCHW (shared, read-only)."""
        if self._d is None:
            S = CONV[self.L][2]
            x, dy = self.nchw()
            W = self.W.double()
            self._d = (conv2d_input(x.shape, W, dy, stride=S),
                       conv2d_input(x.shape, W.abs(), dy.abs(), stride=S), x > 0)
        return self._d

    def partials(self, hip, ws: _Out, target: int = 0):
        """The workspace as fp64 (weight partials [G][co][ci][ky][kx], bias partials [G][co])."""
        C, K = CONV[self.L][:2]
        G, N = hip.f32_wgrad_splits(self.L, self.B, target), K * K * C
        part = ws.t[:G * 64 * N].view(G, 64, K, K, C).double().permute(0, 1, 4, 2, 3)
        return part, ws.t[G * 64 * N:].view(G, 64).double()


class _Conv1Case:
    """conv1 weight gradient at batch B: u8 frame stacks (dense, and the same stacks in a frame
    ring read through ids / idx with repeated entries) and the output gradient dy."""

    def __init__(self, dev, B: int):
        self.L, self.B, self.dev = 1, B, dev
        g = torch.Generator(device=dev).manual_seed(1000 + B)
        F_, R = 300, 100
        self.frames = torch.randint(0, 256, (F_, 84 * 84), dtype=torch.uint8, device=dev, generator=g)
        self.ids = torch.randint(0, F_, (R, 4), dtype=torch.int32, device=dev, generator=g)
        self.idx = torch.randint(0, R, (B,), dtype=torch.int32, device=dev, generator=g)
        self.idx[B - 1] = self.idx[0]  # the odd tail's only live sample repeats an earlier row
        assert len(torch.unique(self.idx)) < B
        self.x = self.frames[self.ids[self.idx.long()].long()].view(B, 4, 84, 84).contiguous()
        self.dy = _operand(torch.randn(B, 400, 32, device=dev, generator=g) / B, 32)
        self._w = None

    def launch(self, hip, target: int = 0, ring: bool = False) -> _Out:
        B = self.B
        nws, G = hip.f32_wgrad_workspace_floats(1, B, target), hip.f32_wgrad_splits(1, B, target)
        assert nws == G * (32 * 256 + 32)
        ws = _Out(self.dev, (nws,), 256)
        src = (self.frames.data_ptr(), self.ids.data_ptr(), self.idx.data_ptr()) if ring else (self.x.data_ptr(), 0, 0)
        hip.f32_conv_bwd(1, *src, self.dy.data_ptr(), 0, 0, 0, ws.ptr(), B, _stream(), target=target)
        torch.cuda.synchronize()
        return ws

    def wgrad_ref(self):
        if self._w is None:
            x, dy = self.x.double(), _nchw(self.dy, self.B, 32, 20)
            self._w = (conv2d_weight(x, (32, 4, 8, 8), dy, stride=4),
                       conv2d_weight(x, (32, 4, 8, 8), dy.abs(), stride=4),
                       dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)))
        return self._w

    def partials(self, hip, ws: _Out, target: int = 0):
        G = hip.f32_wgrad_splits(1, self.B, target)
        return ws.t[:G * 32 * 256].view(G, 32, 4, 8, 8).double(), ws.t[G * 32 * 256:].view(G, 32).double()


class _Fc1Case:
    """FC1 backward at batch B: dz, the layer input a3 ([b][p * 64 + c]) and wfc1p ([n][p * 64 + c])."""

    def __init__(self, dev, B: int):
        self.B, self.dev = B, dev
        g = torch.Generator(device=dev).manual_seed(4000 + B)
        self.dz = _operand(torch.randn(B, 256, device=dev, generator=g) / B, 256)
        self.a3 = _operand(torch.randn(B, 3136, device=dev, generator=g).relu_(), 3136)
        self.w = _operand(torch.randn(256, 3136, device=dev, generator=g) * 0.01, 3136)
        share = float((self.a3 > 0).float().mean())
        assert 0.3 <= share <= 0.7, share


_CASES = {}


def _case(kind, dev, *key):
    if (kind, key) not in _CASES:
        _CASES[kind, key] = kind(dev, *key)
    return _CASES[kind, key]


@pytest.fixture(scope="module", autouse=True)
def _free_cases():
    yield
    _CASES.clear()


@pytest.fixture(scope="module")
def hip(cuda):
    from apex_amd import ops

    return ops.hip()


# ---------------------------------------------------------------- finalize
def _finalize(dev, hip, jobs, outs, name) -> None:
    """grad_finalize of ``jobs`` (writing ``outs``) with its sum-of-squares partials: every
    output written, no guard touched, sumsq[:n] the fp64 sum of squares of the finalized gradients."""
    sumsq = torch.full((SUMSQ,), float("nan"), dtype=torch.float64, device=dev)
    n = hip.grad_finalize(jobs, _stream(), sumsq.data_ptr())
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        o.check((name, "finalized", i))
    assert 0 < n < SUMSQ
    assert bool(torch.isfinite(sumsq[:n]).all()) and bool(torch.isnan(sumsq[n:]).all()), (name, n)
    want = sum(float(o.t.double().pow(2).sum()) for o in outs)
    got = float(sumsq[:n].sum())
    assert want > 0 and abs(got - want) <= BOUND_SUMSQ * want, (name, got, want)


def _finalized_error(name, G: int, fin: torch.Tensor, part: torch.Tensor) -> float:
    """``fin`` against the fp64 sum over the G partials ``part`` (in fin's layout) under
    (ceil(G / 4) + 2) 2^-24 sum_g |part_g|; returns the maximum in units of 2^-24 sum_g |part_g|."""
    assert part.shape[0] == G and part.shape[1:] == fin.shape, (name, part.shape, fin.shape)
    err, mass = (fin.double() - part.sum(0)).abs(), part.abs().sum(0)
    worst = float((err / (U * mass).clamp_min(1e-300)).max())
    assert bool((err <= (math.ceil(G / 4) + 2) * U * mass).all()), (name, G, worst)
    return worst


def _check_conv_wgrad(shape, case, hip, ws: _Out, target: int = 0) -> None:
    """Partials against fp64 (layer bound), then grad_finalize of the same workspace against the
    fp64 sum of the partials."""
    L, dev = case.L, case.dev
    name = f"conv{L}" + (f" target {target}" if target else "")
    ws.check(name + " partials")
    G = hip.f32_wgrad_splits(L, case.B, target)
    part, bpart = case.partials(hip, ws, target)
    ref, scale, bref, bscale = case.wgrad_ref()
    bound = BOUND_CONV1 if L == 1 else BOUND_GEMM
    _report(shape, f"{name} wgrad partials G={G}", _scaled(part.sum(0), ref, scale), bound)
    _report(shape, f"{name} bias partials G={G}", _scaled(bpart.sum(0), bref, bscale), bound)
    grad = _Out(dev, tuple(ref.shape), ref[0].numel())
    bgrad = _Out(dev, tuple(bref.shape), bref.numel())
    job = hip.f32_conv_finalize_job(L, case.B, ws.ptr(), grad.ptr(), bgrad.ptr(), target)
    _finalize(dev, hip, [job], [grad, bgrad], name)
    ws.check(name + " partials after the finalize")
    fw, fb = _finalized_error(name, G, grad.t, part), _finalized_error(name + " bias", G, bgrad.t, bpart)
    print(f"EDGE {shape} {name} finalize G={G} weights {fw:.2f} bias {fb:.2f} x 2^-24 sum|part| "
          f"(bound {math.ceil(G / 4) + 2})")
    # and the finalized gradient itself against fp64 (partials + reduction), under the layer bound
    _report(shape, f"{name} wgrad finalized", _scaled(grad.t, ref, scale), bound)
    _report(shape, f"{name} bias finalized", _scaled(bgrad.t, bref, bscale), bound)


# ---------------------------------------------------------------- 6. the plans reach the edges
@pytest.mark.parametrize("shape", ["E1", "E2"])
def test_plans_reach_the_edges(hip, shape):
    """The default plans are the ones this file's shapes were chosen for: several sample blocks
    with a ragged last one, a shorter last split in at least one layer, splits that begin
    mid-position on E2 (kbps no multiple of nbb; E1's default plans have kbps 6 and 4 at nbb = 2,
    its mid-position plans are the 8-split ones of test_narrow_finalize_path), ragged multi-tile
    input gradients, and an odd batch for conv1."""
    B = SHAPES[shape]
    nbb = (B + 31) // 32
    assert nbb > 1 and B % 32 != 0
    shorter = 0
    for L in (2, 3):
        kbt, kbps, splits = PLANS[shape, L]
        OH, N = CONV[L][4], CONV[L][0] * CONV[L][1] ** 2
        assert kbt == OH * OH * nbb
        assert (hip.f32_wgrad_kbps(L, B), hip.f32_wgrad_splits(L, B)) == (kbps, splits), (shape, L)
        assert (splits - 1) * kbps < kbt <= splits * kbps
        if shape == "E2":
            assert kbps % nbb != 0
        shorter += kbt < splits * kbps
        assert hip.f32_wgrad_workspace_floats(L, B) == splits * (64 * N + 64)
        assert splits >= 16  # the finalize's wide path
    assert shorter >= 1
    assert B % 2 == 1
    assert (hip.f32_wgrad_splits(1, B), hip.f32_wgrad_kbps(1, B)) == ((B + 1) // 2, 2)
    assert (hip.f32_wgrad_splits(1, B, 1), hip.f32_wgrad_kbps(1, B, 1)) == (B, 1)
    assert hip.f32_wgrad_splits(1, B) >= 16
    assert hip.f32_fc1_wgrad_slices(B) == hip.f32_fc1_wgrad_splits() >= 1
    assert hip.f32_fc1_wgrad_workspace_floats() == hip.f32_fc1_wgrad_splits() * 256 * 3136
    # M-tiles of the input gradients: Fc1Dgrad BM 64, the conv ones BM 128
    assert B % 64 != 0 and B % 128 != 0
    assert (-(-B // 64), -(-B // 128)) == {"E1": (1, 1), "E2": (3, 2)}[shape]


# ---------------------------------------------------------------- 1. weight-gradient partials + finalize
@pytest.mark.parametrize("layer", [3, 2])
@pytest.mark.parametrize("shape", ["E1", "E2"])
def test_conv_wgrad_partials_and_finalize(cuda, hip, shape, layer):
    """ConvWgrad<L> under the default plan: the fp64 sum of the partials (weights, and the
    A_COLSUM bias partials) against conv2d_weight / sum dy in fp64 under 1e-6; grad_finalize's
    wide path on the same workspace against the fp64 sum of the partials, scattered from
    [co][ky][kx][ci] to [co][ci][ky][kx]; the workspace of exactly f32_wgrad_workspace_floats
    floats is written whole and nothing around it."""
    case = _case(_ConvCase, cuda, layer, SHAPES[shape])
    dx, ws = case.launch(hip)
    dx.check(f"conv{layer} input gradient")
    _check_conv_wgrad(shape, case, hip, ws)


@pytest.mark.parametrize("target", [0, 1])
@pytest.mark.parametrize("shape", ["E1", "E2"])
def test_conv1_wgrad_partials_and_finalize(cuda, hip, shape, target):
    """f32_conv1_wgrad_x3_k<2> on an odd batch (the last workgroup holds one live sample: its
    second sample has a clamped plane and zeroed dy) and <1> (``target`` 1: one partial per
    sample) against conv2d_weight in fp64 under 4e-7, then grad_finalize's wide path."""
    case = _case(_Conv1Case, cuda, SHAPES[shape])
    assert hip.f32_wgrad_kbps(1, case.B, target) == (1 if target else 2)
    _check_conv_wgrad(shape, case, hip, case.launch(hip, target), target)


@pytest.mark.parametrize("shape", ["E1", "E2"])
def test_fc1_backward(cuda, hip, shape):
    """Fc1Wgrad (k = the batch: a ragged last k-block) and Fc1Dgrad (E2: three M-tiles 64, 64, 7)
    in their one launch: the partials against dz^T a3 in fp64, the two finalize row jobs (sum +
    transpose [n][p * 64 + c] -> [n][c * 49 + p]) against the partials, the input gradient
    against dz W where a3 > 0 and exactly 0.0 elsewhere."""
    c = _case(_Fc1Case, cuda, SHAPES[shape])
    B, dev = c.B, cuda
    G, nws = hip.f32_fc1_wgrad_slices(B), hip.f32_fc1_wgrad_workspace_floats()
    assert nws == G * 256 * 3136  # every slice of the workspace is written at these batches
    ws, dy3 = _Out(dev, (nws,), 3136), _Out(dev, (B, 3136), 3136)
    hip.f32_fc1_bwd_split(c.dz.data_ptr(), c.a3.data_ptr(), c.w.data_ptr(), dy3.ptr(), ws.ptr(), B, _stream())
    torch.cuda.synchronize()
    ws.check("fc1 partials")
    dy3.check("fc1 input gradient")
    dz, a3, w = c.dz.double(), c.a3.double(), c.w.double()
    part = ws.t.view(G, 256, 3136).double()
    _report(shape, f"fc1 wgrad partials G={G}", _scaled(part.sum(0), dz.t() @ a3, dz.abs().t() @ a3), BOUND_GEMM)
    ga, gv = _Out(dev, (128, 3136), 3136), _Out(dev, (128, 3136), 3136)
    jobs = [hip.f32_fc1_finalize_job(0, G, ws.ptr(), ga.ptr()), hip.f32_fc1_finalize_job(1, G, ws.ptr(), gv.ptr())]
    _finalize(dev, hip, jobs, [ga, gv], "fc1")
    for half, out in enumerate((ga, gv)):
        own = part[:, half * 128:(half + 1) * 128].view(G, 128, 49, 64).permute(0, 1, 3, 2).reshape(G, 128, 3136)
        worst = _finalized_error(f"fc1 half {half}", G, out.t, own)
        print(f"EDGE {shape} fc1 finalize half {half} G={G} {worst:.2f} x 2^-24 sum|part|")
    mask = c.a3 > 0
    assert bool((dy3.t[~mask] == 0).all()), "masked input gradients are not exact zeros"
    ref, scale = dz @ w, dz.abs() @ w.abs()
    _report(shape, "fc1 dgrad", _scaled(dy3.t[mask], ref[mask], scale[mask]), BOUND_GEMM)


# ---------------------------------------------------------------- 2. the finalize's narrow path
def _target_for_splits(hip, layer: int, B: int, G: int) -> int:
    """A weight-gradient workgroup target whose plan has ``G`` splits."""
    ntiles = 8 if layer == 2 else 9
    for s in range(1, 256):
        if hip.f32_wgrad_splits(layer, B, s * ntiles) == G:
            return s * ntiles
    raise AssertionError((layer, B, G))


@pytest.mark.parametrize("G", [8, 7])
@pytest.mark.parametrize("layer", [3, 2])
def test_narrow_finalize_path(cuda, hip, layer, G):
    """conv2 / conv3 on E1 with a ``target`` that gives 8 and 7 splits: grad_finalize's narrow
    path (G < 16: 4 chains, and at G = 7 its tail loop) and long splits (13 .. 24 k-blocks, the
    8-split plans beginning mid-position), launch and finalize job built from the same target."""
    B = SHAPES["E1"]
    target = _target_for_splits(hip, layer, B, G)
    kbps, kbt = hip.f32_wgrad_kbps(layer, B, target), PLANS["E1", layer][0]
    assert hip.f32_wgrad_splits(layer, B, target) == G < 16
    assert (G - 1) * kbps < kbt <= G * kbps
    if G == 8:
        assert kbps % 2 != 0 and kbt < G * kbps  # mid-position starts, a shorter last split
    case = _case(_ConvCase, cuda, layer, B)
    dx, ws = case.launch(hip, target=target)
    dx.check(f"conv{layer} input gradient")
    _check_conv_wgrad("E1", case, hip, ws, target)


# ---------------------------------------------------------------- 3. input gradients
@pytest.mark.parametrize("shape,layer,tile", [(s, L, t) for s in ("E1", "E2") for L in (3, 2) for t in (1, 2)]
                         + [("E3", 3, 1), ("E3", 3, 2)])
def test_conv_dgrad_tiles(cuda, hip, shape, layer, tile):
    """Conv3DgradPT / Conv2DgradPT at BK 32 (``tile`` 1) and BK 16 (``tile`` 2), each on its own
    against conv2d_input in fp64: under 1e-6 where the layer input is positive, exactly 0.0
    everywhere else, every element written, nothing past the batch.  E3: conv3 on three M-tiles
    per position."""
    C, K, S, IH, OH = CONV[layer]
    case = _case(_ConvCase, cuda, layer, SHAPES[shape])
    assert -(-case.B // 128) == {"E1": 1, "E2": 2, "E3": 3}[shape]
    dx, ws = case.launch(hip, tile=tile)
    dx.check(f"conv{layer} tile {tile} input gradient")
    ws.check(f"conv{layer} tile {tile} partials")
    ref, scale, mask = case.dgrad_ref()
    got = _nchw(dx.t, case.B, C, IH)
    assert bool((got[~mask] == 0).all()), "masked input gradients are not exact zeros"
    _report(shape, f"conv{layer} dgrad tile {tile}", _scaled(got[mask], ref[mask], scale[mask]), BOUND_GEMM)


# ---------------------------------------------------------------- 4. conv1 through the frame ring
@pytest.mark.parametrize("target", [0, 1])
@pytest.mark.parametrize("shape", ["E1", "E2"])
def test_conv1_wgrad_frame_ring(cuda, hip, shape, target):
    """conv1's weight gradient reading frames[F, 84 * 84] through ids[R, 4] and idx[B] (repeated
    rows) is bit-identical to the dense launch on the gathered stacks: partials and finalized
    gradient."""
    case = _case(_Conv1Case, cuda, SHAPES[shape])
    fins = []
    wss = [case.launch(hip, target, ring=ring) for ring in (False, True)]
    for ring, ws in zip((False, True), wss):
        ws.check(f"conv1 partials ring={ring}")
        grad, bgrad = _Out(cuda, (32, 4, 8, 8), 256), _Out(cuda, (32,), 32)
        job = hip.f32_conv_finalize_job(1, case.B, ws.ptr(), grad.ptr(), bgrad.ptr(), target)
        _finalize(cuda, hip, [job], [grad, bgrad], f"conv1 ring={ring}")
        fins.append((grad, bgrad))
    assert torch.equal(wss[0].t, wss[1].t)
    assert torch.equal(fins[0][0].t, fins[1][0].t) and torch.equal(fins[0][1].t, fins[1][1].t)


# ---------------------------------------------------------------- 5. end to end
def test_backward_end_to_end_ragged_multi_block(cuda):
    """F32DuelingNet.backward at B = 135 (E2) against fp64 autograd, gradients NaN-poisoned
    first: the bounds of test_f32_backward_matches_fp64_autograd; ties heads_bwd and
    heads_wgrad at a ragged multi-block batch to a reference as well."""
    from apex_amd.models.fused_f32 import F32DuelingNet, F32Workspace

    A, B = 18, SHAPES["E2"]
    m = _model(cuda, A=A, seed=3)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    net = F32DuelingNet(m)
    g = torch.Generator(device=cuda).manual_seed(5000 + B)
    x = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device=cuda, generator=g)
    ws = F32Workspace(B, A, cuda, keep_for_backward=True)
    net(x, ws)
    dq = torch.randn(B, A, device=cuda, generator=g) / B
    for p in m.parameters():
        p.grad.fill_(float("nan"))
    net.backward(dq, x, ws)
    torch.cuda.synchronize()
    m64 = _model(cuda, A=A, seed=3).double()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    q = m64(x.double())
    (q * dq.double()).sum().backward()
    worst = 0.0
    for (name, p), p64 in zip(m.named_parameters(), m64.parameters()):
        ref = p64.grad
        err = float((p.grad.double() - ref).norm() / ref.norm().clamp_min(1e-30))
        worst = max(worst, err)
        assert err < 1e-4, (name, err)
        torch.testing.assert_close(p.grad.double(), ref, rtol=1e-3, atol=1e-4 * float(ref.abs().max()),
                                   msg=lambda s, n=name: f"{n}: {s}")
    print(f"EDGE E2 end to end: max relative norm error {worst:.2e} (bound 1e-04)")
