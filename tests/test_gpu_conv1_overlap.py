"""The fp32 conv1 forward's sample pipeline and the conv1 weight gradient's staging
(f32_kernels.hip: f32_conv1_fwd_x3_k<false|true>, f32_conv1_wgrad_x3_k<1|2>), at the shapes where
the pipelined paths do something.

The forward is its own reference.  When the total sample count is at most the grid, every
workgroup has ONE sample: no next-sample prefetch, no problem boundary inside a run, the weights
and the bias loaded once (the "one-sample launch").  A sample's arithmetic does not depend on
the grouping, so every grouped launch below must equal, bit for bit, one-sample launches over the
same samples: three problems in slices of at most 170 samples each (<= 510 samples on a grid of
512).

  B = 171, 3 problems, grid 512: 513 samples in runs of two (257 runs, 255 empty workgroups
      behind them).  Sample 171 -- problem 1's first -- is the second of its run: the weights,
      the bias and (with sign bits) the tile loop's variant change in the middle of a run.  The
      boundary at 342 starts a run; the last run is one sample long.
  B = 172: 516 samples, both boundaries at run starts, a full last run, 254 empty workgroups.
  inputs: dense u8 stacks; a frame ring read through ids (row b) and through idx -> ids, with
      scattered (random, repeated) frame ids; and ids tables whose rows sit 4 and 8 bytes off a
      16-byte boundary (the four ids of a row are then four loads, not one).
  the folded PER draw at 8 samples per workgroup (513 samples on 65 workgroups, both problem
      boundaries inside runs, a last run of one) with problem 0's sign bits on: slots, IS weights,
      a1 rows and sign bits against the separate sampling launch + one-sample launches, and the
      bits against the a1 rows themselves.

Every problem has its own weights and its own non-zero bias.  Outputs live between NaN guard
rows (a dropped sample leaves NaNs, a store outside a region clears guard NaNs).

The weight gradient at B = 1, 2, 3 with one and two samples per workgroup (an odd tail's dead
second sample), from dense stacks, through the idx -> ids lookup and from the batch's frame ids
(``batch_fid``): partials against fp64 under the bound of tests/test_gpu_f32_backward_edges.py
(4e-7 of sum |x dy|), and the three input paths bit-identical."""
import pytest
import torch
from torch.nn.grad import conv2d_weight

from .test_gpu_f32_backward_edges import BOUND_CONV1, _operand, _scaled
from .test_gpu_f32_backward_edges import _Out as _Flat
from .test_gpu_f32_learner_tiles import _Out as _Regions
from .test_gpu_f32_learner_tiles import _replay
from .test_gpu_f32_net import _nchw

pytestmark = pytest.mark.gpu

N = 3
GRID = 512  # the grid of every launch here: 3 x 171 = 513 samples are one more than it holds
SLICE = 170  # 3 x 170 <= GRID: one sample per workgroup
SENTINEL = 0x5A5A5A5A


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def hip(cuda):
    from apex_amd import ops

    return ops.hip()


@pytest.fixture(scope="module")
def weights(cuda):
    """Per problem: conv1 weights [32][4][8][8] and a non-zero bias, all different."""
    g = torch.Generator(device=cuda).manual_seed(77)
    ws = [torch.randn(32, 4, 8, 8, device=cuda, generator=g) * 0.02 for _ in range(N)]
    bs = [torch.randn(32, device=cuda, generator=g) * 0.3 + 0.05 * (k + 1) for k in range(N)]
    assert all(bool((b != 0).all()) for b in bs) and not torch.equal(bs[0], bs[1]) and not torch.equal(bs[1], bs[2])
    return ws, bs


class _Src:
    """The three problems' inputs in one of the modes; ``fields(k, lo)``: problem k's (in, ids, idx)
    pointers for the samples from ``lo`` on."""

    F, R = 600, 256

    def __init__(self, dev, B: int, mode: str):
        g = torch.Generator(device=dev).manual_seed(B * 10 + len(mode))
        self.mode, self.B = mode, B
        if mode == "dense":
            self.x = [torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device=dev, generator=g)
                      for _ in range(N)]
            return
        self.frames = torch.randint(0, 256, (self.F, 84 * 84), dtype=torch.uint8, device=dev, generator=g)
        off = {"ids": 0, "ids_idx": 0, "ids_off8": 2, "ids_idx_off4": 1}[mode]
        rows = self.R if "idx" in mode else B
        self.tables, self.idx = [], []
        for _ in range(N):
            buf = torch.zeros(rows * 4 + 4, dtype=torch.int32, device=dev)
            assert buf.data_ptr() % 16 == 0
            t = buf[off:off + rows * 4].view(rows, 4)
            t.copy_(torch.randint(0, self.F, (rows, 4), dtype=torch.int32, device=dev, generator=g))
            assert t.data_ptr() % 16 == 4 * off
            self.tables.append(t)
            self.idx.append(torch.randint(0, rows, (B,), dtype=torch.int32, device=dev, generator=g)
                            if "idx" in mode else None)

    def fields(self, k: int, lo: int):
        if self.mode == "dense":
            return self.x[k][lo:].data_ptr(), 0, 0
        if self.idx[k] is None:
            return self.frames.data_ptr(), self.tables[k][lo:].data_ptr(), 0
        return self.frames.data_ptr(), self.tables[k].data_ptr(), self.idx[k][lo:].data_ptr()


def _bits_tensor(dev, B: int):
    return torch.full((B, 400), SENTINEL, dtype=torch.int32, device=dev)


def _launch(hip, weights, fields, B: int, lo: int, hi: int, out: _Regions, bits, grid: int, draw=None):
    """conv1 over samples lo .. hi - 1 of every problem, into the same rows of ``out`` (and ``bits``)."""
    ws, bs = weights
    probs = []
    for k in range(N):
        p = (*fields(k, lo), ws[k].data_ptr(), 0, bs[k].data_ptr(), out.regions[k][lo * 400:].data_ptr())
        if k == 0 and bits is not None:
            p += (bits[lo:].data_ptr(),)
        probs.append(p)
    hip.f32_conv_fwd_multi(1, probs, hi - lo, _stream(), c1_grid=grid, draw=draw)


def _one_sample_launches(hip, weights, fields, B: int, dev, with_bits: bool):
    out, bits = _Regions(dev, N, B, "a1"), _bits_tensor(dev, B) if with_bits else None
    for lo in range(0, B, SLICE):
        hi = min(B, lo + SLICE)
        assert N * (hi - lo) <= GRID
        _launch(hip, weights, fields, B, lo, hi, out, bits, GRID)
    torch.cuda.synchronize()
    out.check("one-sample launches")
    return out, bits


def _bits_of(a1: torch.Tensor, B: int) -> torch.Tensor:
    """Sign words [B][400] of a1 rows [B * 400][32]: bit c = channel c > 0."""
    sh = torch.arange(32, device=a1.device, dtype=torch.int64)
    word = ((a1.view(B, 400, 32) > 0).to(torch.int64) << sh).sum(-1)
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)


@pytest.mark.parametrize("with_bits", [False, True], ids=["nobits", "bits"])
@pytest.mark.parametrize("mode", ["dense", "ids", "ids_idx", "ids_off8", "ids_idx_off4"])
@pytest.mark.parametrize("B", [171, 172])
def test_runs_of_two_equal_one_sample_launches(cuda, hip, weights, B, mode, with_bits):
    """513 / 516 samples on 512 workgroups (runs of two: a prefetched second sample, at B = 171 a
    problem boundary inside a run and a one-sample tail) against one-sample launches, bit for bit."""
    src = _Src(cuda, B, mode)
    per = (N * B + GRID - 1) // GRID
    assert per == 2 and (B % 2 == 1) == (B == 171)  # 171: sample 171 is the second of run 85
    ref, ref_bits = _one_sample_launches(hip, weights, src.fields, B, cuda, with_bits)
    out, bits = _Regions(cuda, N, B, "a1"), _bits_tensor(cuda, B) if with_bits else None
    _launch(hip, weights, src.fields, B, 0, B, out, bits, GRID)
    torch.cuda.synchronize()
    out.check(f"runs of two B={B} {mode}")
    for k in range(N):
        assert torch.equal(out.regions[k], ref.regions[k]), (B, mode, k)
    assert not torch.equal(out.regions[0][:400], out.regions[1][:400])  # (different problems, really)
    if with_bits:
        assert torch.equal(bits, ref_bits)
        assert torch.equal(bits, _bits_of(out.regions[0], B))
    if mode != "dense":  # the rows are the ring's: the same stacks as a dense one-sample launch
        k = N - 1
        rows = src.tables[k] if src.idx[k] is None else src.tables[k][src.idx[k].long()]
        dense = src.frames[rows.long()].view(B, 4, 84, 84).contiguous()
        o = _Regions(cuda, N, B, "a1")
        for lo in range(0, B, SLICE):
            _launch(hip, weights, lambda _k, lo_: (dense[lo_:].data_ptr(), 0, 0), B, lo, min(B, lo + SLICE), o, None, GRID)
        torch.cuda.synchronize()
        assert torch.equal(o.regions[k], out.regions[k])


def test_folded_draw_at_eight_samples_per_workgroup(cuda, hip, weights):
    """The folded PER draw at kC1xDrawMax = 8 samples per workgroup (two draw trips per wave, seven
    prefetched samples per run, both problem boundaries inside runs, a last run of one) with the
    sign bits on: idx, w, a1 and bits1 equal the sampling launch followed by one-sample launches."""
    B, grid = 171, 65
    assert (N * B + grid - 1) // grid == 8 and (N * B) % 8 == 1 and B % 8 != 0 and (2 * B) % 8 != 0
    rp = _replay(cuda, seed=91)
    beta = torch.full((1,), 0.55, device=cuda)
    counter = torch.full((1,), 9, dtype=torch.int64, device=cuda)
    tables = (rp.s_ids, rp.s2_ids, rp.s2_ids)

    def fields_of(idx):
        return lambda k, lo: (rp.frames.data_ptr(), tables[k].data_ptr(), idx[lo:].data_ptr())

    # the sampling launch, then one sample per workgroup
    idx_r = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    w_r = torch.full((B,), float("nan"), device=cuda)
    rp.sample_indices(B, idx_r, w_r, counter, beta)
    ref, ref_bits = _one_sample_launches(hip, weights, fields_of(idx_r), B, cuda, True)
    # the draw inside the conv1 launch
    idx = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    w = torch.full((B,), float("nan"), device=cuda)
    draw = hip.make_conv_sample(rp.tree, rp.filled.data_ptr(), beta.data_ptr(), rp.seed, counter.data_ptr(),
                                idx.data_ptr(), w.data_ptr(), int(not rp.exact_mass))
    out, bits = _Regions(cuda, N, B, "a1"), _bits_tensor(cuda, B)
    _launch(hip, weights, fields_of(idx), B, 0, B, out, bits, grid, draw=draw)
    torch.cuda.synchronize()
    out.check("folded draw, 8 per workgroup")
    assert int(idx.min()) >= 0 and int(idx.max()) < rp.capacity and len(torch.unique(idx)) > B // 8
    assert torch.equal(idx, idx_r)
    assert bool(torch.isfinite(w).all()) and torch.equal(w, w_r)
    for k in range(N):
        assert torch.equal(out.regions[k], ref.regions[k]), k
    assert torch.equal(bits, ref_bits)
    assert torch.equal(bits, _bits_of(out.regions[0], B))


class _Wgrad:
    """conv1 weight gradient inputs at batch B: a frame ring, ids / idx with a repeated row, the
    same stacks dense and as the batch's frame ids, and dy between NaN guard rows."""

    def __init__(self, dev, B: int):
        g = torch.Generator(device=dev).manual_seed(300 + B)
        F_, R = 200, 64
        self.B = B
        self.frames = torch.randint(0, 256, (F_, 84 * 84), dtype=torch.uint8, device=dev, generator=g)
        self.ids = torch.randint(0, F_, (R, 4), dtype=torch.int32, device=dev, generator=g)
        self.idx = torch.randint(0, R, (B,), dtype=torch.int32, device=dev, generator=g)
        self.fid = self.ids[self.idx.long()].contiguous()
        self.x = self.frames[self.fid.long()].view(B, 4, 84, 84).contiguous()
        self.dy = _operand(torch.randn(B, 400, 32, device=dev, generator=g) / B, 32)
        x, dy = self.x.double(), _nchw(self.dy, B, 32, 20)
        self.ref = (conv2d_weight(x, (32, 4, 8, 8), dy, stride=4), conv2d_weight(x, (32, 4, 8, 8), dy.abs(), stride=4),
                    dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)))

    def launch(self, hip, dev, target: int, path: str) -> _Flat:
        B = self.B
        G, nws = hip.f32_wgrad_splits(1, B, target), hip.f32_wgrad_workspace_floats(1, B, target)
        assert nws == G * (32 * 256 + 32)
        ws = _Flat(dev, (nws,), 256)
        src = {"dense": (self.x.data_ptr(), 0, 0), "lookup": (self.frames.data_ptr(), self.ids.data_ptr(), self.idx.data_ptr()),
               "fid": (self.frames.data_ptr(), 0, 0)}[path]
        kw = {"batch_fid": self.fid.data_ptr()} if path == "fid" else {}
        hip.f32_conv_bwd(1, *src, self.dy.data_ptr(), 0, 0, 0, ws.ptr(), B, _stream(), target=target, **kw)
        torch.cuda.synchronize()
        ws.check(f"conv1 wgrad B={B} target={target} {path}")
        return ws


@pytest.mark.parametrize("target", [0, 1], ids=["S2", "S1"])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_wgrad_paths_against_fp64_and_each_other(cuda, hip, B, target):
    """f32_conv1_wgrad_x3_k<2> (B = 1, 3: a dead second sample) and <1> from dense stacks, through
    idx -> ids and from batch_fid: each within 4e-7 of fp64, all three bit-identical."""
    assert hip.f32_wgrad_kbps(1, B, target) == (1 if target else 2)
    c = _Wgrad(cuda, B)
    G = hip.f32_wgrad_splits(1, B, target)
    assert G == (B if target else (B + 1) // 2)
    wss = {path: c.launch(hip, cuda, target, path) for path in ("dense", "lookup", "fid")}
    ref, scale, bref, bscale = c.ref
    for path, ws in wss.items():
        part = ws.t[:G * 32 * 256].view(G, 32, 4, 8, 8).double().sum(0)
        bpart = ws.t[G * 32 * 256:].view(G, 32).double().sum(0)
        ew, eb = _scaled(part, ref, scale), _scaled(bpart, bref, bscale)
        print(f"conv1 wgrad B={B} target={target} {path}: weights {ew:.2e} bias {eb:.2e} (bound {BOUND_CONV1:.0e})")
        assert ew < BOUND_CONV1 and eb < BOUND_CONV1, (path, ew, eb)
    assert torch.equal(wss["fid"].t, wss["lookup"].t)
    assert torch.equal(wss["fid"].t, wss["dense"].t)
