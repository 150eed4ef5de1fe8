"""The learner-sized fp32 forward kernels (f32_kernels.hip, launches of n * B >= 1024 rows)
against fp64 references.

At or above 1024 rows the launchers take other tiles and grids than the actor's / evaluator's
small launches: conv1 on 384 workgroups walking runs of samples, conv2 on 128 x 64 (tile 1:
64 x 64, tile 2: 128 x 64 as 4 x 1 waves), conv3 on 64 x 64 (tile 2: 128 x 64, tile 3:
128 x 32), FC1 under the learner's GEMM form.  Shapes:

  S1  n = 3, B = 343 (1029 rows): ragged last M-tiles (conv2 27783 = 217 x 128 + 7, conv3
      16807 = 262 x 64 + 39, FC1 343 = 5 x 64 + 23), a non-empty xcd_chunk tail (654 and 789
      tiles), conv1 runs of 3 samples that cross a problem boundary (343 = 3 x 114 + 1)
  S2  n = 2, B = 512 (1024 rows, the threshold itself): whole tiles; conv1 runs of 3 cross the
      problem boundary (512 = 3 x 170 + 2)

Problems 0 and 1 read the online net and problem 2 the target net; S2T is S2 with problem 1
on the target net, so that the one boundary a conv1 run crosses there separates different
weights.  Every problem has its own input.

Every layer's reference is computed from the SAME layer input the kernel read (the previous
kernel's output), per element scaled by the fp32 dot-product error scale
sum_k |a_k b_k| + |bias|; the bounds are those of tests/test_gpu_f32_net.py.  Every output
lives inside one larger NaN-filled tensor with guard rows around each problem's region: a
dropped tile leaves NaN rows, a store outside a region clears guard NaNs.
The measured maxima: profiles/f32_learner_tiles_fp64.md."""
import pytest
import torch
import torch.nn.functional as F

from .test_gpu_f32_net import _model, _nchw

pytestmark = pytest.mark.gpu

A = 18
SPLITS = 7  # FC1 forward split-K slabs
GUARD = 1024  # guard rows before / after every problem's region (>= one M-tile of 128)
SHAPES = {"S1": (3, 343, "oot"), "S2": (2, 512, "oo"), "S2T": (2, 512, "ot")}  # n, B, net per problem
SEED_ONLINE, SEED_TARGET = 21, 22
# (rows per sample, row width) of every kernel output
GEOM = {"a1": (400, 32), "a2": (81, 64), "a3": (49, 64), "z": (SPLITS, 256), "h": (1, 256), "q": (1, A)}
BOUND = {"conv1": 4e-7, "conv2": 1e-6, "conv3": 1e-6, "fc1": 1e-6}


def _learner_rows(n: int, B: int) -> int:
    """Every launch of this file but the small-path comparison is learner-sized."""
    assert n * B >= 1024, (n, B)
    return n * B


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _d(t):
    return t.detach().double()


class _Out:
    """One layer's outputs of n problems inside one NaN-filled tensor: GUARD rows, then per
    problem its region followed by GUARD rows."""

    def __init__(self, dev, n: int, B: int, name: str):
        per, width = GEOM[name]
        rows = (SPLITS * B) if name == "z" else per * B
        self.big = torch.full((GUARD + n * (rows + GUARD), width), float("nan"), device=dev)
        self.regions = [self.big[GUARD + i * (rows + GUARD):][:rows] for i in range(n)]
        self.guards = [self.big[i * (rows + GUARD):][:GUARD] for i in range(n + 1)]
        assert self.guards[-1].data_ptr() + self.guards[-1].numel() * 4 == self.big.data_ptr() + self.big.numel() * 4

    def check(self, name):
        for i, r in enumerate(self.regions):
            bad = torch.isnan(r).any(1)
            assert not bool(bad.any()), (name, "unwritten rows of problem", i, int(bad.sum()),
                                         bad.nonzero()[:4].flatten().tolist())
        for i, g in enumerate(self.guards):
            assert bool(torch.isnan(g).all()), (name, "store into guard", i, int((~torch.isnan(g)).any(1).sum()))


class _Case:
    """Nets and inputs of one shape; ``small``: the same problems launched one at a time."""

    def __init__(self, dev, n: int, B: int, which_net: str):
        from apex_amd import ops
        from apex_amd.models.fused_f32 import F32DuelingNet

        self.hip = ops.hip()
        self.dev, self.n, self.B = dev, n, B
        online, target = _model(dev, A=A, seed=SEED_ONLINE), _model(dev, A=A, seed=SEED_TARGET)
        on, tg = F32DuelingNet(online), F32DuelingNet(target)
        self.nets = [{"o": on, "t": tg}[k] for k in which_net]
        assert len(self.nets) == n
        g = torch.Generator(device=dev).manual_seed(1000 + B)
        self.x = [torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device=dev, generator=g) for _ in range(n)]
        self._chain = {}
        self._refs = {}

    # -------------------------------------------------------------- launches
    def launch(self, layer: str, src, small: bool = False, which=None, c1_grid: int = 0, tile: int = 0, B=None):
        """One launch of ``layer`` over the problems ``which`` (default: all) reading ``src[i]``;
        returns its _Out (heads: the pair h, q)."""
        which = list(range(self.n)) if which is None else which
        n, B, h, s = len(which), self.B if B is None else B, self.hip, _stream()
        if small:
            assert n * B < 1024
        else:
            _learner_rows(n, B)
        nets = [self.nets[i] for i in which]
        if layer == "heads":
            hh, q = _Out(self.dev, n, B, "h"), _Out(self.dev, n, B, "q")
            hd = []
            for k, net in enumerate(nets):
                m = net.model
                hd.append((src[k].data_ptr(), m.advantage[0].bias.data_ptr(), m.value[0].bias.data_ptr(),
                           m.advantage[2].weight.data_ptr(), m.advantage[2].bias.data_ptr(),
                           m.value[2].weight.data_ptr(), m.value[2].bias.data_ptr(), hh.regions[k].data_ptr(),
                           q.regions[k].data_ptr()))
            h.heads_fwd_multi(hd, SPLITS, B, A, s)
            return hh, q
        out = _Out(self.dev, n, B, {"conv1": "a1", "conv2": "a2", "conv3": "a3", "fc1": "z"}[layer])
        probs = []
        for k, net in enumerate(nets):
            f = net.model.features
            assert src[k].is_contiguous()
            w, bias = {"conv1": (f[0].weight, f[0].bias), "conv2": (net.w2p, f[2].bias),
                       "conv3": (net.w3p, f[4].bias), "fc1": (net.wfc1p, None)}[layer]
            probs.append((src[k].data_ptr(), 0, 0, w.data_ptr(), 0, 0 if bias is None else bias.data_ptr(),
                          out.regions[k].data_ptr()))
        if layer == "fc1":
            assert h.f32_fc1_fwd_multi(probs, B, s) == SPLITS
        else:
            h.f32_conv_fwd_multi(int(layer[-1]), probs, B, s, c1_grid=c1_grid, tile=tile)
        return out

    def chain(self, small: bool = False):
        """The five launches with the default tiles and forms (cached, read-only)."""
        if small not in self._chain:
            groups = [[i] for i in range(self.n)] if small else [list(range(self.n))]
            outs = []
            for which in groups:
                o = {"a1": self.launch("conv1", [self.x[i] for i in which], small, which)}
                o["a2"] = self.launch("conv2", o["a1"].regions, small, which)
                o["a3"] = self.launch("conv3", o["a2"].regions, small, which)
                o["z"] = self.launch("fc1", o["a3"].regions, small, which)
                o["h"], o["q"] = self.launch("heads", o["z"].regions, small, which)
                outs.append(o)
            torch.cuda.synchronize()
            self._chain[small] = outs
        return self._chain[small]

    # -------------------------------------------------------------- fp64 references
    def conv_ref(self, layer: str, i: int, xin: torch.Tensor):
        """(pre-activation, error scale) of conv ``layer`` of problem ``i`` from the input ``xin``
        (the kernel's own input), in the kernel's NHWC row layout."""
        f = self.nets[i].model.features
        L, st, C, H = {"conv1": (0, 4, 4, 84), "conv2": (2, 2, 32, 20), "conv3": (4, 1, 64, 9)}[layer]
        xd = xin.double() if layer == "conv1" else _nchw(xin, self.B, C, H)
        W, b = _d(f[L].weight), _d(f[L].bias)
        pre = F.conv2d(xd, W, b, stride=st)
        sc = F.conv2d(xd.abs(), W.abs(), b.abs(), stride=st)
        nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])  # noqa: E731
        return nhwc(pre), nhwc(sc)

    def cached_conv_ref(self, layer: str, i: int):
        """conv references of the default learner chain (shared by the tile tests: read-only)."""
        if (layer, i) not in self._refs:
            o = self.chain()[0]
            xin = {"conv1": self.x[i], "conv2": o["a1"].regions[i], "conv3": o["a2"].regions[i]}[layer]
            self._refs[layer, i] = self.conv_ref(layer, i, xin)
        return self._refs[layer, i]

    def fc1_ref(self, i: int, a3: torch.Tensor):
        m = self.nets[i].model
        hflat = _nchw(a3, self.B, 64, 7).reshape(self.B, -1)
        W = torch.cat([_d(m.advantage[0].weight), _d(m.value[0].weight)])
        bb = torch.cat([_d(m.advantage[0].bias), _d(m.value[0].bias)])
        return hflat @ W.t() + bb, hflat.abs() @ W.abs().t() + bb.abs()

    def q_ref(self, i: int, hk: torch.Tensor):
        m = self.nets[i].model
        hd = hk.double()
        adv = F.linear(hd[:, :128], _d(m.advantage[2].weight), _d(m.advantage[2].bias))
        val = F.linear(hd[:, 128:], _d(m.value[2].weight), _d(m.value[2].bias))
        return val + adv - adv.mean(1, keepdim=True)


_CASES = {}


def _case(dev, name: str) -> _Case:
    if name not in _CASES:
        _CASES[name] = _Case(dev, *SHAPES[name])
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def _free_cases():
    yield
    _CASES.clear()


def _relu_layer_error(name: str, got: torch.Tensor, pre: torch.Tensor, sc: torch.Tensor, active_only: bool) -> float:
    """Max scaled error of relu(pre) (``active_only``: over the ReLU-active outputs); outputs whose
    reference is clearly negative must be exact zeros."""
    assert got.shape == pre.shape, (name, got.shape, pre.shape)
    assert bool((got >= 0).all()), name
    neg = pre < -1e-6 * sc
    assert bool(neg.any()) and bool((got[neg] == 0).all()), (name, "clamped outputs are not exact zeros")
    err = (got.double() - F.relu(pre)).abs() / sc.clamp_min(1e-30)
    if active_only:
        err = err[pre > 1e-6 * sc]
    return float(err.max())


def _chain_errors(c: _Case, outs, which_of) -> dict:
    """Per-layer maxima (over the problems) of one chain; asserts the q and end-to-end bounds."""
    errs = {k: 0.0 for k in ("conv1", "conv2", "conv3", "fc1", "q", "e2e")}
    for o, which in zip(outs, which_of):
        for k, i in enumerate(which):
            for layer, src, dst in (("conv1", c.x[i], "a1"), ("conv2", o["a1"].regions[k], "a2"),
                                    ("conv3", o["a2"].regions[k], "a3")):
                pre, sc = c.conv_ref(layer, i, src)
                e = _relu_layer_error(layer, o[dst].regions[k], pre, sc, active_only=layer != "conv1")
                errs[layer] = max(errs[layer], e)
                del pre, sc
            pre, sc = c.fc1_ref(i, o["a3"].regions[k])
            errs["fc1"] = max(errs["fc1"], _relu_layer_error("fc1", o["h"].regions[k], pre, sc, True))
            q, q_ref = o["q"].regions[k], c.q_ref(i, o["h"].regions[k])
            errs["q"] = max(errs["q"], float((q.double() - q_ref).abs().max() / q_ref.abs().max()))
            torch.testing.assert_close(q.double(), q_ref, rtol=1e-4, atol=1e-4 * float(q_ref.abs().max()))
            with torch.no_grad():
                q32 = c.nets[i].model(c.x[i].float())
            e2e = float((q - q32).norm() / q32.norm())
            errs["e2e"] = max(errs["e2e"], e2e)
            assert e2e < 1e-5, (i, e2e)
    return errs


def _assert_bounds(tag: str, errs: dict) -> None:
    print(tag, {k: f"{v:.2e}" for k, v in errs.items()})
    for layer, bound in BOUND.items():
        if layer in errs:
            assert errs[layer] < bound, (tag, layer, errs[layer])


# ---------------------------------------------------------------- 1. per-layer fp64 anchor
@pytest.mark.parametrize("shape", ["S1", "S2", "S2T"])
def test_learner_layers_match_fp64(cuda, shape):
    """Every layer of every problem of the learner-sized launch (default tiles and forms):
    conv1 4e-7 of sum |x w| + |b| on every output, conv2 / conv3 / FC1 1e-6 on the ReLU-active
    outputs, exact zeros where the reference is clearly negative, q within rtol 1e-4, the whole
    net within 1e-5 of the fp32 module."""
    c = _case(cuda, shape)
    _learner_rows(c.n, c.B)
    outs = c.chain()
    _assert_bounds(f"learner {shape} n={c.n} B={c.B}", _chain_errors(c, outs, [list(range(c.n))]))


def test_small_path_same_inputs_fp64(cuda):
    """The small-path kernels (one problem per launch: 343 rows) on S1's problems and inputs:
    the comparison column of profiles/f32_learner_tiles_fp64.md, under the same bounds."""
    c = _case(cuda, "S1")
    outs = c.chain(small=True)
    _assert_bounds(f"small S1 n=1 B={c.B}", _chain_errors(c, outs, [[i] for i in range(c.n)]))


# ---------------------------------------------------------------- 2. rows written once, guards untouched
def test_learner_launch_writes_every_row_and_nothing_else(cuda):
    """S1: after the launch no output row of a1, a2, a3, z, h, q holds a NaN (no dropped tile, no
    tail tile mapped onto another tile's rows) and every guard row around every problem's region
    still holds only NaNs (no ragged tile storing past M)."""
    c = _case(cuda, "S1")
    _learner_rows(c.n, c.B)
    o = c.chain()[0]
    for name in ("a1", "a2", "a3", "z", "h", "q"):
        assert len(o[name].regions) == c.n and len(o[name].guards) == c.n + 1
        assert o[name].guards[0].shape[0] >= 128
        o[name].check(name)


# ---------------------------------------------------------------- 3. alternative tiles, conv1 grids
@pytest.mark.parametrize("layer,tile", [("conv2", 1), ("conv2", 2), ("conv3", 2), ("conv3", 3)])
def test_alternative_learner_tiles(cuda, layer, tile):
    """The tiles APEX_F32_TILES selects (passed as ``tile=``), on S1 and the default chain's
    input of the layer: fp64 bound, every row written, guards untouched.  Bit-identity with
    tile 0 is printed, not promised."""
    c = _case(cuda, "S1")
    _learner_rows(c.n, c.B)
    o = c.chain()[0]
    src, dst = ("a1", "a2") if layer == "conv2" else ("a2", "a3")
    out = c.launch(layer, o[src].regions, tile=tile)
    torch.cuda.synchronize()
    out.check(f"{layer} tile {tile}")
    err, same = 0.0, True
    for i in range(c.n):
        pre, sc = c.cached_conv_ref(layer, i)
        err = max(err, _relu_layer_error(layer, out.regions[i], pre, sc, True))
        same = same and torch.equal(out.regions[i], o[dst].regions[i])
    print(f"learner S1 {layer} tile {tile}: {err:.2e} bit-identical to tile 0: {same}")
    assert err < BOUND[layer], (layer, tile, err)


def test_conv1_grids_bit_identical(cuda):
    """conv1 on 384 workgroups (runs of 3 samples, one run crosses from problem 0 into 1), on
    129 (runs of 8 crossing both boundaries: the weights are re-split inside the run) and on
    1029 (one sample each: never re-splits, the reference of the other two): a sample's
    arithmetic does not depend on the grouping, so all three are bit-identical."""
    c = _case(cuda, "S1")
    total = _learner_rows(c.n, c.B)
    outs = {g: c.launch("conv1", c.x, c1_grid=g) for g in (total, 384, 129)}
    torch.cuda.synchronize()
    default = c.chain()[0]["a1"]
    for g, out in outs.items():
        out.check(f"conv1 grid {g}")
        for i in range(c.n):
            assert torch.equal(out.regions[i], outs[total].regions[i]), (g, i)
            assert torch.equal(out.regions[i], default.regions[i]), (g, i, "default grid")
    pre, sc = c.cached_conv_ref("conv1", c.n - 1)  # and the one-sample grid itself is anchored
    assert _relu_layer_error("conv1", outs[total].regions[c.n - 1], pre, sc, False) < BOUND["conv1"]


# ---------------------------------------------------------------- 5. folded PER draw on the learner grid
def _replay(dev, seed: int):
    from apex_amd.engine.hbm_replay import HBMReplay

    C = 4096
    g = torch.Generator(device=dev).manual_seed(seed)
    rp = HBMReplay(C, n_envs=64, device=dev, frame_capacity=C, seed=1234)
    prio = torch.rand(C, device=dev, generator=g) * 4 + 0.05
    prio[::7] = 0.0
    rp.write_priorities(torch.arange(C, dtype=torch.int32, device=dev), prio, dedup=False)
    rp.filled.fill_(C)
    rp.s_ids.copy_(torch.randint(0, C, (C, 4), dtype=torch.int32, device=dev, generator=g))
    rp.s2_ids.copy_(torch.randint(0, C, (C, 4), dtype=torch.int32, device=dev, generator=g))
    rp.frames.copy_(torch.randint(0, 256, rp.frames.shape, dtype=torch.uint8, device=dev, generator=g))
    return rp


def _draw_probs(rp, nets, idx, out):
    ids = (rp.s_ids, rp.s2_ids, rp.s2_ids)
    probs = []
    for k, net in enumerate(nets):
        f = net.model.features
        probs.append((rp.frames.data_ptr(), ids[k].data_ptr(), idx.data_ptr(), f[0].weight.data_ptr(), 0,
                      f[0].bias.data_ptr(), out.regions[k].data_ptr()))
    return probs


@pytest.mark.parametrize("B", [343, 1024])
def test_conv1_folded_draw_on_learner_grid(cuda, B):
    """conv1 drawing the PER rows itself (384 workgroups: runs of 3 samples at B = 343, of 8 at
    B = 1024 -- two draw trips per wave) against per_sample with the same seed, counter and beta
    followed by conv1 reading ``idx``: identical slots, IS weights and activations."""
    c = _case(cuda, "S1")
    hip, n = c.hip, 3
    _learner_rows(n, B)
    rp = _replay(cuda, seed=50 + B)
    beta = torch.full((1,), 0.55, device=cuda)
    counter = torch.full((1,), 5, dtype=torch.int64, device=cuda)
    got, idxs, ws = [], [], []
    for fold in (True, False):
        idx = torch.full((B,), -1, dtype=torch.int32, device=cuda)
        w = torch.full((B,), float("nan"), device=cuda)
        out = _Out(cuda, n, B, "a1")
        draw = None
        if fold:  # (engine/learner.py _conv1_draw, no staged rows)
            draw = hip.make_conv_sample(rp.tree, rp.filled.data_ptr(), beta.data_ptr(), rp.seed, counter.data_ptr(),
                                        idx.data_ptr(), w.data_ptr(), int(not rp.exact_mass))
        else:
            rp.sample_indices(B, idx, w, counter, beta)
        hip.f32_conv_fwd_multi(1, _draw_probs(rp, c.nets, idx, out), B, _stream(), draw=draw)
        torch.cuda.synchronize()
        out.check(f"conv1 draw={fold}")
        got.append(out)
        idxs.append(idx)
        ws.append(w)
    assert int(idxs[0].min()) >= 0 and int(idxs[0].max()) < rp.capacity
    assert torch.equal(idxs[0], idxs[1])
    assert bool(torch.isfinite(ws[0]).all()) and torch.equal(ws[0], ws[1])
    assert bool((rp.leaf_sum[idxs[0].long()] > 0).all())
    assert len(torch.unique(idxs[0])) > B // 8  # (a real draw, not one slot)
    for k in range(n):
        assert torch.equal(got[0].regions[k], got[1].regions[k]), k
    # and the drawn rows are the ones the activations came from: the same stacks as dense inputs
    j = idxs[0].long()
    dense = [rp.frames[t[j].long()].view(B, 4, 84, 84).contiguous() for t in (rp.s_ids, rp.s2_ids, rp.s2_ids)]
    ref = c.launch("conv1", dense, B=B)
    torch.cuda.synchronize()
    for k in range(n):
        assert torch.equal(ref.regions[k], got[0].regions[k]), k


def test_conv1_folded_draw_refuses_more_than_8_per_workgroup(cuda):
    """3 x 1025 samples on 384 workgroups would be 9 per workgroup: the launcher refuses (no launch)."""
    c = _case(cuda, "S1")
    B = 1025
    rp = _replay(cuda, seed=7)
    beta = torch.full((1,), 0.5, device=cuda)
    counter = torch.zeros(1, dtype=torch.int64, device=cuda)
    idx = torch.zeros(B, dtype=torch.int32, device=cuda)
    w = torch.zeros(B, device=cuda)
    out = _Out(cuda, 3, B, "a1")
    draw = c.hip.make_conv_sample(rp.tree, rp.filled.data_ptr(), beta.data_ptr(), rp.seed, counter.data_ptr(),
                                  idx.data_ptr(), w.data_ptr(), int(not rp.exact_mass))
    with pytest.raises(ValueError, match="samples per workgroup"):
        c.hip.f32_conv_fwd_multi(1, _draw_probs(rp, c.nets, idx, out), B, _stream(), draw=draw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.big).all())
