"""Prefetch depth of the fp32 GEMM bodies (f32_kernels.hip gemm_body<P, SS, D>): a ring of D
register stages keeps D k-blocks of operand loads in flight.  The ring changes neither the k
order, nor the staged values, nor the MFMA k-slots, so every depth is BIT-identical to depth 1,
in every GEMM form, down to workgroups with fewer k-blocks than stages."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMS = (0, 1 + 4, 2 + 8, 3 + 12)  # register split | stage split, 2 LDS images | 1 image | 1 image, 3 waves
DEPTHS = (1, 2, 3)


def _pf(d: int) -> int:
    """The same depth in all three fields: learner forward, backward pairs, small forward."""
    return (d - 1) * (1 + 4 + 16)


def _model(dev, A=18, seed=0):
    from apex_amd.models.dqn import DuelingDQN

    torch.manual_seed(seed)
    m = DuelingDQN.from_shapes((4, 84, 84), A).to(dev)
    with torch.no_grad():
        for mod in list(m.features) + list(m.advantage) + list(m.value):
            if getattr(mod, "bias", None) is not None:
                mod.bias.uniform_(-0.1, 0.1)
    m.flatten_parameters()
    return m


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("B", [96, 384, 343])
def test_prefetch_depths_bit_identical(cuda, B):
    """Every activation, the three Q rows, dz, every input gradient and every parameter
    gradient of the 3-problem learner pass (B = 96: the small tiles, B = 384: the learner-sized
    ones, B = 343: those with ragged last tiles and a non-empty xcd_chunk tail) at depths 1..3
    under the four GEMM forms against depth 1 of the register split."""
    from apex_amd import ops
    from apex_amd.models.fused import forward_multi
    from apex_amd.models.fused_f32 import F32DuelingNet, F32Workspace

    hip = ops.hip()
    A = 18
    m, mt = _model(cuda, A=A, seed=11), _model(cuda, A=A, seed=12)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    net, tnet = F32DuelingNet(m), F32DuelingNet(mt)
    x = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device=cuda)
    x2 = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device=cuda)
    dq = torch.randn(B, A, device=cuda) / B
    prev_ss, prev_pf = hip.f32_stage_split(), hip.f32_prefetch()
    outs = {}
    try:
        for form in FORMS:
            for d in DEPTHS:
                hip.f32_set_stage_split(form)
                hip.f32_set_prefetch(_pf(d))
                for p in m.parameters():
                    p.grad.fill_(float("nan"))
                wss = [F32Workspace(B, A, cuda, keep_for_backward=(i == 0)) for i in range(3)]
                forward_multi([(net, x, wss[0], None, None), (net, x2, wss[1], None, None),
                               (tnet, x2, wss[2], None, None)])
                net.backward(dq, x, wss[0])
                torch.cuda.synchronize()
                ws = wss[0]
                outs[form, d] = [t.clone() for t in (ws.a1, ws.a2, ws.a3, ws.h, ws.q, wss[1].q, wss[2].q, ws.dz,
                                                     ws.dy3, ws.dy2, ws.dy1)] + [p.grad.clone() for p in m.parameters()]
    finally:
        hip.f32_set_stage_split(prev_ss)
        hip.f32_set_prefetch(prev_pf)
    ref = outs[0, 1]
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    for key, out in outs.items():
        for i, (a, b) in enumerate(zip(ref, out)):
            assert torch.equal(a, b), (key, i, float((a - b).abs().max()))


@pytest.mark.parametrize("B", [32, 64, 96, 40])
def test_ring_edges_fc1_backward(cuda, B):
    """FC1 backward: the weight gradient's K is the batch -- 1, 2 and 3 k-blocks of 32 samples
    (fewer than, as many as, one more than the stages) and a ragged last block (B = 40)."""
    from apex_amd import ops

    hip = ops.hip()
    g = torch.Generator(device=cuda).manual_seed(100 + B)
    dz = torch.randn(B, 256, device=cuda, generator=g)
    a3 = torch.randn(B, 3136, device=cuda, generator=g).relu_()
    w = torch.randn(256, 3136, device=cuda, generator=g) * 0.02
    nws = hip.f32_fc1_wgrad_workspace_floats()
    prev_ss, prev_pf = hip.f32_stage_split(), hip.f32_prefetch()
    try:
        for form in FORMS:
            hip.f32_set_stage_split(form)
            got = {}
            for d in DEPTHS:
                hip.f32_set_prefetch(_pf(d))
                dy3 = torch.full((B, 3136), float("nan"), device=cuda)
                ws = torch.full((nws,), float("nan"), device=cuda)
                hip.f32_fc1_bwd_split(dz.data_ptr(), a3.data_ptr(), w.data_ptr(), dy3.data_ptr(), ws.data_ptr(), B,
                                      _stream())
                torch.cuda.synchronize()
                got[d] = (dy3, ws[:256 * 3136].clone())
            assert bool(torch.isfinite(got[1][0]).all()) and bool(torch.isfinite(got[1][1]).all())
            for d in DEPTHS[1:]:
                assert torch.equal(got[1][0], got[d][0]), (form, d, "dgrad")
                assert torch.equal(got[1][1], got[d][1]), (form, d, "wgrad")
    finally:
        hip.f32_set_stage_split(prev_ss)
        hip.f32_set_prefetch(prev_pf)


def _target_for(hip, layer: int, B: int, kbps: int) -> int:
    """A weight-gradient workgroup target whose split plan has ``kbps`` k-blocks per split."""
    ntiles = 8 if layer == 2 else 9
    for s in range(1, 2048):
        if hip.f32_wgrad_kbps(layer, B, s * ntiles) == kbps:
            return s * ntiles
    raise AssertionError((layer, B, kbps))


@pytest.mark.parametrize("layer", [3, 2])
def test_ring_edges_conv_backward(cuda, layer):
    """conv3 / conv2 backward at B = 32 (one sample block: a k-block per output position, 49 /
    81 in all) with the weight gradient split into 1, 2 and 3 k-blocks per workgroup; the plans
    with 2 k-blocks per split (49 = 24 x 2 + 1, 81 = 40 x 2 + 1) and conv3's with 3 (16 x 3 + 1)
    end in a shorter split.  The input-gradient half of the launch has 1..9 (conv3) / 1..4
    (conv2) taps per workgroup."""
    from apex_amd import ops

    hip = ops.hip()
    B = 32
    IH, C, OH, taps = (9, 64, 7, 9) if layer == 3 else (20, 32, 9, 16)
    kbt = OH * OH
    g = torch.Generator(device=cuda).manual_seed(200 + layer)
    xin = torch.randn(B, IH * IH, C, device=cuda, generator=g).relu_()
    dy = torch.randn(B, OH * OH, 64, device=cuda, generator=g)
    wt = torch.randn(taps, C, 64, device=cuda, generator=g) * 0.05
    prev_ss, prev_pf = hip.f32_stage_split(), hip.f32_prefetch()
    ragged = 0
    try:
        for kbps in (1, 2, 3):
            target = _target_for(hip, layer, B, kbps)
            assert hip.f32_wgrad_kbps(layer, B, target) == kbps
            splits = hip.f32_wgrad_splits(layer, B, target)
            assert (splits - 1) * kbps < kbt <= splits * kbps
            ragged += kbt < splits * kbps
            nws = hip.f32_wgrad_workspace_floats(layer, B, target)
            for form in FORMS:
                hip.f32_set_stage_split(form)
                got = {}
                for d in DEPTHS:
                    hip.f32_set_prefetch(_pf(d))
                    dx = torch.full((B, IH * IH, C), float("nan"), device=cuda)
                    ws = torch.full((nws,), float("nan"), device=cuda)
                    hip.f32_conv_bwd(layer, xin.data_ptr(), 0, 0, dy.data_ptr(), wt.data_ptr(), xin.data_ptr(),
                                     dx.data_ptr(), ws.data_ptr(), B, _stream(), target=target)
                    torch.cuda.synchronize()
                    got[d] = (dx, ws)
                assert bool(torch.isfinite(got[1][0]).all()) and bool(torch.isfinite(got[1][1]).all())
                for d in DEPTHS[1:]:
                    assert torch.equal(got[1][0], got[d][0]), (kbps, form, d, "dgrad")
                    assert torch.equal(got[1][1], got[d][1]), (kbps, form, d, "wgrad partials")
    finally:
        hip.f32_set_stage_split(prev_ss)
        hip.f32_set_prefetch(prev_pf)
    assert ragged >= 1
