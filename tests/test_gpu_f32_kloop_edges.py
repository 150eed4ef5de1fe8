"""The k loops of the fp32 GEMM bodies (f32_kernels.hip gemm_body<P, SS>) at their edges: the
double-buffered forms store the next k-block into the other LDS image, the single-image forms hold
it in registers behind a second barrier; both guard that store and its loads with "one more
k-block".  Workgroups with exactly one k-block (no "more" iteration), two, three, and a short
last split must come out BIT-identical in every form.  (The whole network in every form:
test_gpu_f32_net.py::test_stage_split_gemms_bit_identical.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMS = (0, 1 + 4, 2 + 8, 3 + 12)  # register split | stage split, 2 LDS images | 1 image | 1 image, 3 waves


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("B", [32, 64, 96, 40])
def test_kloop_edges_fc1_backward(cuda, B):
    """FC1 backward: the weight gradient's K is the batch -- 1, 2 and 3 k-blocks of 32 samples and
    a ragged last block (B = 40)."""
    from apex_amd import ops

    hip = ops.hip()
    g = torch.Generator(device=cuda).manual_seed(100 + B)
    dz = torch.randn(B, 256, device=cuda, generator=g)
    a3 = torch.randn(B, 3136, device=cuda, generator=g).relu_()
    w = torch.randn(256, 3136, device=cuda, generator=g) * 0.02
    nws = hip.f32_fc1_wgrad_workspace_floats()
    prev_ss = hip.f32_stage_split()
    got = {}
    try:
        for form in FORMS:
            hip.f32_set_stage_split(form)
            dy3 = torch.full((B, 3136), float("nan"), device=cuda)
            ws = torch.full((nws,), float("nan"), device=cuda)
            hip.f32_fc1_bwd_split(dz.data_ptr(), a3.data_ptr(), w.data_ptr(), dy3.data_ptr(), ws.data_ptr(), B,
                                  _stream())
            torch.cuda.synchronize()
            got[form] = (dy3, ws[:256 * 3136].clone())
    finally:
        hip.f32_set_stage_split(prev_ss)
    assert bool(torch.isfinite(got[0][0]).all()) and bool(torch.isfinite(got[0][1]).all())
    for form in FORMS[1:]:
        assert torch.equal(got[0][0], got[form][0]), (form, "dgrad")
        assert torch.equal(got[0][1], got[form][1]), (form, "wgrad")


def _target_for(hip, layer: int, B: int, kbps: int) -> int:
    """A weight-gradient workgroup target whose split plan has ``kbps`` k-blocks per split."""
    ntiles = 8 if layer == 2 else 9
    for s in range(1, 2048):
        if hip.f32_wgrad_kbps(layer, B, s * ntiles) == kbps:
            return s * ntiles
    raise AssertionError((layer, B, kbps))


@pytest.mark.parametrize("layer", [3, 2])
def test_kloop_edges_conv_backward(cuda, layer):
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
    prev_ss = hip.f32_stage_split()
    ragged = 0
    try:
        for kbps in (1, 2, 3):
            target = _target_for(hip, layer, B, kbps)
            assert hip.f32_wgrad_kbps(layer, B, target) == kbps
            splits = hip.f32_wgrad_splits(layer, B, target)
            assert (splits - 1) * kbps < kbt <= splits * kbps
            ragged += kbt < splits * kbps
            nws = hip.f32_wgrad_workspace_floats(layer, B, target)
            got = {}
            for form in FORMS:
                hip.f32_set_stage_split(form)
                dx = torch.full((B, IH * IH, C), float("nan"), device=cuda)
                ws = torch.full((nws,), float("nan"), device=cuda)
                hip.f32_conv_bwd(layer, xin.data_ptr(), 0, 0, dy.data_ptr(), wt.data_ptr(), xin.data_ptr(),
                                 dx.data_ptr(), ws.data_ptr(), B, _stream(), target=target)
                torch.cuda.synchronize()
                got[form] = (dx, ws)
            assert bool(torch.isfinite(got[0][0]).all()) and bool(torch.isfinite(got[0][1]).all())
            for form in FORMS[1:]:
                assert torch.equal(got[0][0], got[form][0]), (kbps, form, "dgrad")
                assert torch.equal(got[0][1], got[form][1]), (kbps, form, "wgrad partials")
    finally:
        hip.f32_set_stage_split(prev_ss)
    assert ragged >= 1
