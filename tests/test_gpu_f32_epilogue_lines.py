"""Line-owned epilogue of the fp32 GEMM bodies against the element epilogue.

The line-owned epilogue (``f32_set_epilogue`` bits 3-5, one per launch class) takes the row-owned
values -- operand roles swapped on the MFMA, bias + ReLU, ReLU mask and sign bits per lane-owned
row -- and sends each 32 x 32 block through a wave-private piece of the LDS tile, so that 8
consecutive lanes hold the 128 bytes of one output row and every store instruction writes whole
lines.  Same products, same k order, same adds: every check is an exact (bitwise) equality against
the element epilogue (knob 0) -- activations, FC1 slabs, sign-bit words, the three input
gradients, the weight-gradient partials with their bias column sums (whose LDS reduction follows
the transpose in the same buffer), whole captured learner steps.  Every output sits in a
sentinel-filled buffer with room for 128 more samples: nothing may be written past the live rows
(a lane now tests four rows per block: 8k + lane / 8) and no sentinel may stay inside them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT_F = -7.31e22      # fp32 sentinel (no computed value equals it)
SENT_I = -1163005939   # 0xBAADF00D
PAD_SAMPLES = 128      # a tile reaches at most 127 rows (samples, for the position-major tiles) past the batch

FORMS_DEFAULT = 3 + 4 * 3 + 16 * (0 + 1)   # learner forward / backward pairs form 3, small forward form 0
FORMS_SMALL_3 = 3 + 4 * 3 + 16 * (3 + 1)   # the small-forward tiles on form 3 too
FORMS_REGISTER = 0 + 4 * 0 + 16 * (0 + 1)  # every class on the register split (form 0)

ELEMENT = 0
LINES = 8 + 16 + 32    # every class line-owned
LINES_OVER_ROWS = 7 + LINES  # the line bit wins over the class's row bit


def _model(dev, A=18, seed=0):
    """conv biases that leave whole sign-bit words zero and many stored outputs exactly 0."""
    from apex_amd.models.dqn import DuelingDQN

    torch.manual_seed(seed)
    m = DuelingDQN.from_shapes((4, 84, 84), A).to(dev)
    with torch.no_grad():
        for mod in list(m.features) + list(m.advantage) + list(m.value):
            if getattr(mod, "bias", None) is not None:
                mod.bias.uniform_(-0.1, 0.1)
        f = m.features
        f[0].bias.uniform_(-0.1, -0.01)
        f[0].bias[16:24] = -1e6
        f[2].bias[32:] = -1e6
        f[4].bias[:32] = -1e6
    m.flatten_parameters()
    return m


def _frames(B, dev, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device=dev, generator=g)
    x[::2, :, :40, :] = 0
    return x


def _pad(ws, names, keep):
    """Move the named workspace tensors to the front of sentinel-filled buffers with room for
    PAD_SAMPLES more samples behind them; the whole buffers land in ``keep``."""
    for name in names:
        t = getattr(ws, name)
        per = t.numel() // ws.B if name != "z" else 256
        sent = SENT_I if t.dtype == torch.int32 else SENT_F
        big = torch.full((t.numel() + PAD_SAMPLES * per,), sent, dtype=t.dtype, device=t.device)
        setattr(ws, name, big[:t.numel()].view(t.shape))
        keep[name] = (big, t.numel(), sent)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


_cache = {}


def _run(cuda, B, epi, resolve, forms=FORMS_DEFAULT, passes=1):
    """One forward (``passes`` problems in one launch per layer) and, for a single pass, the FC1 +
    conv backward from a fixed dz; returns {name: tensor} of every GEMM output (clones) with the
    tails of the padded buffers checked.  Cached: each configuration runs once."""
    key = (B, epi, resolve, forms, passes)
    if key in _cache:
        return _cache[key]
    from apex_amd import ops
    from apex_amd.models.fused_f32 import F32DuelingNet, F32Workspace, forward_multi_f32

    hip = ops.hip()
    prev = hip.f32_epilogue(), hip.f32_batch_resolve(), hip.f32_stage_split()
    out = {}
    try:
        hip.f32_set_epilogue(epi)
        assert hip.f32_epilogue() == epi
        hip.f32_set_batch_resolve(resolve)
        hip.f32_set_stage_split(forms)
        net = F32DuelingNet(_model(cuda))
        net.enable_backward(B)
        for p in net.model.parameters():
            p.grad = torch.zeros_like(p)
        wss, keeps = [], []
        for k in range(passes):
            ws = F32Workspace(B, 18, cuda, keep_for_backward=(k == 0))
            keep = {}
            _pad(ws, ("a2", "a3", "z") + (("dy3", "dy2", "dy1", "bits1", "bits2", "bits3") if k == 0 else ()), keep)
            wss.append(ws)
            keeps.append(keep)
        xs = [_frames(B, cuda, seed=k + 1) for k in range(passes)]
        forward_multi_f32([(net, xs[k], wss[k], None, None) for k in range(passes)], sign_bits=True)
        ws = wss[0]
        assert ws.bits_valid == bool(resolve & 1)
        if passes == 1:
            ws.dz.copy_(torch.randn(B, 256, device=cuda, generator=torch.Generator(device=cuda).manual_seed(7)))
            for t in (net._fc1_ws, *net._wgrad_wss):
                t.fill_(SENT_F)
            net._fc1_bwd(ws)
            net._conv_chain(xs[0], ws, None, None)
            out["fc1 partials"] = net._fc1_ws.clone()
            for k, t in zip((1, 2, 3), net._wgrad_wss):
                out[f"conv{k} partials"] = t.clone()  # (with the bias column sums behind the partials)
        torch.cuda.synchronize()
        for k, (w, keep) in enumerate(zip(wss, keeps)):
            for name, (big, n, sent) in keep.items():
                if name.startswith("bits") and not w.bits_valid:
                    assert bool((big == sent).all()), (name, "written without the knob")
                    continue
                if name.startswith("dy") and passes > 1:
                    continue
                assert bool((big[n:] == sent).all()), (name, k, "rows past the last live row were written")
                assert not bool((big[:n] == sent).any()), (name, k, "a sentinel inside the live rows")
                out[f"{name}[{k}]"] = big[:n].clone()
    finally:
        hip.f32_set_epilogue(prev[0])
        hip.f32_set_batch_resolve(prev[1])
        hip.f32_set_stage_split(prev[2])
    _cache[key] = out
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), name


# B = 1: one live row in a tile; 33: the rows end inside the second 32 x 32 block (and inside its
# first 8-row store group); 70: inside an 8-row store group of the third block, ragged second tile
# of 64; 130: ragged tile of 128 (conv2 forward, the input gradients), more than one M-tile
BATCHES = [1, 33, 70, 130]


@pytest.mark.parametrize("forms", [FORMS_DEFAULT, FORMS_SMALL_3, FORMS_REGISTER],
                         ids=["small-form0", "small-form3", "all-form0"])
@pytest.mark.parametrize("resolve", [0, 1], ids=["masks", "bits"])
@pytest.mark.parametrize("B", BATCHES)
def test_line_epilogue_bit_identical(cuda, B, resolve, forms):
    """a2, a3, FC1 slabs, sign-bit words, dy3 / dy2 / dy1, conv and FC1 weight-gradient partials:
    element epilogue (knob 0) against line-owned in every class, nothing written past the live rows."""
    old = _run(cuda, B, ELEMENT, resolve, forms)
    new = _run(cuda, B, LINES, resolve, forms)
    assert {"a2[0]", "a3[0]", "z[0]", "dy3[0]", "dy2[0]", "dy1[0]", "fc1 partials", "conv2 partials",
            "conv3 partials"} <= new.keys()
    assert ("bits2[0]" in new) == bool(resolve)
    _same(old, new)
    dy3 = new["dy3[0]"]
    assert bool((dy3 == 0).any()) and bool((dy3 != 0).any())  # the mask masks


@pytest.mark.parametrize("epi", [8, 16, 32, 1 + 16, LINES_OVER_ROWS],
                         ids=["learner-forward", "pairs", "small-forward", "rows-forward-lines-pairs", "over-rows"])
def test_line_epilogue_per_class(cuda, epi):
    """One class at a time on the line-owned epilogue (8 = the learner-sized forward, which B = 70
    does not reach: every launch stays as it was; 16 = the pairs; 32 = the small forward), mixed
    with row-owned classes, and with the row bits set beneath the line bits."""
    _same(_run(cuda, 70, ELEMENT, 1), _run(cuda, 70, epi, 1))


@pytest.mark.parametrize("B", BATCHES)
def test_line_epilogue_bits_and_fp32_masks_agree(cuda, B):
    """The masked input gradients of the line-owned epilogue: identical fed sign bits (applied to the
    lane-owned row before the transpose) or fp32 masks (read at the stored row after it)."""
    bits = _run(cuda, B, LINES, 1)
    masks = _run(cuda, B, LINES, 0)
    for name in ("dy3[0]", "dy2[0]", "dy1[0]", "fc1 partials", "conv1 partials", "conv2 partials", "conv3 partials"):
        assert torch.equal(_bits(bits[name]), _bits(masks[name])), name
    # and the words are the sign of what was stored
    for name, C in (("2", 64), ("3", 64)):
        w = bits[f"bits{name}[0]"].view(B, -1, C // 32)
        act = bits[f"a{name}[0]"].view(B, -1, C)
        sh = torch.arange(32, device=w.device, dtype=torch.int32)
        got = ((w.reshape(B, -1, C // 32, 1) >> sh) & 1).bool().reshape(B, -1, C)
        assert torch.equal(got, act > 0), name


def test_line_epilogue_learner_sized_forward(cuda):
    """3 x 342 = 1026 rows: the learner-sized forward tiles (conv2 128 x 64: two blocks per wave,
    conv3 / FC1 64 x 64 on form 3), problem boundaries inside a tile's rows; problem 0 writes the
    sign bits."""
    old = _run(cuda, 342, ELEMENT, 1, passes=3)
    new = _run(cuda, 342, LINES, 1, passes=3)
    assert {"a2[2]", "a3[1]", "z[2]", "bits2[0]", "bits3[0]"} <= new.keys()
    _same(old, new)


def test_captured_learner_steps_identical_with_line_epilogue(cuda):
    """Three captured learner steps at B = 96 on a 128-leaf replay, every class line-owned against
    every class element: the same parameters, gradient, loss, batch, IS weights, priorities."""
    from apex_amd import ops
    from apex_amd.engine.apex import ApexEngine, EngineConfig
    from apex_amd.engine.learner import LearnerConfig

    hip = ops.hip()
    prev = hip.f32_epilogue()
    engs = []
    try:
        for mask in (LINES, ELEMENT):
            hip.f32_set_epilogue(mask)  # read at launch: the graphs keep the kernels they captured
            cfg = EngineConfig(n_envs=16, replay_capacity=128, threshold_size=112, overlap=True, use_graphs=True,
                               publish_param_interval=2, target_update_interval=4,
                               learner=LearnerConfig(batch_size=96, forward="hip"))
            torch.manual_seed(0)
            eng = ApexEngine(cfg, cuda)
            eng.fill()
            eng.capture()
            for _ in range(3):
                eng.train_step()
            torch.cuda.synchronize()
            engs.append(eng)
    finally:
        hip.f32_set_epilogue(prev)
    la, lb = (e.learner for e in engs)
    for name in ("flat", "flat_grad", "loss", "idx", "w", "prio", "step_counter"):
        a, b = getattr(la, name), getattr(lb, name)
        assert torch.equal(_bits(a), _bits(b)), name
    assert torch.isfinite(la.flat).all() and la.idx.unique().numel() > 8


@pytest.mark.parametrize("forms", [3 + 4 * 0 + 16 * (3 + 1), 1 + 4 * 1 + 16 * (1 + 1), 2 + 4 * 2 + 16 * (2 + 1)],
                         ids=["swapped", "form1", "form2"])
def test_every_epilogue_is_built_at_every_form(cuda, forms):
    """Every class is built with every epilogue at every form (nothing is left to throw): the
    element and row-owned epilogues at forms that are not the classes' defaults (swapped: the small
    forward on form 3 and the pairs on form 0; every class on form 1; on form 2) launch and compute
    the bits of the defaults.  The prefetch ring's setter is gone with the ring."""
    from apex_amd import ops

    hip = ops.hip()
    assert not hasattr(hip, "f32_set_prefetch") and not hasattr(hip, "f32_prefetch")
    ref = _run(cuda, 8, LINES, 1, FORMS_DEFAULT)
    for epi in (ELEMENT, 7):
        _same(ref, _run(cuda, 8, epi, 1, forms))


def test_retired_prefetch_variable_throws():
    """A non-zero APEX_F32_PREFETCH is not ignored: in a process that has it, reading the form mask
    (as every GEMM launch does) raises, also after the mask was set by hand; zero is accepted.  The
    variable is read once per process, hence the child processes (they load the library only)."""
    import os
    import subprocess
    import sys

    code = ("from apex_amd import ops\nhip = ops.hip()\nhip.f32_set_stage_split(31)\n"
            "try:\n    print('mask', hip.f32_stage_split())\nexcept ValueError as e:\n    print('raised', e)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("4", "raised APEX_F32_PREFETCH"), ("0", "mask 31")):
        env = dict(os.environ, APEX_F32_PREFETCH=value, APEX_NO_AUTOBUILD="1")
        out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=120)
        assert want in out.stdout, (value, out.stdout, out.stderr[-500:])
