"""ReLU sign bits: written by the conv forwards of the gradient pass, read by the input gradients.

The conv1 / conv2 / conv3 forwards of problem 0 also write one bit per stored activation (set
exactly when it is > 0, words of 32 channels: bits1 [B][400], bits2 [B][81][2], bits3 [B][49][2]);
the FC1 / conv3 / conv2 input gradients then mask with those bits instead of re-reading the fp32
activation.  Nothing computed changes: every check here is an exact equality."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -1163005939  # 0xBAADF00D
PAD = 64                # sentinel words on each side of a bits buffer


def _model(dev, A=18, seed=0):
    """Biases that make whole words zero and many stored outputs exactly 0: conv1 biases all
    negative (pixels over all-zero frames then store 0 on every channel: a zero word), channels
    16..23 far below zero; conv2 channels 32..63 (its word 1) and conv3 channels 0..31 (its word 0)
    far below zero."""
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
    x[::2, :, :40, :] = 0  # every other sample: output rows 0..8 of conv1 see only zeros
    return x


def _padded_bits(ws):
    """Move the workspace's bits buffers into sentinel-filled buffers with PAD words around."""
    bufs = {}
    for name in ("bits1", "bits2", "bits3"):
        t = getattr(ws, name)
        big = torch.full((PAD + t.numel() + PAD,), SENTINEL, dtype=torch.int32, device=t.device)
        setattr(ws, name, big[PAD:PAD + t.numel()].view(t.shape))
        bufs[name] = big
    return bufs


def _unpack(bits, C):
    """[B][P] or [B][P][2] words -> bool [B][P][C] (bit c of word c // 32)."""
    B, P = bits.shape[0], bits.shape[1]
    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits.reshape(B, P, -1, 1) >> sh) & 1).bool().reshape(B, P, C)


def _check_bits(ws, bufs, B):
    for name, act, C in (("bits1", ws.a1, 32), ("bits2", ws.a2, 64), ("bits3", ws.a3.view(B, 49, 64), 64)):
        got = _unpack(getattr(ws, name), C)
        assert torch.equal(got, act > 0), name
        big = bufs[name]
        assert bool((big[:PAD] == SENTINEL).all()) and bool((big[-PAD:] == SENTINEL).all()), name
    # the cases the biases are built for: zero words, and stored activations that are exactly 0
    assert bool((ws.bits1 == 0).any()) and bool((ws.bits2[:, :, 1] == 0).all()) and bool((ws.bits3[:, :, 0] == 0).all())
    assert bool((ws.bits1 != 0).any()) and bool((ws.bits2[:, :, 0] != 0).any()) and bool((ws.bits3[:, :, 1] != 0).any())
    assert bool((ws.a1 == 0).any()) and bool((ws.a2 == 0).any()) and bool((ws.a3 == 0).any())


# B = 1; 70: ragged inside a 128-row tile, tiles crossing sample boundaries; 130: two tiles of
# FC1 rows and a 2-row tail
@pytest.mark.parametrize("B", [1, 70, 130])
def test_forward_bits_equal_activation_sign(cuda, B):
    from apex_amd.models.fused_f32 import F32DuelingNet, F32Workspace, forward_multi_f32

    net = F32DuelingNet(_model(cuda))
    x = _frames(B, cuda)
    ws = F32Workspace(B, 18, cuda, keep_for_backward=True)
    bufs = _padded_bits(ws)
    forward_multi_f32([(net, x, ws, None, None)], sign_bits=True)
    torch.cuda.synchronize()
    assert ws.bits_valid
    _check_bits(ws, bufs, B)


def test_forward_bits_learner_sized_tiles(cuda):
    """3 x 342 = 1026 rows: the learner-sized forward tiles (conv2 128 x 64, conv3 64 x 64); only
    problem 0 writes bits."""
    from apex_amd.models.fused_f32 import F32DuelingNet, F32Workspace, forward_multi_f32

    B = 342
    net = F32DuelingNet(_model(cuda))
    wss = [F32Workspace(B, 18, cuda, keep_for_backward=(k == 0)) for k in range(3)]
    bufs = _padded_bits(wss[0])
    xs = [_frames(B, cuda, seed=k + 1) for k in range(3)]
    forward_multi_f32([(net, xs[k], wss[k], None, None) for k in range(3)], sign_bits=True)
    torch.cuda.synchronize()
    assert wss[0].bits_valid and not wss[1].bits_valid and not wss[2].bits_valid
    _check_bits(wss[0], bufs, B)


def _backward(net, x, ws):
    """FC1 + conv backward from ws.dz; every input gradient and weight-gradient partial."""
    for t in (ws.dy3, ws.dy2, ws.dy1, net._fc1_ws, *net._wgrad_wss):
        t.fill_(12345.0)  # (stale results of the other path would compare equal)
    net._fc1_bwd(ws)
    net._conv_chain(x, ws, None, None)
    torch.cuda.synchronize()
    return [t.clone() for t in (ws.dy3, ws.dy2, ws.dy1, net._fc1_ws, *net._wgrad_wss)]


@pytest.mark.parametrize("B", [1, 70, 130])
def test_backward_identical_with_bits_and_fp32_masks(cuda, B):
    from apex_amd import ops
    from apex_amd.models.fused_f32 import F32DuelingNet, F32Workspace, forward_multi_f32

    hip = ops.hip()
    net = F32DuelingNet(_model(cuda))
    net.enable_backward(B)
    for p in net.model.parameters():  # (the finalize jobs the launchers return name the .grad views)
        p.grad = torch.zeros_like(p)
    x = _frames(B, cuda)
    ws = F32Workspace(B, 18, cuda, keep_for_backward=True)
    ws.dz.copy_(torch.randn(B, 256, device=cuda, generator=torch.Generator(device=cuda).manual_seed(7)))
    prev = hip.f32_batch_resolve()
    try:
        hip.f32_set_batch_resolve(3)
        forward_multi_f32([(net, x, ws, None, None)], sign_bits=True)
        assert ws.bits_valid
        with_bits = _backward(net, x, ws)
        hip.f32_set_batch_resolve(0)  # the knob: the same forward writes no bits, the fp32 masks are read
        for t in (ws.bits1, ws.bits2, ws.bits3):
            t.fill_(SENTINEL)
        forward_multi_f32([(net, x, ws, None, None)], sign_bits=True)
        assert not ws.bits_valid
        with_masks = _backward(net, x, ws)
        assert all(bool((t == SENTINEL).all()) for t in (ws.bits1, ws.bits2, ws.bits3))
    finally:
        hip.f32_set_batch_resolve(prev)
    names = ("dy3", "dy2", "dy1", "fc1 partials", "conv1 partials", "conv2 partials", "conv3 partials")
    for name, a, b in zip(names, with_bits, with_masks):
        assert torch.equal(a, b), name
    assert bool((with_bits[0] == 0).any()) and bool((with_bits[0] != 0).any())  # the mask masks


def test_captured_learner_steps_identical_with_knobs_on_and_off(cuda):
    """Three captured learner steps at B = 96 on a 128-leaf replay, sign bits + compact rows on
    (mask 3) and off (mask 0): the same parameters, gradient, loss, batch, IS weights, priorities."""
    from apex_amd import ops
    from apex_amd.engine.apex import ApexEngine, EngineConfig
    from apex_amd.engine.learner import LearnerConfig

    hip = ops.hip()
    prev = hip.f32_batch_resolve()
    engs = []
    try:
        for mask in (3, 0):
            hip.f32_set_batch_resolve(mask)  # read when the step is traced (the graphs keep their pointers)
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
        hip.f32_set_batch_resolve(prev)
    la, lb = (e.learner for e in engs)
    assert la.draws_in_conv1 and lb.draws_in_conv1
    assert la.ws_s.bits_valid and la.batch_rows and not lb.ws_s.bits_valid and not lb.batch_rows
    for name in ("flat", "flat_grad", "loss", "idx", "w", "prio", "step_counter"):
        assert torch.equal(getattr(la, name), getattr(lb, name)), name
    assert torch.isfinite(la.flat).all() and la.idx.unique().numel() > 8
