"""The drawn batch's compact rows: the PER draw folded into the conv1 forward also writes the
batch's frame ids of s and its (action, reward, done) in row order -- a drawn slot that the same
launch scatters is taken from its staging row, exactly as the frame ids are -- so the conv1 weight
gradient and the loss launch read row b directly instead of through idx and the replay tables."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_compact_rows_equal_table_rows_at_drawn_slots(cuda):
    """Overlapped engine, actor rows staged every step (the pattern of
    test_conv1_draw_equals_sampling_launch): 64 envs x 40 steps > the 2048 free slots of the 4096
    ring, so staged rows overwrite drawn slots of the very launch that draws them."""
    from apex_amd import ops
    from apex_amd.engine.apex import ApexEngine, EngineConfig
    from apex_amd.engine.learner import LearnerConfig

    hip = ops.hip()
    prev = hip.f32_batch_resolve()
    hip.f32_set_batch_resolve(3)  # read when the step is traced (the graphs keep their pointers)
    try:
        _compact_rows_check(cuda, ApexEngine, EngineConfig, LearnerConfig)
    finally:
        hip.f32_set_batch_resolve(prev)


def _compact_rows_check(cuda, ApexEngine, EngineConfig, LearnerConfig):
    cfg = EngineConfig(n_envs=64, replay_capacity=4096, threshold_size=2048, overlap=True, use_graphs=True,
                       publish_param_interval=4, target_update_interval=6,
                       learner=LearnerConfig(batch_size=256, forward="hip"))
    torch.manual_seed(0)
    eng = ApexEngine(cfg, cuda)
    eng.fill()
    eng.capture()
    L, rp = eng.learner, eng.replay
    assert L.draws_in_conv1 and L.batch_rows
    overwritten = 0
    for _ in range(40):
        torch.cuda.synchronize()
        before = rp.s_ids.clone()
        eng.train_step()
        torch.cuda.synchronize()  # the tables now hold this step's scattered rows, not yet the next step's
        idx = L.idx.long()
        assert torch.equal(L.batch_fid, rp.s_ids[idx])
        assert torch.equal(L.a, rp.action[idx])
        assert torch.equal(L.r, rp.reward[idx])
        assert torch.equal(L.d, rp.done[idx])
        changed = (before != rp.s_ids).any(1)  # slots this step's launch scattered (frame ids never repeat)
        overwritten += int(changed[idx].sum())
    assert overwritten > 0  # drawn slots were overwritten by the launch that drew them
    assert L.idx.unique().numel() > L.B // 2


# B = 2; 3: the odd tail of the 2-sample workgroups; 96
@pytest.mark.parametrize("B", [2, 3, 96])
def test_conv1_wgrad_and_loss_identical_with_compact_rows(cuda, B):
    from apex_amd import ops

    hip = ops.hip()
    g = torch.Generator(device=cuda).manual_seed(B)
    s = torch.cuda.current_stream().cuda_stream
    C, F, A = 300, 500, 18
    frames = torch.randint(0, 256, (F, 84 * 84), dtype=torch.uint8, device=cuda, generator=g)
    ids = torch.randint(0, F, (C, 4), dtype=torch.int32, device=cuda, generator=g)
    idx = torch.randint(0, C, (B,), dtype=torch.int32, device=cuda, generator=g)
    fid = ids[idx.long()].contiguous()
    # conv1 weight-gradient partials (+ bias partials)
    dy1 = torch.randn(B, 400, 32, device=cuda, generator=g)
    n = hip.f32_wgrad_workspace_floats(1, B)
    outs = []
    for kw in ({}, {"batch_fid": fid.data_ptr()}):
        ws = torch.full((n,), 12345.0, device=cuda)
        hip.f32_conv_bwd(1, frames.data_ptr(), ids.data_ptr(), idx.data_ptr(), dy1.data_ptr(), 0, 0, 0, ws.data_ptr(),
                         B, s, **kw)
        outs.append(ws)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0] != 12345.0).any())
    # the loss launch: (a, r, d) through idx from the tables, or row b of the compact arrays
    act = torch.randint(0, A, (C,), dtype=torch.int32, device=cuda, generator=g)
    rew = torch.randn(C, device=cuda, generator=g)
    done = (torch.rand(C, device=cuda, generator=g) < 0.3).float()
    q, q2, q2t = (torch.randn(B, A, device=cuda, generator=g) for _ in range(3))
    w = torch.rand(B, device=cuda, generator=g)
    h = torch.randn(B, 256, device=cuda, generator=g).relu()
    w_adv2 = torch.randn(A, 128, device=cuda, generator=g)
    w_val2 = torch.randn(128, device=cuda, generator=g)
    step = torch.zeros(1, dtype=torch.int64, device=cuda)
    blocks = hip.dqn_heads_bwd_blocks(B)
    res = []
    for a_, r_, d_, i_ in ((act, rew, done, idx.data_ptr()),
                           (act[idx.long()].contiguous(), rew[idx.long()].contiguous(), done[idx.long()].contiguous(), 0)):
        out = {"delta": torch.full((B,), 12345.0, device=cuda), "lw": torch.full((B,), 12345.0, device=cuda),
               "dz": torch.full((B, 256), 12345.0, device=cuda),
               "part": torch.full((blocks * ((A + 1) * 128 + (A + 1) + 256),), 12345.0, device=cuda)}
        hip.dqn_heads_bwd({"q": q.data_ptr(), "q2": q2.data_ptr(), "q2t": q2t.data_ptr(), "act": a_.data_ptr(),
                           "rew": r_.data_ptr(), "done": d_.data_ptr(), "idx": i_, "w": w.data_ptr(),
                           "h": h.data_ptr(), "w_adv2": w_adv2.data_ptr(), "w_val2": w_val2.data_ptr(),
                           "step": step.data_ptr(), **{k: v.data_ptr() for k, v in out.items()}}, B, A, 0.97, s)
        res.append(out)
    torch.cuda.synchronize()
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    assert bool((res[0]["delta"] != 12345.0).all())
