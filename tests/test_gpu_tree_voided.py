"""A slot voided by an actor row that emitted nothing (raw priority 0) stays voided when the same
tree launch also carries a learner priority for it: the learner may have drawn the slot while the
tree still held its old priority, and its leaf must not re-arm the old row."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _replay(cuda, capacity=4096, E=64):
    from apex_amd.engine.hbm_replay import HBMReplay

    rp = HBMReplay(capacity, E, device=cuda)
    slots = torch.arange(capacity, dtype=torch.int32, device=cuda)
    for s0 in range(0, capacity, 1024):   # every slot armed with priority 1
        rp.write_priorities(slots[s0:s0 + 1024], torch.ones(1024, device=cuda), dedup=True)
    return rp


def test_learner_leaf_does_not_rearm_a_voided_slot(cuda):
    rp = _replay(cuda)
    E, B = 64, 256
    pre_slots = torch.arange(128, 128 + E, dtype=torch.int32, device=cuda)
    pre_prio = torch.full((E,), 2.0, device=cuda)
    voided = torch.tensor([3, 17, 40, 63], device=cuda)
    pre_prio[voided] = 0.0
    g = torch.Generator(device="cpu").manual_seed(3)
    idx = torch.randint(0, 4096, (B,), generator=g).to(torch.int32).to(cuda)
    idx[:8] = torch.tensor([131, 131, 145, 168, 191, 130, 150, 129], dtype=torch.int32)  # 131, 145, 168, 191 are voided
    prio = torch.full((B,), 5.0, device=cuda)
    rp.write_batch(pre=(pre_slots, pre_prio, rp.filled), idx=idx, prio=prio)
    torch.cuda.synchronize()
    leaf = rp.leaf_sum.cpu()
    a = rp.alpha
    for e in range(E):
        slot = 128 + e
        if e in voided.tolist():
            assert leaf[slot] == 0 and torch.isinf(rp.leaf_min[slot]), slot
        elif slot in idx.tolist():
            assert leaf[slot] == pytest.approx(5.0 ** a), slot     # an emitted slot: the learner's leaf lands last
        else:
            assert leaf[slot] == pytest.approx(2.0 ** a), slot
    other = [int(i) for i in idx.tolist() if not 128 <= i < 128 + E]
    assert all(leaf[i] == pytest.approx(5.0 ** a) for i in other)
    assert bool((rp.owner == -1).all())                            # every claim released
    assert float(rp.node_sum[-1][0]) == pytest.approx(float(rp.leaf_sum.double().sum()), rel=1e-9)
    assert int(rp.filled.item()) == E
