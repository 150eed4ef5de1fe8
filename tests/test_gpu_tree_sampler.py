"""The PER sampler (``per_sample_k`` / ``tree_sample_leaf``) against the exact host model of
``tests/tree_oracle.py``: every drawn leaf must equal the model's, row for row, on ragged trees,
at every fill level that moves the excluded slot, with and without ``exclude_last``.

Exactness: the node sums are compared bit for bit and the model descends over sums rebuilt from
the device's own leaves.  That is valid only while fp64 sums of the fp32 leaves are exact in any
order -- log2(C) + log2(max leaf / min positive leaf) + 25 <= 53 -- which every test asserts on the
leaves it read back before relying on it."""
import numpy as np
import pytest
import torch

from . import tree_oracle as to

pytestmark = pytest.mark.gpu

SEED = (0xB5AD << 32) | 0x4ECE1F35          # 48 bits: the high key word is in play
CTRS = ((1 << 32) + 7, (2 << 32) + 8)       # above 2^32; two of them, so a stuck counter shows


def _replay(cuda, C, alpha=1.0):
    from apex_amd.engine.hbm_replay import HBMReplay

    return HBMReplay(C, n_envs=1, device=cuda, alpha=alpha, frame_capacity=4, seed=SEED)  # the tree only


def _load(rp, prio, exact=True):
    """Writes every leaf, reads the tree back and checks every node against the device's own
    leaves: (leaves, model sums, model mins)."""
    C = rp.capacity
    dev = rp.device
    rp.write_priorities(torch.arange(C, dtype=torch.int32, device=dev), torch.from_numpy(prio).to(dev), dedup=False)
    torch.cuda.synchronize()
    leaf = rp.leaf_sum.cpu().numpy()
    sums, mins = to.build(leaf, rp.leaf_min.cpu().numpy())
    assert len(rp.node_sum) == len(sums) - 1
    if exact:
        assert to.exact_sum_bits(leaf) <= 53
    for k, (s, m) in enumerate(zip(rp.node_sum, rp.node_min)):
        if exact:
            assert np.array_equal(s.cpu().numpy(), sums[k + 1]), k
        else:
            np.testing.assert_allclose(s.cpu().numpy(), sums[k + 1], rtol=1e-12, atol=1e-9)
        assert np.array_equal(m.cpu().numpy(), mins[k + 1]), k
    return leaf, sums, mins


def _draw(rp, B, filled, excl, ctr, beta, **kw):
    dev = rp.device
    rp.filled.fill_(filled)
    out_i = torch.full((B,), -7, dtype=torch.int32, device=dev)
    out_w = torch.full((B,), -7.0, dtype=torch.float32, device=dev)
    counter = torch.tensor([ctr], dtype=torch.int64, device=dev)
    rp.sample_indices(B, out_i, out_w, counter, beta=beta, exclude_last=bool(excl), **kw)
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_w.cpu().numpy()


def _model(sums, sizes, B, filled, excl, ctr):
    rows = [to.sample(sums, sizes, i, B, filled, excl, SEED, ctr) for i in range(B)]
    assert not any(fb for _, _, fb in rows)
    return np.array([n for n, _, _ in rows]), np.array([v for _, v, _ in rows])


@pytest.mark.parametrize("C", to.SAMPLER_CAPACITIES)
def test_draws_equal_the_host_model(cuda, C):
    rp = _replay(cuda, C)
    sizes = to.level_sizes(C)
    assert sizes == rp.level_sizes
    beta_dev = torch.tensor([0.7], dtype=torch.float32, device=cuda)
    cases = 0
    for filled in to.sampler_fills(C):
        length = min(filled, C)
        leaf, sums, mins = _load(rp, to.sampler_leaves(C, length))
        assert not leaf[length:].any()
        pmin = float(mins[-1][0])  # the root min: it includes the excluded leaf
        for excl in (0, 1):
            rest = float(sums[-1][0]) - (float(leaf[length - 1]) if excl and length > 0 else 0.0)
            if length < 1 + excl or rest <= 0.0:
                continue
            for B in to.SAMPLER_BATCHES:
                for ctr, beta in zip(CTRS, (0.4, beta_dev)):
                    idx, w = _draw(rp, B, filled, excl, ctr, beta)
                    want, value = _model(sums, sizes, B, filled, excl, ctr)
                    assert np.array_equal(idx, want), (C, filled, excl, B, ctr)
                    assert (leaf[idx] > 0).all() and (idx < length).all()
                    assert not (excl and (idx == length - 1).any())
                    b = 0.4 if ctr == CTRS[0] else float(np.float32(0.7))
                    ww = [to.is_weight(v, pmin, 1.0, b) for v in value]
                    np.testing.assert_allclose(w, ww, rtol=1e-5, atol=0)
                    cases += 1
    assert cases > 0


def test_the_two_counters_draw_differently(cuda):
    """The model's own draws differ between the counters and between seeds that differ above bit
    32: a sampler that ignored either could not match both."""
    C, B = 4097, 64
    sums, sizes = to.build(to.sampler_leaves(C, C))[0], to.level_sizes(C)
    a = [to.sample(sums, sizes, i, B, C, 0, SEED, CTRS[0])[0] for i in range(B)]
    assert a != [to.sample(sums, sizes, i, B, C, 0, SEED, CTRS[1])[0] for i in range(B)]
    assert a != [to.sample(sums, sizes, i, B, C, 0, SEED, CTRS[0] & 0xFFFFFFFF)[0] for i in range(B)]
    assert a != [to.sample(sums, sizes, i, B, C, 0, SEED & 0xFFFFFFFF, CTRS[0])[0] for i in range(B)]
    rp = _replay(cuda, C)
    _load(rp, to.sampler_leaves(C, C))
    idx, _ = _draw(rp, B, C, 0, CTRS[0], 0.4)
    assert np.array_equal(idx, a)
    idx, _ = _draw(rp, B, C, 0, CTRS[0], 0.4, seed=SEED & 0xFFFFFFFF)
    assert np.array_equal(idx, [to.sample(sums, sizes, i, B, C, 0, SEED & 0xFFFFFFFF, CTRS[0])[0] for i in range(B)])


def test_weights_with_a_global_pair_and_with_shard_slots(cuda):
    """``glob`` = (global min priority, weight scale) and ``shard`` = (slots, world 3, rank 1)
    change the weights only: they follow the model's formula, the draws stay the model's."""
    C, B, filled, excl = 4097, 64, 4097, 1
    rp = _replay(cuda, C)
    leaf, sums, mins = _load(rp, to.sampler_leaves(C, filled))
    want, value = _model(sums, to.level_sizes(C), B, filled, excl, CTRS[0])
    glob = torch.tensor([0.25, 2.5], dtype=torch.float32, device=cuda)
    idx, w = _draw(rp, B, filled, excl, CTRS[0], 0.4, glob=glob)
    assert np.array_equal(idx, want)
    np.testing.assert_allclose(w, [to.is_weight(v, 0.25, 2.5, 0.4) for v in value], rtol=1e-5, atol=0)
    slots = np.array([[1000.5, 3.0], [np.float32(sums[-1][0]), mins[-1][0]], [333.25, 0.75]], np.float32)
    pmin, wscale = to.shard_glob(slots, 3, 1)
    assert pmin == 0.75 and 0 < wscale < 3
    idx, w = _draw(rp, B, filled, excl, CTRS[0], 0.4, shard=(torch.from_numpy(slots).to(cuda), 3, 1))
    assert np.array_equal(idx, want)
    np.testing.assert_allclose(w, [to.is_weight(v, pmin, wscale, 0.4) for v in value], rtol=1e-5, atol=0)
    packed = torch.full((6,), -1.0, dtype=torch.float32, device=cuda)
    rp.pack_shard_slots(packed, 3, 1)
    assert packed.cpu().tolist() == [0.0, 0.0, float(slots[1, 0]), float(slots[1, 1]), 0.0, 0.0]


def test_wide_range_sums_within_the_trees_own_tolerance(cuda):
    """Priorities over a range of 2^40: the sums are no longer exact in any order, so only they
    are compared (rtol 1e-12, atol 1e-9), not the draws."""
    C = 4097
    rng = np.random.default_rng(5)
    prio = (2.0 ** rng.uniform(-20.0, 20.0, size=C)).astype(np.float32)
    prio[rng.random(C) < 0.2] = 0.0
    rp = _replay(cuda, C)
    leaf, _, _ = _load(rp, prio, exact=False)
    assert to.exact_sum_bits(leaf) > 53 and leaf.max() / leaf[leaf > 0].min() > 2.0 ** 38


def _regions(C, C_r, filled, behind):
    """Two regions of C_r slots in a tree of C, the first holding ``filled`` rows, the second ``behind``."""
    rng = np.random.default_rng(C)
    prio = np.zeros(C, np.float32)
    prio[:filled] = rng.integers(1, 256, size=filled)
    prio[C_r:C_r + behind] = rng.integers(1, 256, size=behind) * (64 if behind == 1 else 1)
    return prio


@pytest.mark.parametrize("C,C_r,filled,behind", [(65, 64, 64, 1), (4200, 2100, 1000, 900), (4200, 2100, 1985, 2100)])
def test_exclusion_with_live_mass_behind_the_excluded_slot(cuda, C, C_r, filled, behind):
    """The central learner's layout: region r at (r - 1) C_r and one fill counter for all of them,
    so slot ``filled - 1`` lies inside the first region with live mass behind it in the second.
    The excluded leaf must leave the mass at every level, not only the total and the leaf level:
    every draw equals a brute-force cumulative search over the leaves with that slot removed.
    (The descent that kept its mass in the upper levels shifted every draw aimed past it, and at
    a node edge returned the slot before it.)"""
    prio = _regions(C, C_r, filled, behind)
    rp = _replay(cuda, C)
    leaf, sums, _ = _load(rp, prio)
    assert leaf[filled - 1] > 0 and leaf[filled:].sum() > 0
    cum = to.brute_force_cum(leaf, filled, 1)
    past = 0
    for B in (3, 64, 257):
        for ctr in CTRS:
            idx, _ = _draw(rp, B, filled, 1, ctr, 0.4)
            want = [to.brute_force_draw(cum, i, B, SEED, ctr) for i in range(B)]
            assert np.array_equal(idx, want), (B, ctr)
            assert np.array_equal(idx, _model(sums, to.level_sizes(C), B, filled, 1, ctr)[0])
            assert (idx != filled - 1).all()
            past += int((idx >= C_r).sum())
    assert past > 0
