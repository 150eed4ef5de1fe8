"""The host model of the priority tree (``tests/tree_oracle.py``) checked on its own: the level
layout against the engine's, the Philox double against Random123's known answers, the scan and the
descent against ``np.cumsum``, and the writers' rules on hand-written cases.  No GPU: these pin the
oracle that ``test_gpu_tree_sampler.py`` and ``test_gpu_tree_writers.py`` compare the kernels with."""
import math

import numpy as np
import pytest

from . import tree_oracle as to

SEED = (0xB5AD << 32) | 0x4ECE1F35  # a 48-bit seed: the high key word is in play
CTRS = ((1 << 32) + 7, (2 << 32) + 8)


# ------------------------------------------------------------------ layout, nodes, RNG, scan
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 4095, 4096, 4097, 5000, 262144, 262145, 2_000_000, 1 << 24])
def test_level_sizes_equal_the_engines(C):
    from apex_amd.engine.hbm_replay import tree_level_sizes

    assert to.level_sizes(C) == tree_level_sizes(C)


def test_level_sizes_of_the_ragged_capacities():
    assert to.level_sizes(1) == [1, 1]
    assert to.level_sizes(65) == [65, 2, 1]
    assert to.level_sizes(4097) == [4097, 65, 2, 1]
    assert to.level_sizes(262145) == [262145, 4097, 65, 2, 1]


def test_build_sums_and_mins():
    rng = np.random.default_rng(0)
    leaf = rng.integers(0, 50, size=4097).astype(np.float32)
    sums, mins = to.build(leaf)
    assert [len(s) for s in sums] == to.level_sizes(4097) and sums[1].dtype == np.float64
    assert mins[1].dtype == np.float32
    for n in range(65):
        kids = leaf[64 * n:64 * n + 64]
        assert sums[1][n] == kids.astype(np.float64).sum()
        assert mins[1][n] == (kids[kids > 0].min() if (kids > 0).any() else np.inf)
    assert sums[2][1] == leaf[4096] and sums[3][0] == leaf.astype(np.float64).sum()
    assert mins[3][0] == leaf[leaf > 0].min()
    # an explicit min array is reduced as given
    _, m2 = to.build(leaf, np.full(4097, 3.0, np.float32))
    assert (m2[1] == 3.0).all() and m2[3][0] == 3.0


def test_exact_sum_bits():
    assert to.exact_sum_bits(np.zeros(5, np.float32)) == 0
    assert to.exact_sum_bits(np.array([1.0, 1.5], np.float32)) == 1 + 0 + 25
    assert to.exact_sum_bits(np.array([1.0, 255.0, 0.0], np.float32)) == 2 + 7 + 25
    for C in to.SAMPLER_CAPACITIES:
        assert to.exact_sum_bits(to.sampler_leaves(C, C)) <= 51


@pytest.mark.parametrize("ctr,key,x,y", [
    ((0, 0, 0, 0), (0, 0), 0x6627E8D5, 0xE169C58D),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, 0x408F276D, 0x41C83B0E),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), 0xD16CFE09, 0x94FDCCEB),
])
def test_uniform_double_from_the_random123_known_answers(ctr, key, x, y):
    """Words 0 and 1 of the known answers, packed as common.h packs them."""
    seed, stream, counter = (key[1] << 32) | key[0], (ctr[3] << 32) | ctr[2], (ctr[1] << 32) | ctr[0]
    want = (((x << 21) ^ y) & ((1 << 53) - 1)) * 2.0 ** -53
    got = to.uniform_double(seed, stream, counter)
    assert got == want and 0.0 <= got < 1.0


def test_uniform_double_uses_every_high_word():
    base = to.uniform_double(3, 5, 7)
    assert base != to.uniform_double(3 + 2 ** 33, 5, 7)
    assert base != to.uniform_double(3, 5 + 2 ** 32, 7)
    assert base != to.uniform_double(3, 5, 7 + 2 ** 32)
    us = np.array([to.uniform_double(SEED, s, CTRS[0]) for s in range(2000)])
    assert us.min() >= 0.0 and us.max() < 1.0 and abs(us.mean() - 0.5) < 0.03


def test_hillis_steele_equals_cumsum_on_integers():
    rng = np.random.default_rng(1)
    for _ in range(20):
        v = rng.integers(0, 1 << 30, size=64).astype(np.float64)
        assert (to.hillis_steele(v) == np.cumsum(v)).all()
    v = np.arange(64, dtype=np.float64)
    to.hillis_steele(v)
    assert (v == np.arange(64)).all()  # the input is left alone


# ------------------------------------------------------------------ the descent
@pytest.mark.parametrize("C", to.SAMPLER_CAPACITIES)
def test_sample_equals_the_brute_force_cumulative_search(C):
    """Every capacity, fill level, exclusion and batch size of the GPU test, on exact-sum inputs:
    the descent lands on the leaf np.searchsorted finds, with no fallback taken."""
    sizes = to.level_sizes(C)
    drawn = 0
    for filled in to.sampler_fills(C):
        length = min(filled, C)
        leaf = to.sampler_leaves(C, length)
        assert to.exact_sum_bits(leaf) <= 53
        sums, _ = to.build(leaf)
        for excl in (0, 1):
            rest = float(sums[-1][0]) - (float(leaf[length - 1]) if excl and length > 0 else 0.0)
            if length < 1 + excl or rest <= 0.0:
                continue
            cum = to.brute_force_cum(leaf, filled, excl)
            for B in to.SAMPLER_BATCHES:
                for ctr in CTRS:
                    for i in range(B):
                        node, value, fb = to.sample(sums, sizes, i, B, filled, excl, SEED, ctr)
                        want = to.brute_force_draw(cum, i, B, SEED, ctr)
                        assert (node, fb) == (want, False), (C, filled, excl, B, i)
                        assert value == leaf[node] and value > 0 and node < length
                        assert not (excl and node == length - 1)
                        drawn += 1
    assert drawn > 0


def test_sample_is_stratified():
    C, B = 4097, 64
    leaf = to.sampler_leaves(C, C)
    sums, _ = to.build(leaf)
    cum = np.cumsum(leaf.astype(np.float64))
    for i in range(B):
        node, _, _ = to.sample(sums, to.level_sizes(C), i, B, C, 0, SEED, CTRS[0])
        lo, hi = (cum[node - 1] if node else 0.0), cum[node]
        assert hi > i * cum[-1] / B and lo < (i + 1) * cum[-1] / B


def _violation_case():
    """Capacity 65, 64 slots counted as filled, live mass at slot 64: behind the excluded slot 63."""
    leaf = np.zeros(65, np.float32)
    leaf[:64] = 1.0
    leaf[64] = 64.0
    return leaf, to.build(leaf)[0], to.level_sizes(65)


def test_exclusion_with_live_mass_behind_the_excluded_slot():
    """The precondition the earlier descent relied on, broken: the excluded leaf's mass stayed in
    its ancestor, so draws aimed past it entered the wrong node and took the fallback there.  It
    is the model's one deterministic route into the fallback branch."""
    leaf, sums, sizes = _violation_case()
    B = 127  # strata of one unit of mass: draws 63.. are aimed at slot 64
    old = [to.sample(sums, sizes, i, B, 64, 1, SEED, CTRS[0], consistent=False) for i in range(B)]
    new = [to.sample(sums, sizes, i, B, 64, 1, SEED, CTRS[0]) for i in range(B)]
    cum = to.brute_force_cum(leaf, 64, 1)
    want = [to.brute_force_draw(cum, i, B, SEED, CTRS[0]) for i in range(B)]
    assert want == list(range(63)) + [64] * 64
    assert [n for n, _, _ in new] == want and not any(fb for _, _, fb in new)
    # the first draw meant for slot 64 lies within the excluded leaf's mass of the old node sum
    assert old[63][0] == 62 and old[63][2]
    assert [n for n, _, _ in old[:63] + old[64:]] == want[:63] + want[64:]
    assert not any(fb for _, _, fb in old[:63] + old[64:])


def test_descents_agree_where_nothing_lives_behind_the_excluded_slot():
    for C in (65, 4097):
        for filled in to.sampler_fills(C):
            length = min(filled, C)
            leaf = to.sampler_leaves(C, length)
            sums, sizes = to.build(leaf)[0], to.level_sizes(C)
            for i in range(64):
                a = to.sample(sums, sizes, i, 64, filled, 1, SEED, CTRS[1])
                assert a == to.sample(sums, sizes, i, 64, filled, 1, SEED, CTRS[1], consistent=False)


def test_is_weight():
    assert to.is_weight(4.0, 1.0, 1.0, 0.5) == 0.5
    assert to.is_weight(4.0, 1.0, 3.0, 0.5) == 1.5
    assert to.is_weight(0.0, 1.0, 3.0, 0.5) == 3.0          # a massless leaf
    assert to.is_weight(4.0, math.inf, 3.0, 0.5) == 3.0     # an empty tree's min
    assert to.is_weight(4.0, 0.0, 3.0, 0.5) == 3.0
    pmin, ws = to.shard_glob(np.array([[2.0, 0.5], [6.0, 0.25], [4.0, 1.0]], np.float32), 3, 1)
    assert pmin == 0.25 and ws == 1.5


# ------------------------------------------------------------------ the writers
def test_prio_mix_rounds_every_step_in_fp32():
    d = np.array([0.3, 1.7, 0.0], np.float32)
    got = to.prio_mix(d)
    f = np.float32
    want = [f(f(f(f(0.9) * f(1.7)) + f(f(0.1) * x)) + f(1e-6)) for x in d]
    assert got.dtype == np.float32 and list(got) == want


def test_writer_last_write_wins():
    m = to.TreeModel(100, 0.5)
    m.write_priorities([5, 7, 5, 5, -1, 100], np.array([4.0, 9.0, 16.0, 25.0, 36.0, 49.0], np.float32), dedup=True)
    assert m.leaf_sum[5] == 5.0 and m.leaf_min[5] == 5.0 and m.leaf_sum[7] == 3.0
    assert m.leaf_sum.sum() == 8.0                      # -1 and C are skipped
    assert m.max_prio == 25.0                           # the winners' raw priorities: not 36 or 49
    m.write_priorities([1, 2, 3], np.array([1.0, 4.0, 100.0], np.float32), dedup=False, bumps=(3, 1))
    assert list(m.leaf_sum[1:4]) == [1.0, 2.0, 10.0] and m.max_prio == 100.0
    assert (m.filled, m.bump) == (3, 1)
    b = to.TreeModel(100, 1.0)
    b.write_batch(idx=[9, 9, 9, 4], prio=np.array([1.0, 2.0, 3.0, 4.0], np.float32))
    assert b.leaf_sum[9] == 3.0 and b.leaf_sum[4] == 4.0 and b.max_prio == 4.0


def test_writer_invalid_priorities_void():
    m = to.TreeModel(10, 1.0)
    m.write_priorities(np.arange(10), np.full(10, 2.0, np.float32), dedup=False)
    m.write_priorities([0, 1, 2, 3, 4], np.array([0.0, -1.0, np.nan, np.inf, 3.0], np.float32), dedup=True)
    assert list(m.leaf_sum[:5]) == [0.0, 0.0, 0.0, 0.0, 3.0] and np.isinf(m.leaf_min[:4]).all()
    assert m.leaf_min[4] == 3.0 and m.max_prio == 3.0   # inf never becomes the running max


def test_writer_void_beats_learner():
    m = to.TreeModel(64, 1.0)
    m.write_priorities(np.arange(64), np.full(64, 2.0, np.float32), dedup=False)
    pre = (np.array([10, 11, 12, 13, -1]), np.array([3.0, 0.0, np.nan, np.inf, 7.0], np.float32))
    m.write_batch(pre=pre, idx=[10, 11, 12, 13, 11], prio=np.full(5, 5.0, np.float32))
    assert m.leaf_sum[10] == 5.0                        # a learner leaf lands after an emitted actor leaf
    assert m.leaf_sum[11] == 0.0 and m.leaf_sum[12] == 0.0 and np.isinf(m.leaf_min[11])  # voided: stays voided
    assert m.leaf_sum[13] == 5.0                        # +inf is > 0: an invalid leaf, but no void claim
    assert (m.filled, m.bump) == (5, 1) and m.max_prio == 5.0
    assert (m.owner == -1).all() and m.ticket == 0


def test_writer_max_priority_rule():
    m = to.TreeModel(64, 0.6)
    m.write_batch(pre=(np.array([1, 2]), np.array([9.0, 0.0], np.float32)))
    assert m.max_prio == 9.0                            # actor rows always count
    m.write_batch(idx=[3, 4])                           # prio=None: the current max, which does not move
    assert m.leaf_sum[3] == 9.0 ** 0.6 and m.max_prio == 9.0 and m.bump == 2
    m.write_batch(idx=[5, 5], prio=np.array([50.0, 20.0], np.float32))
    assert m.max_prio == 20.0                           # the loser's 50 is never written
    m.write_batch(idx=[6, 7], mix=(np.array([30.0, 1.0], np.float32), np.array([2.0, 4.0], np.float32)))
    assert m.loss_out == 3.0 and list(m.prio_out) == list(to.prio_mix([30.0, 1.0]))
    assert m.max_prio == m.prio_out.max() and m.max_prio.dtype == np.float32
    m.write_priorities([8], None, dedup=True)
    assert m.leaf_sum[8] == float(m.max_prio) ** 0.6
