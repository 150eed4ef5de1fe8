"""Host model of the fanout-64 priority tree (``ops/csrc/tree_dev.h``, ``replay_kernels.hip``,
``tree_sample_leaf`` in ``common.h``): the level layout, the fp64 node sums / fp32 node mins, the
Philox-driven stratified descent with its 64-wide Hillis-Steele scan, the importance weight, and a
sequential model of the three writers (``write_priorities`` sorted / ring, ``write_batch``).
numpy and pure Python only -- no GPU code is imported, so the model is checked on any machine
(``test_tree_oracle_host.py``) before the kernels are compared with it
(``test_gpu_tree_sampler.py``, ``test_gpu_tree_writers.py``)."""
from __future__ import annotations

import math

import numpy as np

from .actor_oracle import philox4x32_10

FANOUT = 64
f32 = np.float32


# ------------------------------------------------------------------ layout and node values
def level_sizes(C):
    """Nodes per level, leaves first; capacity 1 still has one internal level."""
    sizes = [int(C)]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + FANOUT - 1) // FANOUT)
    if len(sizes) == 1:
        sizes.append(1)
    return sizes


def _groups(a, n, pad, dtype):
    out = np.full(n * FANOUT, pad, dtype=dtype)
    out[:len(a)] = a
    return out.reshape(n, FANOUT)


def build(leaf, leaf_min=None):
    """(sums, mins), one array per level with the leaves at index 0: fp64 sums and fp32 mins over
    groups of 64 children, padded with 0 / +inf.  ``leaf_min`` defaults to the writers' rule: the
    leaf's own value where it has mass, +inf where it has none."""
    leaf = np.asarray(leaf, dtype=np.float32)
    if leaf_min is None:
        leaf_min = np.where(leaf > 0, leaf, f32(np.inf)).astype(np.float32)
    sums, mins = [leaf.astype(np.float64)], [np.asarray(leaf_min, dtype=np.float32)]
    for n in level_sizes(len(leaf))[1:]:
        sums.append(_groups(sums[-1], n, 0.0, np.float64).sum(1))
        mins.append(_groups(mins[-1], n, np.inf, np.float32).min(1))
    return sums, mins


def exact_sum_bits(leaf):
    """Bits an exact sum of these fp32 leaves can need: log2(C) + log2(max / min positive) + 25,
    in whole exponents.  While it is <= 53, fp64 sums of the leaves are exact in any order."""
    leaf = np.asarray(leaf, dtype=np.float32)
    pos = leaf[leaf > 0]
    if pos.size == 0:
        return 0
    assert np.isfinite(pos).all()
    e = np.frexp(pos)[1]
    return int(math.ceil(math.log2(max(len(leaf), 1)))) + int(e.max() - e.min()) + 25


# ------------------------------------------------------------------ the draw
def uniform_double(seed, stream, counter):
    """53 random bits of Philox4x32-10 times 2^-53: counter words (counter lo, counter hi,
    stream lo, stream hi), key (seed lo, seed hi), bits = ((x << 21) ^ y) mod 2^53."""
    seed, stream, counter = int(seed), int(stream), int(counter)
    x, y, _, _ = philox4x32_10((counter, counter >> 32, stream, stream >> 32), (seed, seed >> 32))
    bits = ((x << 21) ^ y) & ((1 << 53) - 1)
    return bits * 2.0 ** -53


def hillis_steele(v):
    """Inclusive scan of 64 lanes in the wave's order: offsets 1, 2, 4, .. 32, lane l adds the
    value lane l - o held before the step."""
    v = np.array(v, copy=True)
    assert v.shape == (FANOUT,)
    o = 1
    while o < FANOUT:
        w = v.copy()
        v[o:] = v[o:] + w[:-o]
        o <<= 1
    return v


def sample(levels, sizes, i, B, length, exclude_last, seed, ctr, consistent=True):
    """Stratified draw ``i`` of ``B``: (leaf, its stored value, whether a level took the "no hit"
    fallback).  ``levels``: the sums of :func:`build`.  With ``exclude_last`` the leaf
    ``length - 1`` is left out of the mass: out of the total, and out of the child that holds it at
    every level.  ``consistent=False`` is the earlier descent, which removed it from the total and
    the leaf level only -- right only while no live leaf lies behind slot ``length - 1``."""
    L = len(sizes) - 1
    C = sizes[0]
    length = min(int(length), C)
    excl = bool(exclude_last) and length > 0
    xs = length - 1
    xv = float(levels[0][xs]) if excl else 0.0
    total = float(levels[L][0]) - xv
    u = uniform_double(seed, i, ctr)
    mass = (u + float(i)) * total / float(B)
    node, fallback, value = 0, False, 0.0
    for level in range(L, 0, -1):
        src = levels[level - 1]
        lo = node * FANOUT
        v = np.zeros(FANOUT, dtype=np.float64)
        n = max(0, min(FANOUT, sizes[level - 1] - lo))
        v[:n] = src[lo:lo + n]
        if excl and (consistent or level == 1):
            xc = xs >> (6 * (level - 1))
            if lo <= xc < lo + FANOUT:
                v[xc - lo] = max(v[xc - lo] - xv, 0.0)
        incl = hillis_steele(v)
        hit = np.nonzero(incl > mass)[0]
        if hit.size:
            k = int(hit[0])
        else:
            fallback = True
            nz = np.nonzero(v > 0.0)[0]
            k = int(nz[-1]) if nz.size else 0
        if level == 1:
            value = float(src[lo + k]) if lo + k < sizes[0] else 0.0
        mass = max(mass - (incl[k] - v[k]), 0.0)
        node = lo + k
    return node, value, fallback


def is_weight(p, pmin, wscale, beta):
    """wscale (p / pmin)^-beta in fp64; wscale alone for a massless leaf or a tree without a min."""
    p, pmin, wscale, beta = float(p), float(pmin), float(wscale), float(beta)
    if p > 0.0 and pmin > 0.0 and math.isfinite(pmin):
        return wscale * (p / pmin) ** -beta
    return wscale


def shard_glob(slots, world, rank):
    """(global min priority, this shard's weight scale as fp32) from the exchanged per-shard
    (mass, min priority) fp32 pairs: world * M_rank / sum M."""
    slots = np.asarray(slots, dtype=np.float32).reshape(-1, 2)[:world]
    m = float(slots[:, 0].astype(np.float64).sum())
    return float(slots[:, 1].min()), float(f32(world * float(slots[rank, 0]) / max(m, 1e-300)))


# ------------------------------------------------------------------ the writers
def prio_mix(delta):
    """(0.9f max(delta) + 0.1f delta_i) + 1e-6f, one fp32 rounding per operation (no fma)."""
    delta = np.asarray(delta, dtype=np.float32)
    dmax = delta.max()
    return ((f32(0.9) * dmax + f32(0.1) * delta) + f32(1e-6)).astype(np.float32)


class TreeModel:
    """Sequential model of the writers.  Leaves are kept in fp64 (``p ** alpha`` of the fp32
    priority); a write with ``p <= 0`` or a non-finite ``p`` leaves sum 0 / min +inf."""

    def __init__(self, C, alpha, max_prio=1.0):
        self.C, self.alpha = int(C), float(alpha)
        self.leaf_sum = np.zeros(self.C, dtype=np.float64)
        self.leaf_min = np.full(self.C, np.inf, dtype=np.float64)
        self.max_prio = f32(max_prio)
        self.filled = 0
        self.bump = 0
        self.owner = np.full(self.C, -1, dtype=np.int32)
        self.ticket = 0
        self.prio_out = None
        self.loss_out = None

    @staticmethod
    def valid(p):
        p = float(p)
        return p > 0.0 and math.isfinite(p)

    def _in(self, s):
        return 0 <= int(s) < self.C

    def _write(self, s, p):
        """One leaf; returns the raw priority to fold into the running max (0 if invalid)."""
        if self.valid(p):
            self.leaf_sum[s] = self.leaf_min[s] = float(f32(p)) ** self.alpha
            return f32(p)
        self.leaf_sum[s], self.leaf_min[s] = 0.0, np.inf
        return f32(0.0)

    def _learner_prios(self, B, prio, mix):
        """(fp32 priorities [B], whether they move the running max)."""
        if mix is not None:
            delta, lw = mix
            assert len(delta) == B and len(lw) == B
            self.prio_out = prio_mix(delta)
            self.loss_out = float(np.asarray(lw, dtype=np.float32).astype(np.float64).sum() / B)
            return self.prio_out, True
        if prio is not None:
            assert len(prio) == B
            return np.asarray(prio, dtype=np.float32), True
        return np.full(B, self.max_prio, dtype=np.float32), False

    def write_priorities(self, idx, prio=None, dedup=True, mix=None, bumps=(0, 0)):
        """``bumps``: what the launch adds to (``filled``, ``bump``)."""
        idx = np.asarray(idx, dtype=np.int64)
        B = len(idx)
        if B == 0:
            return
        assert mix is None or dedup
        self.filled += int(bumps[0])
        self.bump += int(bumps[1])
        p, moves = self._learner_prios(B, prio, mix)
        rows = range(B)
        if dedup:  # the last position of each slot wins
            last = {int(s): k for k, s in enumerate(idx)}
            rows = sorted(last.values())
        pmax = f32(0.0)
        for k in rows:
            if self._in(idx[k]):
                pmax = max(pmax, self._write(int(idx[k]), p[k]))
        if moves:
            self.max_prio = max(self.max_prio, pmax)

    def write_batch(self, pre=None, idx=None, prio=None, mix=None):
        E = 0 if pre is None else len(pre[0])
        B = 0 if idx is None else len(idx)
        if E + B == 0:
            return
        pmax = f32(0.0)
        voided = set()
        for e in range(E):  # actor rows first
            s, p = int(pre[0][e]), f32(pre[1][e])
            if not self._in(s):
                continue
            pmax = max(pmax, self._write(s, p))
            if not p > 0:  # nothing emitted: no learner row of this call re-arms the slot
                voided.add(s)
        if B:
            idx = np.asarray(idx, dtype=np.int64)
            p, moves = self._learner_prios(B, prio, mix)
            last = {int(s): k for k, s in enumerate(idx)}  # the largest position wins
            for s, k in last.items():
                if self._in(s) and s not in voided:
                    wp = self._write(s, p[k])
                    if moves:
                        pmax = max(pmax, wp)
        self.max_prio = max(self.max_prio, pmax)
        self.filled += E
        self.bump += 1


# ------------------------------------------------------------------ inputs of the sampler tests
SAMPLER_CAPACITIES = (1, 63, 64, 65, 4095, 4096, 4097, 262145)
SAMPLER_BATCHES = (1, 3, 64, 257)


def sampler_fills(C):
    """``filled`` values to draw at: full, one short, wrapped (slot C - 1 is the newest), and
    64 k + 1 (the newest leaf alone in its level-1 node)."""
    k = max(1, (C - 1) // 128) if C > 64 else 0
    return sorted({C, C - 1, 2 * C + 5, 64 * k + 1})


def sampler_leaves(C, length, seed=0):
    """fp32 priorities in [1, 256) with about 20 % zero-mass holes, two whole empty level-1 nodes
    where the tree has them, nothing at slots >= length.  Exact-sum inputs: log2(C) + 8 + 25 <= 53."""
    rng = np.random.default_rng(seed + 7919 * C)
    p = rng.uniform(1.0, 256.0, size=C).astype(np.float32)
    p = np.minimum(p, np.nextafter(f32(256.0), f32(0.0)))
    p[rng.random(C) < 0.2] = 0.0
    n1 = (C + FANOUT - 1) // FANOUT
    if n1 >= 4:
        for a in (1, n1 // 2):
            p[a * FANOUT:(a + 1) * FANOUT] = 0.0
    p[min(int(length), C):] = 0.0
    return p


def brute_force_cum(leaf, length, exclude_last):
    """Cumulative fp64 masses of the leaves with the excluded one zeroed (exact on exact-sum
    inputs, so independent of the order of summation)."""
    m = np.asarray(leaf, dtype=np.float64).copy()
    length = min(int(length), len(m))
    if exclude_last and length > 0:
        m[length - 1] = 0.0
    return np.cumsum(m)


def brute_force_draw(cum, i, B, seed, ctr):
    """The leaf whose cumulative-mass interval holds draw ``i``'s mass: the first with
    cum > mass; C if the mass is past the end."""
    mass = (uniform_double(seed, i, ctr) + float(i)) * float(cum[-1]) / float(B)
    return int(np.searchsorted(cum, mass, side="right"))
