"""The host models of the actor kernels (``tests/actor_oracle.py``) checked on their own:
Philox known answers, the epsilon-greedy rule, textbook n-step conservation and the game's
invariants.  No GPU: these pin the oracle that ``test_gpu_actor.py`` compares the kernels with."""
from collections import Counter

import numpy as np
import pytest

from . import actor_oracle as ao


# ------------------------------------------------------------------ Philox
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    assert ao.philox4x32_10(ctr, key) == want


def test_uniform4_word_layout_and_range():
    # counter / stream / seed split into (lo, hi) words exactly as common.h packs them
    seed, stream = (0x299F31D0 << 32) | 0xA4093822, (0x03707344 << 32) | 0x13198A2E
    ctr = (0x85A308D3 << 32) | 0x243F6A88
    u = ao.uniform4(seed, stream, ctr)
    want = [np.float32((w >> 8) * 2.0 ** -24) for w in (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)]
    assert [x.dtype for x in u] == [np.float32] * 4 and list(u) == want
    # the high words matter
    assert ao.uniform4(3, 5, 7) != ao.uniform4(3 + 2 ** 33, 5, 7)
    assert ao.uniform4(3, 5, 7) != ao.uniform4(3, 5, 7 + 2 ** 32)
    assert ao.uniform4(3, 5, 7) != ao.uniform4(3, 5 + 2 ** 32, 7)
    us = np.array([ao.uniform4(1, s, 0) for s in range(500)])
    assert us.min() >= 0.0 and us.max() < 1.0 and abs(us.mean() - 0.5) < 0.03


# ------------------------------------------------------------------ epsilon-greedy
def test_select_actions_ref_rules():
    E, A = 64, 6
    rng = np.random.default_rng(0)
    q = rng.standard_normal((E, A)).astype(np.float32)
    q[0] = 1.0                       # all equal -> index 0
    q[1] = [0, 2, 2, 1, 2, 0]        # tie -> the lower index
    q[2] = [0, 1, 2, 3, 4, 5]        # maximum at the last index
    greedy = ao.select_actions_ref(q, np.zeros(E, np.float32), 9, 4)
    assert greedy[0] == 0 and greedy[1] == 1 and greedy[2] == 5
    assert (greedy == q.argmax(1)).all()  # u0 >= 0 is never below eps = 0 ... unless u0 == 0 exactly
    rand = ao.select_actions_ref(q, np.ones(E, np.float32), 9, 4)
    assert (rand == ao.select_actions_ref(-q, np.ones(E, np.float32), 9, 4)).all()  # Q is ignored
    assert rand.min() >= 0 and rand.max() < A and len(set(rand.tolist())) == A
    for e in range(E):
        u = ao.uniform4(9, e, 4)
        assert rand[e] == min(int(np.float32(u[1] * np.float32(A))), A - 1)
    assert (ao.select_actions_ref(q, np.ones(E, np.float32), 9, 5) != rand).any()


# ------------------------------------------------------------------ textbook n-step conservation
class _DeviceTextbookQueue:
    """The textbook branch's bookkeeping of ``nstep_emit_k`` (window ring, drain ring of n rows,
    at most one emission per step), carrying only row ids: checks that the n-entry drain ring
    never overflows and that its timing is the oracle's FIFO."""

    def __init__(self, n):
        self.n, self.start, self.len = n, 0, 0
        self.win = [None] * n
        self.drain, self.dhead, self.dcnt = [None] * n, 0, 0

    def step(self, sa, done):
        n, out = self.n, None
        if self.len == n:
            out = (self.win[self.start], 0)
            self.start = (self.start + 1) % n
            self.len -= 1
        self.win[(self.start + self.len) % n] = sa
        self.len += 1
        if out is None and self.dcnt > 0:
            out = (self.drain[self.dhead], 1)
            self.dhead = (self.dhead + 1) % n
            self.dcnt -= 1
        if done:
            for j in range(self.len):
                row = self.win[(self.start + j) % n]
                if out is None:
                    out = (row, 1)
                else:
                    assert self.dcnt < n, "drain ring overflow"
                    self.drain[(self.dhead + self.dcnt) % n] = row
                    self.dcnt += 1
            self.len = self.start = 0
        assert self.len + self.dcnt <= n
        return out


EPISODES = [[5, 3, 9], [5, 2, 9], [7, 3, 3, 9], [1, 1, 1, 9], [6, 5, 9], [9, 1, 2, 1, 4, 1, 1, 3]]


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("lengths", EPISODES, ids=lambda v: "-".join(map(str, v)))
def test_textbook_oracle_conserves_batchstorage_rows(n, lengths):
    from apex_amd.replay.nstep import BatchStorage

    rng = np.random.default_rng(n * 100 + len(lengths))
    gamma = float(np.float32(0.99))
    orc = ao.NStepOracle(n, 0.99, "textbook", (0, 0, 0, 0))
    ref = BatchStorage(n, gamma, mode="textbook")
    dev = _DeviceTextbookQueue(n)
    emitted, t = [], 0
    for L in lengths:
        for i in range(L):
            hist, done = orc.hist, i == L - 1
            a, r = int(rng.integers(0, 6)), np.float32(rng.uniform(-2, 2))
            q = rng.standard_normal(6).astype(np.float32)
            ref.add(hist, float(r), a, done, q)
            row = orc.add(a, r, done, q, 100 + t)
            drow = dev.step(hist, done)
            assert (row is None) == (drow is None), (t, row, drow)
            if row is not None:
                assert (row.s_ids, int(row.done)) == drow
                emitted.append(row)
            assert len(orc.pending) <= n
            assert orc.hist == ((100 + t,) * 4 if done else hist[1:] + (100 + t,))
            t += 1
    key = lambda s, a, R, d: (tuple(s), int(a), round(float(R), 9), float(d))  # noqa: E731
    got = Counter(key(r.s_ids, r.action, r.reward, r.done) for r in emitted + list(orc.pending))
    want = Counter(key(ref.states[k], ref.actions[k], ref.rewards[k], ref.dones[k]) for k in range(len(ref)))
    assert got == want and sum(want.values()) == len(ref)
    # every (s, a) of a finished episode appears exactly once
    assert len(ref) == sum(lengths) and len(set(r.s_ids for r in emitted + list(orc.pending))) == len(ref)
    prios = ref.compute_priorities()
    for k, row in enumerate(orc.rows):  # compute_priorities mixes in float32 Q arithmetic: a few float32 ulp
        assert abs(row.prio - prios[k]) <= 2.0 ** -22 * (abs(prios[k]) + 4.0)


def test_reference_oracle_counts_stale_q_and_first_step_terminals():
    orc = ao.NStepOracle(3, 0.99, "reference", (0, 0, 0, 0))
    q = np.arange(4, dtype=np.float32)
    rows = []
    for t, done in enumerate([0, 0, 0, 0, 1,   # a long episode: regular emissions, then the terminal one
                              0, 1,            # 2 steps: its terminal row reads the previous episode's Q (Q3)
                              1,               # first step terminal: nothing (Q4)
                              0, 0, 0, 0]):
        rows.append(orc.add(t % 4, 0.5, bool(done), q + t, 10 + t))
    assert [r is not None for r in rows] == [False, False, False, True, True, False, True, False,
                                             False, False, False, True]
    assert orc.stale_q == 1 and orc.first_step_terminal == 1
    # Q3: the row emitted at t=6 starts at the state of t=5 but its priority uses Q of t=2
    r6 = rows[6]
    R = 0.5 + float(np.float32(0.99)) * 0.5
    assert r6.action == 5 % 4 and r6.done == 1.0
    assert r6.prio == pytest.approx(abs(R - float((q + 2)[5 % 4])) + 1e-6, rel=1e-12)


# ------------------------------------------------------------------ the game
@pytest.mark.parametrize("A,life,clip,repeat,max_steps", [(18, 1, 1, 4, 9), (18, 0, 0, 4, 0), (6, 1, 1, 4, 0),
                                                          (4, 0, 0, 1, 0)])
def test_env_oracle_free_running_invariants(A, life, clip, repeat, max_steps):
    E, F, seed = 4, 64, 7
    env = ao.VecEnvOracle(E, A, F, repeat, clip, life, max_steps)
    rng = np.random.default_rng(A)
    for e in range(E):
        st, log = env.reset(e, seed, 1), np.zeros(4, np.float32)
        assert env.frame_slot(0, e, reset=True) == e
        for t in range(120):
            out = env.step(st, int(rng.integers(0, A)), e, seed, t, log)
            st, log = out.state, out.ep_log
            assert 0 <= st[ao.S_PX] <= 80 and 42 <= st[ao.S_PY] <= 76
            ex = st[ao.S_EX:ao.S_EX + 6]
            assert (ex >= 0).all() and (ex <= 78).all()
            assert out.frame.dtype == np.uint8 and out.frame.shape == (84, 84)
            assert set(np.unique(out.frame).tolist()) <= set(ao.GREYS)
            assert 0 < (out.frame == 200).sum() <= 16  # the player is on screen (an enemy may graze it)
            if clip:
                assert out.reward in (-1.0, 0.0, 1.0)
            if max_steps:
                assert st[ao.S_EPLEN] < max_steps
            if out.done:
                assert st[ao.S_EPLEN] == 0 and st[ao.S_EPRET] == 0
            assert env.frame_slot(t, e) == ((t + 1) * E + e) % F
        if max_steps:
            assert log[2] >= 120 // max_steps


def test_env_oracle_fma_switch_changes_the_draws():
    """The two roundings of 4 + 72 u and 0.4 + 0.8 u differ on some draws (so a GPU test can tell
    which one the device uses) and never by more than one ulp."""
    fused, plain = (ao.VecEnvOracle(8, 18, 64, fused=f) for f in (True, False))
    a = np.stack([fused.reset(e, 3, 1) for e in range(8)])
    b = np.stack([plain.reset(e, 3, 1) for e in range(8)])
    assert (a != b).any()
    assert np.abs(a - b).max() <= np.spacing(np.float32(76.0))
    assert (a[:, ao.S_EY:ao.S_EY + 6] == 8 + 6 * np.arange(6)).all()
    assert (np.abs(a[:, ao.S_EVX:ao.S_EVX + 6]) >= np.float32(0.4)).all()
