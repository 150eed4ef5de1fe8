"""Host n-step batcher: reference-mode parity (Q1-Q4) and textbook semantics."""
import numpy as np
import pytest

from apex_amd.replay.nstep import BatchStorage

from . import goldens


def _drive(bs, rewards, dones, A=3, seed=0):
    rng = np.random.RandomState(seed)
    for t, (r, d) in enumerate(zip(rewards, dones)):
        bs.add(f"s{t}", r, t % A, d, rng.randn(A).astype(np.float32))
    return bs


def test_q1_reference_sums_n_plus_one_rewards():
    bs = _drive(BatchStorage(3, 0.5), [1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 0])
    # R(s0) = 1 + .5*2 + .25*3 + .125*4 = 3.25 with next = s3
    assert bs.states[0] == "s0" and bs.next_states[0] == "s3"
    assert bs.rewards[0] == pytest.approx(1 + 1 + 0.75 + 0.5)


def test_q2_q4_done_semantics():
    bs = _drive(BatchStorage(3, 0.5), [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 1])
    assert bs.states == ["s0", "s1", "s2"]  # tail s3, s4 dropped on done
    assert bs.next_states[-1] == "s5" and bs.dones[-1] == 1.0
    bs2 = _drive(BatchStorage(3, 0.5), [1], [1])  # Q4: no IndexError
    assert len(bs2) == 0


def test_textbook_mode():
    bs = _drive(BatchStorage(3, 0.5, mode="textbook"), [1, 2, 3, 4, 5], [0, 0, 0, 0, 1])
    assert bs.states == ["s0", "s1", "s2", "s3", "s4"]
    assert bs.next_states[0] == "s3" and bs.dones[0] == 0.0
    assert bs.rewards[0] == pytest.approx(1 + 0.5 * 2 + 0.25 * 3)
    assert bs.dones[2:] == [1.0, 1.0, 1.0]
    assert bs.rewards[4] == pytest.approx(5.0)
    assert bs.rewards[3] == pytest.approx(4 + 0.5 * 5)
    pr = bs.compute_priorities()
    assert pr.shape == (5,) and (pr > 0).all()


def _drive_reference_mode(bs, raises_on_lone_done):
    """400 scripted steps into either implementation's BatchStorage(3, 0.99): every batch it
    emits (priorities + the five lists) and the steps at which a done arrives on an empty
    window (Q4: the reference raises IndexError there, this framework emits nothing)."""
    rng = np.random.RandomState(3)
    T, A = 400, 6
    rewards = rng.randn(T)
    dones = rng.rand(T) < 0.06
    dones[0] = False
    qs = rng.randn(T, A).astype(np.float32)
    out, k, lone = {}, 0, []
    for t in range(T):
        args = (rng.randn(2).astype(np.float32), float(rewards[t]), int(t % A), bool(dones[t]), qs[t])
        if dones[t] and len(bs.state_deque) == 0:
            lone.append(t)
            if raises_on_lone_done:
                with pytest.raises(IndexError):
                    bs.add(*args)
            else:
                bs.add(*args)
            continue
        bs.add(*args)
        if len(bs) >= 50:
            b, p = bs.make_batch()
            out[f"prios{k}"] = np.asarray(p)
            for j, x in enumerate(b):
                out[f"batch{k}_{j}"] = np.asarray(x)
            k += 1
            bs.reset()
    out["n_batches"] = np.int64(k)
    out["lone_done_steps"] = np.asarray(lone, dtype=np.int64)
    return out


def test_reference_mode_matches_reference_batchstorage():
    """Against the reference's BatchStorage(3, 0.99) (recorded: tests/golden/nstep_reference_mode.npz)."""
    theirs = goldens.load("nstep_reference_mode")
    ours = _drive_reference_mode(BatchStorage(3, 0.99), raises_on_lone_done=False)
    n = int(theirs["n_batches"])
    assert int(ours["n_batches"]) == n and n >= 1
    np.testing.assert_array_equal(ours["lone_done_steps"], theirs["lone_done_steps"])
    for k in range(n):
        np.testing.assert_allclose(ours[f"prios{k}"], theirs[f"prios{k}"], rtol=1e-12)
        for j in range(5):
            np.testing.assert_array_equal(ours[f"batch{k}_{j}"], theirs[f"batch{k}_{j}"])
