"""The tall bf16 kernels over a bf16 observation ring (``ring_dtype="bf16"``): ``vec_host_tail`` rounds a row once
where it is written, as ``vectb_*`` round an fp32 row at every read: no bit may differ from the fp32-ring run; Q and
the flat gradient equal fp64 on exact inputs; a random learner step stays under the tall bf16 tests' K_TALL_BF16."""
import pytest
import torch

from apex_amd.models.dqn import DuelingDQN

from . import test_gpu_vector_tall_bf16 as tb
from . import test_gpu_vector_wide as wide
from . import test_gpu_vector_wide_bf16 as wbf
from .test_gpu_vector_tall import _tall_engine
from .test_gpu_vector_wide import _bias
from .vector_host_fixtures import TapeVectorEnv

pytestmark = pytest.mark.gpu


def _engine(cuda, obs, A, B=32, seed=0, vec=None, wide_dtype=None, ring_dtype="bf16", **kw):
    eng = _tall_engine(cuda, obs, A, B, seed, vec, tall_dtype="bf16", ring_dtype=ring_dtype, **kw)
    assert eng.learner.ring.dtype == eng.shard.ring.dtype == (torch.bfloat16 if ring_dtype == "bf16" else torch.float32)
    return eng


def _shard(cuda, x, A, m, steps=()):
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.vector_host import VectorHostShard

    rp = HBMReplay(4096, n_envs=len(x), n_step=3, device=cuda, frame_bytes=2 * x.shape[1])
    sh = VectorHostShard(rp, TapeVectorEnv(x, list(steps), A), seed=5, wide=True, tall=True, tall_dtype="bf16",
                         ring_dtype="bf16")
    sh.set_policy(m.to(cuda))
    sh.act()
    torch.cuda.synchronize()
    return sh


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


# 129: rows of 258 bytes, only 2-byte aligned (one store per component); 264, 1024: the paired dword stores
@pytest.mark.parametrize("obs", [129, 264, 1024])
def test_ring_rows_are_the_rounded_observations(cuda, obs, E=33, A=3):
    gen = torch.Generator().manual_seed(obs)
    x = torch.randn(2, E, obs, generator=gen)
    # exact bf16 rounding midpoints (ties go to the even neighbour, down and up) in the first and the last columns
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(2 + 3 * 2.0 ** -7)])
    x[:, :, :4], x[:, :, -4:] = ties, ties.flip(0)
    x[1, 7, 0::2], x[1, 7, 1::2] = float("inf"), float("-inf")   # (the row written after the only forward)
    step = dict(obs=x[1].numpy(), reward=torch.ones(E).numpy(), done=torch.zeros(E).numpy())
    sh = _shard(cuda, x[0].numpy(), A, DuelingDQN.from_shapes((obs,), A), [step])
    sh.act_and_step()
    ring, want = sh.ring.cpu(), x.to(torch.bfloat16)
    assert ring.dtype == torch.bfloat16 and ring.shape == (sh.replay.frame_capacity, obs) and 2 * E < len(ring)
    assert _bits(ring[:E]) == _bits(want[0]) and _bits(ring[E:2 * E]) == _bits(want[1])
    assert not ring[2 * E:].view(torch.int16).any()                 # every other row is untouched
    assert torch.equal(sh.observe().cpu(), want[1].float())         # observe() stays fp32 [E, obs]
    sh.close()


# 129: dword-unaligned rows, a one-column last slab; 260: 8-byte but not 16-byte aligned rows; 264: 16-byte aligned
# rows one octet past the first slab seam; 1024: four full slabs, the widest A, a ragged third row tile of the batch
@pytest.mark.parametrize("obs,A,B", [(129, 3, 1), (260, 18, 33), (264, 5, 32), (1024, 32, 96)])
def test_bf16_ring_is_bit_equal_to_the_fp32_ring(cuda, obs, A, B, E=16, T=12):
    runs = []
    for ring_dtype in ("fp32", "bf16"):
        gen = torch.Generator().manual_seed(obs)
        rows = torch.randn(T + 1, E, obs, generator=gen).numpy()   # arbitrary floats, not pre-rounded
        tape = [dict(obs=rows[t + 1], reward=torch.randn(E, generator=gen).numpy(),
                     done=(torch.rand(E, generator=gen) < 0.1).float().numpy()) for t in range(T)]
        eng = _engine(cuda, obs, A, B, seed=obs, vec=TapeVectorEnv(rows[0], tape, A), ring_dtype=ring_dtype, lr=1e-3)
        L = eng.learner
        _bias(L.model, gen)   # (the target keeps the initial weights: the two nets differ)
        eng.publish_params()
        rec = []
        for _ in range(T):
            eng.actor_step()
            rec += [eng.shard.q.clone(), eng.shard.actions.clone()]   # vectb_act's, of the step just taken
        assert len(eng.replay) >= B   # the draw fills every row of the batch
        for _ in range(3):
            L.sample()
            L.forward_backward()
            rec += [t.clone() for t in (L.idx, L.vec, L.q_s, L.q_s2, L.qt_s2, L.delta, L.lw, L.flat_grad, L.part)]
            L.optimize()
            L.write_priorities()
            rec += [L.loss.clone(), L.prio.clone(), L.flat.clone()]
        assert all(bool(torch.isfinite(t).all()) for t in rec) and float(L.flat_grad.abs().max()) > 0
        runs.append([_bits(t) for t in rec])
        eng.close()
    assert [a == b for a, b in zip(*runs)] == [True] * len(runs[0])


@pytest.fixture
def _over_bf16_ring(monkeypatch):   # the tall bf16 tests' bodies over a bf16 ring, under their own bound
    monkeypatch.setattr(wide, "K_E32", tb.K_TALL_BF16)
    monkeypatch.setattr(wbf, "_host_engine", _engine)
    monkeypatch.setattr(tb, "_engine", _engine)
    monkeypatch.setattr(tb, "_shard", _shard)


@pytest.mark.parametrize("obs,A", [(260, 16), (1024, 32)])
def test_bf16_ring_q_and_gradient_are_exact_on_exact_inputs(cuda, obs, A, _over_bf16_ring):
    tb.test_tall_bf16_act_is_exact_on_exact_inputs(cuda, obs, A)
    tb.test_tall_bf16_learner_is_exact_on_exact_inputs(cuda, obs, A)


def test_bf16_ring_learner_step_matches_fp64_with_the_same_rounding(cuda, _over_bf16_ring, obs=260, A=18, B=33):
    wbf.test_bf16_learner_step_matches_fp64_with_the_same_rounding(cuda, obs, A, B)


def test_bf16_ring_eager_reruns_and_graph_are_bit_equal(cuda, _over_bf16_ring):
    tb.test_tall_bf16_eager_and_graph_are_bit_equal(cuda)   # obs 260: 30 SGD steps eager and captured
    tb.test_tall_bf16_forward_backward_reruns_are_bit_equal(cuda, obs=260)
