"""The host-env evaluator of a ``wide_net`` engine (``engine/vector_host_eval.py``): the one-launch act
``vecw_host_eval_act`` against the three-launch step form (bit for bit) and against fp64 PyTorch within
``test_gpu_vector_wide``'s bound, K_E32 x fp32 PyTorch's own error per act; weight sets; launcher refusals."""
import numpy as np
import pytest
import torch

from apex_amd import ops
from apex_amd.engine.vector import vec_net
from apex_amd.engine.vector_host_eval import VectorHostEvaluator
from apex_amd.models.dqn import DuelingDQN

from .test_gpu_vector_wide import K_E32, U32, _bias, _cast, _check, _err, _host_engine
from .vector_host_fixtures import TapeVectorEnv

pytestmark = pytest.mark.gpu


def _tape(obs, N, steps, gen):
    """steps + 1 observation blocks [N, obs] (the reset row first) and the tape: env e ends every 2 + e % 3 steps."""
    rows = torch.randn(steps + 1, N, obs, generator=gen).numpy()
    done = lambda t: ((t + 1) % (2 + np.arange(N) % 3) == 0).astype(np.float32)  # noqa: E731
    return rows, [dict(obs=rows[t + 1], reward=np.ones(N, np.float32), done=done(t)) for t in range(steps)]


def _evaluator(eng, rows, tape, kernel="fused"):
    return VectorHostEvaluator(eng, TapeVectorEnv(rows[0], tape, eng.A), kernel=kernel, seed=11)


def _act(ev):
    ev.step_begin()
    ev.stream.synchronize()
    out = ev.q.cpu().numpy().copy(), ev.actions.cpu().numpy().copy()
    ev.step_end()
    return out


def _check_q(tag, q, x, model):
    """q [N, A] against the fp64 forward within the wide bound; the fp64 rows and the bound in absolute terms."""
    x = torch.from_numpy(x)
    q64, q32 = (_cast(model, dt)(x.to(dt)).detach().numpy() for dt in (torch.float64, torch.float32))
    _check(tag, q, q32, q64)
    return q64, K_E32 * max(_err(q32, q64), U32) * np.abs(q64).max()


# (5, 3, 1): one row, K padded 5 -> 8, features.0 rows unaligned; (9, 3, 33): obs % 4 != 0, a second workgroup with
# one live row; (12, 6, 8): A % 4 != 0, value.0 unaligned in the flat vector; (128, 32, 64): the limits, both full
@pytest.mark.parametrize("obs,A,N", [(5, 3, 1), (9, 3, 33), (12, 6, 8), (128, 32, 64)])
def test_fused_equals_step_equals_fp64(cuda, obs, A, N):
    eng = _host_engine(cuda, obs, A, seed=obs)
    gen = torch.Generator().manual_seed(obs)
    _bias(eng.learner.model, gen)
    rows, tape = _tape(obs, N, 3, gen)
    fused, step = _evaluator(eng, rows, tape), _evaluator(eng, rows, tape, "step")
    for k in range(3):
        (q, act), (qs, acts) = _act(fused), _act(step)
        assert np.array_equal(q.view(np.uint32), qs.view(np.uint32)) and np.array_equal(act, acts), k
        q64, bound = _check_q(f"eval act obs={obs} A={A} N={N} k={k}", q, rows[k], eng.learner.model)
        assert (np.diff(np.sort(q64, axis=1)[:, -2:]) > 2 * bound).all()   # no near-tie (an entry may move by it)
        assert np.array_equal(act, q64.argmax(1)), k
    fused.close(), step.close(), eng.close()


def test_refresh_switches_the_weight_set_and_run_agrees(cuda):
    eng = _host_engine(cuda, 12, 6, seed=2)
    gen = torch.Generator().manual_seed(7)
    _bias(eng.learner.model, gen)
    rows, tape = _tape(12, 8, 12, gen)
    ev, old = _evaluator(eng, rows, tape), _cast(eng.learner.model, torch.float64)
    _check_q("old set", _act(ev)[0], rows[0], old)
    _bias(eng.learner.model, gen)                      # the online parameters move on (same stream as refresh)
    assert ev.refresh() is True
    q1 = _act(ev)[0]
    _check_q("new set", q1, rows[1], eng.learner.model)
    assert _err(q1, old(torch.from_numpy(rows[1]).double()).detach().numpy()) > 1e-3   # not the old set's
    ev.close()
    episodes = []
    for kernel in ("fused", "step"):
        ev = _evaluator(eng, rows, tape, kernel)
        ev.run(12)
        episodes.append([e[:2] for e in ev.poll()])
        ev.close()
    assert episodes[0] == episodes[1] and len(episodes[0]) == sum(12 // (2 + e % 3) for e in range(8))
    eng.close()


@pytest.mark.parametrize("bad,k", [(dict(N=0), 0), (dict(N=65), 0), ({}, -1), (dict(stage=0), 0)])
def test_launcher_refusals(cuda, bad, k):
    h, N, m = ops.hip(), 8, DuelingDQN.from_shapes((9,), 3).to(cuda)
    stage = torch.zeros(N * (2 * 9 + 3), device=cuda)
    q, actions = torch.full((N, 3), -12345.0, device=cuda), torch.full((N,), -77, dtype=torch.int32, device=cuda)
    d = dict(N=N, seed=1, stage=stage.data_ptr(), q=q.data_ptr(), actions=actions.data_ptr())
    with pytest.raises(ValueError):
        h.vecw_host_eval_act(h.make_vecw_host_eval_act(vec_net(h, m), dict(d, **bad)), k,
                             torch.cuda.current_stream().cuda_stream)
    assert (q == -12345.0).all() and (actions == -77).all()   # nothing reached the GPU (the reads synchronize)
