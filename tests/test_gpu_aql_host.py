"""The host-env AQL engine (``engine/aql_host.py``, ``aql_host_tail``) on the GPU.

Small shapes throughout: E = 7 envs (the last 4-wave workgroup of the tail is partial), batch 8,
capacity 100 (not a multiple of 7: one step's ring slots wrap mid-step within the runs)."""
import json

import numpy as np
import pytest
import torch

from apex_amd import envs, train_aql

from . import aql_host_fixtures as fx

pytestmark = pytest.mark.gpu

E, CAP, BATCH = 7, 100, 8
EAGER_ITERS, GRAPH_ITERS = 27, 3


def _cfg(env_id, **kw):
    from apex_amd.engine.aql import AQLEngineConfig

    base = dict(env_id=env_id, n_envs=E, capacity=CAP, batch_size=BATCH, seed=3, learner_steps=2, max_step=40,
                fused_acting=False)   # (max_step 40: a short beta horizon, beta moves every iteration)
    base.update(kw)
    return AQLEngineConfig(**base)


def _final(eng):
    torch.cuda.synchronize()
    r, L = eng.replay, eng.learner
    t = dict(st=r.st, st2=r.st2, action=r.action, reward=r.reward, done=r.done, a_mu=r.a_mu, leaf_sum=r.leaf_sum,
             leaf_min=r.leaf_min, level1=r.node_sum[0], root=r.node_sum[-1], filled=r.filled, actor_ctr=eng.actor_ctr,
             obs_buf=eng.obs_buf, ep_len=eng.ep_len, ep_ret=eng.ep_ret, ep_count=eng.ep_count, ep_log=eng.ep_log,
             beta=L.beta, idx=L.idx, flat=L.flat, tflat=L.tflat, actor_flat=eng.actor_flat)
    return {k: v.detach().cpu().clone() for k, v in t.items()}


def _run(eng, eager, graphed, after=lambda: None):
    eng.fill()
    for _ in range(eager):
        eng.iteration()
        after()
    eng.capture()
    for _ in range(graphed):
        eng.iteration()
        after()
    return _final(eng)


# ------------------------------------------------------------------ 1. tape equivalence
def _record_tape(env_id, cuda):
    """The existing engine (separate acting launches), fill + eager + graph-captured iterations;
    after every acting step: env_act, the rows just written at ``slots`` and obs_buf."""
    from apex_amd.engine.aql import AQLEngine

    eng = AQLEngine(_cfg(env_id), cuda)
    assert eng._tail is None
    torch.cuda.synchronize()
    first = eng.obs_buf.cpu().numpy().copy()
    steps = []

    def record():
        torch.cuda.synchronize()
        sl = eng.slots.long()
        r = eng.replay
        done = r.done[sl].cpu().numpy().copy()
        steps.append(dict(env_act=eng.env_act.cpu().numpy().copy(), next_obs=r.st2[sl].cpu().numpy().copy(),
                          reward=r.reward[sl].cpu().numpy().copy(), done=done, ended=done.copy(),
                          reset_obs=eng.obs_buf.cpu().numpy().copy(), slots=sl.cpu().numpy().copy()))

    step = eng.actor_step

    def fill_step(*a, **k):   # (fill() acts through actor_step: record each of its steps)
        step(*a, **k)
        record()

    eng.actor_step = fill_step
    eng.fill()
    del eng.actor_step
    n_fill = len(steps)
    for _ in range(EAGER_ITERS):
        eng.iteration()
        record()
    eng.capture()
    for _ in range(GRAPH_ITERS):
        eng.iteration()
        record()
    return eng, first, steps, n_fill, _final(eng)


@pytest.mark.parametrize("env_id", ["Pendulum-v0", "BipedalWalker-v3", "CartPole-v0"])
def test_tape_equivalence(cuda, env_id):
    """A scripted host env that plays back what the device envs of the existing engine did (and
    checks that it is handed the same actions, bit for bit) leaves ``AQLHostEngine(host_overlap=
    False)`` with the same replay, tree, counters, episode state, beta and learner as the existing
    engine with its separate acting launches: ``aql_host_tail`` writes what select + env step +
    ring write wrote.  ep_log rows of episodes that ended in the SAME acting step are compared as
    a set: both kernels log those in the order their waves reach an atomic counter."""
    from apex_amd.engine.aql_host import AQLHostEngine

    ref, first, steps, n_fill, want = _record_tape(env_id, cuda)
    assert n_fill == 2 and len(steps) == n_fill + EAGER_ITERS + GRAPH_ITERS
    assert any((s["slots"][1:] < s["slots"][:-1]).any() for s in steps)          # a step's slots wrapped
    n_done = int(sum(s["done"].sum() for s in steps))
    if env_id == "CartPole-v0":
        assert n_done >= 1                                                       # (a condition on the input)
    vec = fx.ScriptedVec(first, steps, ref.cont, ref.adim, ref.model.num_actions, ref.low.cpu().numpy(),
                         ref.high.cpu().numpy(), ref.eval_limit)
    eng = AQLHostEngine(_cfg(env_id), vec, cuda, host_overlap=False)
    assert eng.T == ref.T and eng.K == ref.K == 2
    got = _run(eng, EAGER_ITERS, GRAPH_ITERS)
    assert vec.t == len(steps) and eng.env_steps == E * len(steps)
    assert eng.learner_steps == ref.learner_steps and list(eng.target_syncs) == list(ref.target_syncs)
    for k in want:
        if k != "ep_log":
            assert torch.equal(got[k], want[k]), (k, (got[k].double() - want[k].double()).abs().max().item())
    assert int(want["ep_count"]) == n_done
    c = 0
    for s in steps:   # rows [c, c + m) are the m episodes that ended in this step
        m = int(s["done"].sum())
        a, b = got["ep_log"][c:c + m].tolist(), want["ep_log"][c:c + m].tolist()
        assert sorted(a) == sorted(b), (c, a, b)
        c += m
    assert torch.equal(got["ep_log"][c:], want["ep_log"][c:])
    assert got["beta"].item() != _cfg(env_id).beta_start
    eng.close()


# ------------------------------------------------------------------ 2. cap reset
def test_cap_reset_keeps_done_zero(cuda):
    """ended = 1 with done = 0 (the length cap): the replay's done stays 0, obs_buf takes
    reset_obs, ep_log gets the return and length, ep_ret / ep_len restart -- every acting step
    compared exactly with the numpy model (at most one env ends per step: the log order is then
    defined)."""
    from apex_amd.engine.aql_host import AQLHostEngine

    rng = np.random.RandomState(0)
    n_steps, obs = 20, 3
    steps = []
    for t in range(n_steps):
        nxt = rng.uniform(-1, 1, size=(E, obs)).astype(np.float32)
        ended = np.zeros(E, np.float32)
        done = np.zeros(E, np.float32)
        if t % 3 == 2:
            ended[(5 * t) % E] = 1.0          # a cap reset: done stays 0
        if t % 7 == 5:
            e = (5 * t + 1) % E
            ended[:] = 0.0
            ended[e] = done[e] = 1.0          # a terminal, for contrast
        rst = np.where(ended[:, None] != 0, rng.uniform(-1, 1, size=(E, obs)).astype(np.float32), nxt)
        steps.append(dict(next_obs=nxt, reset_obs=rst, reward=rng.uniform(-2, 2, size=E).astype(np.float32),
                          done=done, ended=ended))
    caps = sum(int(((s["ended"] != 0) & (s["done"] == 0)).sum()) for s in steps)
    assert caps >= 4 and all(s["ended"].sum() <= 1 for s in steps)
    first = rng.uniform(-1, 1, size=(E, obs)).astype(np.float32)
    vec = fx.ScriptedVec(first, steps, True, 1, 1, [-2.0], [2.0])
    eng = AQLHostEngine(_cfg("scripted"), vec, cuda, host_overlap=False)
    r = eng.replay
    torch.cuda.synchronize()
    assert np.array_equal(eng.obs_buf.cpu().numpy(), first)
    st = dict(st=np.zeros((CAP, obs), np.float32), st2=np.zeros((CAP, obs), np.float32),
              action=np.zeros(CAP, np.int32), reward=np.zeros(CAP, np.float32), done=np.zeros(CAP, np.float32),
              a_mu=np.zeros((CAP, eng.T, 1), np.float32), filled=0, obs_buf=first.copy(),
              ep_len=np.zeros(E, np.int32), ep_ret=np.zeros(E, np.float32), ep_count=0,
              ep_log=np.zeros((eng.log_cap, 2), np.float32))
    for t, s in enumerate(steps):
        eng.actor_step()
        torch.cuda.synchronize()
        fx.tail_model(st, s, eng.amu.cpu().numpy(), eng.act_idx.cpu().numpy(), CAP, eng.log_cap)
        got = dict(st=r.st, st2=r.st2, action=r.action, reward=r.reward, done=r.done, a_mu=r.a_mu,
                   obs_buf=eng.obs_buf, ep_len=eng.ep_len, ep_ret=eng.ep_ret, ep_log=eng.ep_log)
        for k, v in got.items():
            assert np.array_equal(v.cpu().numpy(), st[k]), (t, k)
        assert int(r.filled) == st["filled"] == E * (t + 1) and int(eng.ep_count) == st["ep_count"]
        assert int(eng.actor_ctr) == t + 1
        sl = eng.slots.cpu().numpy()
        assert sl.tolist() == [(E * t + e) % CAP for e in range(E)]
        assert np.array_equal(r.done[eng.slots.long()].cpu().numpy(), s["done"])        # a cap reset stores done = 0
        assert (r.leaf_sum[eng.slots.long()] > 0).all()
    assert st["ep_count"] == sum(int(s["ended"].sum()) for s in steps)
    assert float(r.node_sum[-1][0]) == pytest.approx(float(r.leaf_sum.double().sum()), rel=1e-12)
    assert eng.finished_episodes() == [(float(a), int(b)) for a, b in st["ep_log"][:st["ep_count"]]]
    eng.close()


# ------------------------------------------------------------------ 3. overlap is race-free
def test_overlap_is_race_free(cuda):
    """host_overlap=True as is == the same run with a device synchronize after every enqueue:
    the one-stream order alone protects the staging block, the actions and the published weights."""
    from apex_amd.engine.aql_host import AQLHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    class Synced(AQLHostEngine):
        syncs = 0

        def _enqueued(self):
            torch.cuda.synchronize()
            self.syncs += 1

    out = []
    for cls in (AQLHostEngine, Synced):
        vec = HostVectorEnv("MountainCarContinuous-v0", E, seed=21, max_episode_length=9)
        eng = cls(_cfg("MountainCarContinuous-v0"), vec, cuda)
        assert eng.host_overlap
        out.append(_run(eng, 8, 6))
        if cls is Synced:
            assert eng.syncs > 5 * 14
        eng.close()
    # (the car never reaches the goal this early: every env ends at the cap, all E in one step,
    # and the tail logs the episodes of one step in the order its waves reach the counter)
    n = int(out[0]["ep_count"])
    assert n == E * (16 // 9) and not out[0]["done"].any()
    for k in out[0]:
        if k != "ep_log":
            assert torch.equal(out[0][k], out[1][k]), k
    for c in range(0, n, E):
        assert sorted(out[0]["ep_log"][c:c + E].tolist()) == sorted(out[1]["ep_log"][c:c + E].tolist()), c
    assert torch.equal(out[0]["ep_log"][n:], out[1]["ep_log"][n:])


# ------------------------------------------------------------------ 4. a real host env
def test_mountain_car_through_the_public_engine(cuda):
    """MountainCarContinuous-v0 (the GPU-env engine refuses it) trains under AQLHostEngine, and
    the replay holds exactly what fresh envs with seeds seed + i do when fed the stored actions."""
    from apex_amd.engine.aql import AQLEngine, AQLEvaluator
    from apex_amd.engine.aql_host import AQLHostEngine
    from apex_amd.envs.host_vector import HostVectorEnv

    env_id, seed, cap_len, iters = "MountainCarContinuous-v0", 5, 5, 10
    with pytest.raises(ValueError, match="GPU AQL env must be one of"):
        AQLEngine(_cfg(env_id), cuda)
    vec = HostVectorEnv(env_id, E, seed=seed, max_episode_length=cap_len)
    eng = AQLHostEngine(_cfg(env_id, track_losses=True), vec, cuda)
    eng.fill()
    for _ in range(iters):
        eng.iteration()
    torch.cuda.synchronize()
    lq, lp, n = eng.learner.take_loss_means()
    assert n == iters * eng.K and np.isfinite(lq) and np.isfinite(lp)
    assert all(np.isfinite(v) for v in eng.learner.stats().values())
    n_steps = 2 + iters
    assert int(eng.replay.filled) == E * n_steps <= CAP and eng.env_steps == E * n_steps
    r = eng.replay
    st, st2, rew, done = (x.cpu().numpy() for x in (r.st, r.st2, r.reward, r.done))
    a_mu, action = r.a_mu.cpu().numpy(), r.action.cpu().numpy()
    sim = [envs.make(env_id) for _ in range(E)]
    for i, e in enumerate(sim):
        e.seed(seed + i)
    cur = [np.asarray(e.reset(), dtype=np.float32) for e in sim]
    length = [0] * E
    resets = 0
    for t in range(n_steps):
        for i, e in enumerate(sim):
            slot = t * E + i
            assert np.array_equal(st[slot], cur[i]), (t, i)
            a = a_mu[slot, action[slot]].astype(np.float32).reshape(e.action_space.shape)
            o, rr, d, _ = e.step(a)
            o = np.asarray(o, dtype=np.float32)
            assert np.array_equal(st2[slot], o) and rew[slot] == np.float32(rr) and done[slot] == float(d), (t, i)
            length[i] += 1
            if d or length[i] >= cap_len:
                cur[i], length[i] = np.asarray(e.reset(), dtype=np.float32), 0
                resets += 1
            else:
                cur[i] = o
    assert resets == E * (n_steps // cap_len) and int(eng.ep_count) == resets and not done.any()   # cap resets
    assert np.array_equal(eng.obs_buf.cpu().numpy(), np.stack(cur))
    # the device-env evaluators are refused; the host one runs
    with pytest.raises(RuntimeError, match="evaluate"):
        eng.rollout_evaluate(2)
    with pytest.raises(TypeError, match="AQLEngine"):
        AQLEvaluator(eng, 2)
    ret = eng.evaluate(1, seed=3)
    assert len(ret) == 1 and np.isfinite(ret[0])
    eng.close()


def test_launcher_limits(cuda):
    from apex_amd.engine.aql_host import AQLHostEngine

    vec = fx.ScriptedVec(np.zeros((1025, 2), np.float32), [], True, 1, 1, [-1.0], [1.0])
    with pytest.raises(ValueError, match="1024"):
        AQLHostEngine(_cfg("scripted", capacity=4096), vec, cuda)
    vec = fx.ScriptedVec(np.zeros((E, 2), np.float32), [], True, 1, 1, [-1.0], [1.0])
    eng = AQLHostEngine(_cfg("scripted"), vec, cuda)
    h = eng.hip
    d = dict(E=1025, obs=2, adim=1, T=eng.T, stage=eng.stage_dev.data_ptr(), obs_buf=eng.obs_buf.data_ptr(),
             amu=eng.amu.data_ptr(), act_idx=eng.act_idx.data_ptr(), ep_len=eng.ep_len.data_ptr(),
             ep_ret=eng.ep_ret.data_ptr(), ep_count=eng.ep_count.data_ptr(), ep_log=eng.ep_log.data_ptr(),
             log_cap=eng.log_cap, alpha=0.6, max_prio=eng.replay.max_prio.data_ptr(),
             filled=eng.replay.filled.data_ptr(), counter=eng.actor_ctr.data_ptr(), ticket=eng._ticket.data_ptr())
    with pytest.raises(ValueError, match="1024"):   # the launcher throws before anything is launched
        h.aql_host_tail(h.make_aql_host_tail(eng.ins, eng.replay.tree, d), torch.cuda.current_stream().cuda_stream)
    eng.close()


# ------------------------------------------------------------------ 5. CLI
def test_cli_trains_and_checkpoints(cuda, tmp_path, monkeypatch):
    scalars = []

    class Writer(train_aql.NullWriter):
        def add_scalar(self, tag, value, step=None, *a, **k):
            scalars.append((tag, float(value)))

    monkeypatch.setattr(train_aql, "NullWriter", Writer)
    log = tmp_path / "log.jsonl"
    assert train_aql.main(["--host-envs", "--env", "MountainCarContinuous-v0", "--n-envs", "4", "--max-step", "30",
                           "--batch-size", "8", "--capacity", "1000", "--save-interval", "20", "--log-interval", "10",
                           "--no-tb", "--save-dir", str(tmp_path), "--json-log", str(log),
                           "--max-episode-length", "11"]) == 0
    for it in (0, 20, 29):
        assert (tmp_path / f"model{it}.pth").exists() and (tmp_path / f"model{it}.pth.train.pt").exists()
    from apex_amd.models.aql import AQL
    from apex_amd.utils.checkpoint import load_model

    m = AQL(envs.make("MountainCarContinuous-v0"), propose_sample=1, uniform_sample=50, device="cpu")
    load_model(m, str(tmp_path / "model29.pth"))
    assert all(torch.isfinite(p).all() for p in m.parameters())
    recs = [json.loads(x) for x in log.read_text().splitlines()]
    assert recs and recs[-1]["iteration"] == 29 and recs[-1]["learner_steps"] > 0
    assert sum(r["episodes"] for r in recs) > 0                     # host episodes reached the log
    rates = [v for tag, v in scalars if tag == "actor/env_steps_per_sec"]
    assert rates and all(v > 0 for v in rates)
