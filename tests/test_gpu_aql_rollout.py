"""Greedy evaluation of the GPU AQL engine on the device: the stepwise evaluator
(``AQLEngine.evaluate``), the one-launch rollout (``aql_rollout`` / ``rollout_evaluate``) and the
non-blocking ``AQLEvaluator``.

The rollout must reproduce the stepwise evaluator bit for bit; its trace is teacher-forced
through the existing kernels (``aql_propose``, ``aql_candidate_q``), checked against the fp64
eval-mode ``Q_Network`` and against the host envs of ``envs/classic.py``.
"""
import copy
import json

import numpy as np
import pytest
import torch

from . import aql_rollout_fixtures as fx

pytestmark = pytest.mark.gpu

SENT = -12345.0
U5P3 = dict(uniform_sample=5, propose_sample=3)          # T = 8
T67 = dict(uniform_sample=60, propose_sample=7)          # T = 67: a candidate loop crosses a wave width
CASES = {"cartpole": ("CartPole-v0", fx.CARTPOLE_KW, 5, None),           # natural T = 2 + 3
         "pendulum": ("Pendulum-v0", U5P3, 3, None),
         "bipedal": ("BipedalWalker-v3", U5P3, 5, 48),
         "pendulum67": ("Pendulum-v0", T67, 3, 40)}
# (CartPole's env seeds are self-checked on the host: test_aql_rollout_host)
SEEDS = {"cartpole": fx.CARTPOLE_SEEDS[0], "pendulum": 77, "bipedal": 4321, "pendulum67": 99}
_ENGINES, _TRACES = {}, {}


def _engine(cuda, env_id, fill=0, **kw):
    from apex_amd.engine.aql import AQLEngine, AQLEngineConfig

    cfg = AQLEngineConfig(env_id=env_id, n_envs=64, capacity=8192, batch_size=32, use_graphs=False, **kw)
    eng = AQLEngine(cfg, cuda)
    # non-zero biases (every bias path exercised), non-zero NoisyNet sigma AND epsilon (a kernel
    # that wrongly applies the noise in evaluation is caught): the host self-check's weights
    fx.set_params(eng.model)
    eng.learner.sync_target()
    eng.publish()
    if fill:
        eng.fill(fill)
    torch.cuda.synchronize()
    return eng


def _shared(cuda, case):
    if case not in _ENGINES:
        env_id, kw, _, _ = CASES[case]
        _ENGINES[case] = _engine(cuda, env_id, **kw)
    return _ENGINES[case]


def _trace_bufs(eng, rows, Tr):
    dev = eng.device
    f = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=dev)  # noqa: E731
    return dict(obs=f(rows, Tr, eng.obs), amu=f(rows, Tr, eng.T, eng.adim), q=f(rows, Tr, eng.T),
                act=torch.full((rows, Tr), -7, dtype=torch.int32, device=dev), rew=f(rows, Tr))


def _traced(cuda, case):
    """One traced launch per case (computed once, shared, never modified)."""
    if case not in _TRACES:
        from apex_amd.engine.aql import AQLRolloutBuffers

        eng = _shared(cuda, case)
        _, _, n, limit = CASES[case]
        limit = eng.eval_limit if limit is None else limit
        ro = AQLRolloutBuffers(eng, eng.eval_net, n)
        tr = _trace_bufs(eng, n, limit)
        ro.launch(SEEDS[case], limit, tr)
        torch.cuda.synchronize()
        _TRACES[case] = dict(eng=eng, n=n, limit=limit, seed=SEEDS[case], returns=ro.returns.cpu().numpy(),
                             lengths=ro.lengths.cpu().numpy(), ended=ro.ended.cpu().numpy(),
                             **{k: v.cpu().numpy() for k, v in tr.items()}, dev=tr)
    return _TRACES[case]


# ------------------------------------------------------------------ 1. rollout == stepwise
@pytest.mark.parametrize("case,n,limit", [("cartpole", 1, None), ("cartpole", 4, None), ("cartpole", 5, None),
                                          ("cartpole", 9, None), ("pendulum", 3, None), ("bipedal", 5, 48),
                                          ("pendulum67", 3, 40)])
def test_rollout_equals_stepwise(cuda, case, n, limit):
    eng = _shared(cuda, case)
    seed = SEEDS[case]
    a = eng.evaluate(n, seed=seed, max_episode_steps=limit)
    b = eng.rollout_evaluate(n, seed=seed, max_episode_steps=limit)
    lengths, ended = eng._rollout.lengths.tolist(), eng._rollout.ended.tolist()
    print(case, n, a, b, lengths, ended)
    assert len(a) == len(b) == n
    assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    assert all(e in (1, 2) for e in ended)
    if case == "cartpole":
        assert b == [float(x) for x in lengths]                # reward 1 per step
        if n == 9:
            assert len(set(lengths)) > 1                        # episodes of different lengths in one launch
    if case == "pendulum":
        assert lengths == [200] * n and ended == [2] * n       # Pendulum never terminates
    if limit is not None:
        assert all(x <= limit for x in lengths)


def test_default_seed_and_time_limit(cuda):
    eng = _shared(cuda, "cartpole")
    assert eng.evaluate(4) == eng.rollout_evaluate(4)           # default seed: the same derivation
    assert eng.rollout_evaluate(4, seed=fx.CARTPOLE_SEEDS[1]) == eng.evaluate(4, seed=fx.CARTPOLE_SEEDS[1])
    cut = eng.rollout_evaluate(6, seed=SEEDS["cartpole"], max_episode_steps=3)
    assert cut == [3.0] * 6 and eng._rollout.ended.tolist() == [2] * 6
    # a cut at 10 steps: every episode that survives 10 steps returns exactly 10.0 (with these
    # random weights the greedy episodes last 8 to 11 steps, so shorter ones keep their return;
    # the 3-step cut above binds on every episode)
    full = eng.rollout_evaluate(6, seed=SEEDS["cartpole"])
    cut10 = eng.rollout_evaluate(6, seed=SEEDS["cartpole"], max_episode_steps=10)
    assert cut10 == [min(x, 10.0) for x in full] and 10.0 in cut10
    assert [e for x, e in zip(full, eng._rollout.ended.tolist()) if x > 10.0] == [2] * sum(x > 10.0 for x in full)
    assert cut10 == eng.evaluate(6, seed=SEEDS["cartpole"], max_episode_steps=10)


# ------------------------------------------------------------------ 2. teacher-forced trace
@pytest.mark.parametrize("case", list(CASES))
def test_trace_teacher_forced_through_stepwise_kernels(cuda, case):
    tr = _traced(cuda, case)
    eng, n, dev = tr["eng"], tr["n"], tr["dev"]
    h, s = eng.hip, torch.cuda.current_stream().cuda_stream
    steps = min(int(tr["lengths"].max()), 24)
    ctr = torch.zeros(1, dtype=torch.int64, device=eng.device)
    amu = torch.zeros(n, eng.T, eng.adim, device=eng.device)
    q = torch.zeros(n, eng.T, device=eng.device)
    ws = torch.zeros(h.aql_workspace_floats(), device=eng.device)
    for t in range(steps):
        live = tr["lengths"] > t
        obs_t = dev["obs"][:, t].contiguous()
        obs_t[torch.as_tensor(~live, device=eng.device)] = 0.0   # (rows past their end: sentinels)
        ctr.fill_(t)
        h.aql_propose(eng.eval_net, obs_t.data_ptr(), n, eng.low.data_ptr(), eng.high.data_ptr(),
                      eng.var.data_ptr(), tr["seed"] ^ 0x9909, ctr.data_ptr(), amu.data_ptr(), 0, s)
        am_t = dev["amu"][:, t].contiguous()
        h.aql_candidate_q(eng.eval_net, ws.data_ptr(), obs_t.data_ptr(), am_t.data_ptr(), n, q.data_ptr(), s)
        torch.cuda.synchronize()
        a_ref, q_ref = amu.cpu().numpy(), q.cpu().numpy()
        assert np.array_equal(a_ref[live].view(np.uint32), tr["amu"][live, t].view(np.uint32)), t
        assert np.array_equal(q_ref[live].view(np.uint32), tr["q"][live, t].view(np.uint32)), t
        assert np.array_equal(tr["act"][live, t], np.argmax(tr["q"][live, t], axis=1)), t   # first argmax
    U = int(eng.model.uniform_sample)
    for b in range(n):
        L = min(int(tr["lengths"][b]), tr["limit"])
        uni = tr["amu"][b, :L, :U]
        if eng.cont:
            lo, hi = eng.low.cpu().numpy(), eng.high.cpu().numpy()
            assert (uni >= lo).all() and (uni <= hi).all()
        else:
            na = int(eng.model.num_actions)
            cand = tr["amu"][b, :L, :, 0]
            assert np.isin(cand, np.arange(na)).all()
            assert all(len(set(row[:U])) == U for row in cand)   # distinct: without replacement


# ------------------------------------------------------------------ 3. eval mode against fp64
@pytest.mark.parametrize("case", ["cartpole", "bipedal", "pendulum67"])
def test_trace_q_is_the_eval_mode_fp64_q(cuda, case):
    tr = _traced(cuda, case)
    eng, n = tr["eng"], tr["n"]
    rows = [(b, t) for b in range(n) for t in range(min(int(tr["lengths"][b]), 16))]
    bi, ti = np.array(rows).T
    obs = torch.as_tensor(tr["obs"][bi, ti], dtype=torch.float64, device=eng.device)
    am = torch.as_tensor(tr["amu"][bi, ti], dtype=torch.float64, device=eng.device)
    q32 = torch.as_tensor(tr["q"][bi, ti], dtype=torch.float64, device=eng.device)
    ref = copy.deepcopy(eng.model).double()
    R, T = len(rows), eng.T

    def q64(mode_train):
        ref.q.train(mode_train)
        with torch.no_grad():
            qn = ref.q
            a_out = qn.action_out(am.reshape(R * T, eng.adim)).reshape(R, T, qn.A_OUT)
            q_f = qn.q_feature(obs).repeat(1, T).reshape(R, T, qn.F_OUT)
            return qn.forward(torch.relu(torch.cat([a_out, q_f], dim=2))).reshape(R, T)

    means, noisy = q64(False), q64(True)
    err = float((q32 - means).abs().max() / means.abs().max().clamp_min(1e-30))
    err_noisy = float((q32 - noisy).abs().max() / noisy.abs().max().clamp_min(1e-30))
    print(case, "rel err vs means", err, "vs noisy", err_noisy)
    assert err < 1e-5, err                      # the project's bound for this forward
    assert err_noisy > 1e-3, err_noisy          # the test tells the two apart


# ------------------------------------------------------------------ 4. env against the host
def _sum32(x):
    acc = np.float32(0.0)
    for v in x:
        acc = np.float32(acc + np.float32(v))
    return acc


def _check_returns(tr):
    for b in range(tr["n"]):
        L = int(tr["lengths"][b])
        assert 1 <= L <= tr["limit"]
        assert _sum32(tr["rew"][b, :L]).view(np.uint32) == tr["returns"][b].view(np.uint32)


def test_cartpole_env_from_trace(cuda):
    from apex_amd import envs

    tr = _traced(cuda, "cartpole")
    _check_returns(tr)
    env = envs.make("CartPole-v0").unwrapped
    assert (np.abs(tr["obs"][:, 0]) <= 0.05).all()
    total = skipped = 0
    for b in range(tr["n"]):
        L = int(tr["lengths"][b])
        for t in range(L):
            s = tr["obs"][b, t].astype(np.float64)
            a = int(tr["amu"][b, t, tr["act"][b, t], 0])
            env.reset()
            env.state = tuple(float(x) for x in s)
            env.steps_beyond_done = None
            ns, rr, dd, _ = env.step(a)
            total += 1
            assert rr == tr["rew"][b, t] == 1.0
            near = min(abs(abs(ns[0]) - 2.4), abs(abs(ns[2]) - env.theta_threshold_radians)) < 1e-4
            if near:
                skipped += 1
                continue
            if t + 1 < L:
                assert not dd
                np.testing.assert_allclose(tr["obs"][b, t + 1], ns, rtol=1e-4, atol=1e-5)
            else:   # the episode's last step: the host's terminal flag decides `ended`
                assert tr["ended"][b] == (1 if dd else 2)
                assert dd or L == tr["limit"]
    assert skipped <= 0.01 * total, (skipped, total)


def test_pendulum_env_from_trace(cuda):
    from apex_amd import envs

    tr = _traced(cuda, "pendulum")
    _check_returns(tr)
    env = envs.make("Pendulum-v0").unwrapped
    o0 = tr["obs"][:, 0]
    np.testing.assert_allclose(o0[:, 0] ** 2 + o0[:, 1] ** 2, 1.0, atol=1e-5)
    assert (np.abs(o0[:, 2]) <= 1.0).all()
    assert (tr["lengths"] == 200).all() and (tr["ended"] == 2).all()
    for b in range(tr["n"]):
        for t in range(0, 199):
            c, sn, thd = (float(x) for x in tr["obs"][b, t])
            u = float(tr["amu"][b, t, tr["act"][b, t], 0])
            env.reset()
            env.state = np.array([np.arctan2(sn, c), thd])
            ns, rr, dd, _ = env.step(np.array([u]))
            np.testing.assert_allclose(tr["obs"][b, t + 1], ns, rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(tr["rew"][b, t], rr, rtol=1e-4, atol=1e-5)


def test_bipedal_env_from_trace(cuda):
    tr = _traced(cuda, "bipedal")
    _check_returns(tr)
    eng = tr["eng"]
    A, Bm, wv = (x.double().cpu().numpy() for x in (eng.dynA, eng.dynB, eng.dynw))
    assert (np.abs(tr["obs"][:, 0]) < 0.6).all()   # s0 ~ N(0, 0.1): 6 sigma
    for b in range(tr["n"]):
        L = int(tr["lengths"][b])
        for t in range(L):
            s = tr["obs"][b, t].astype(np.float64)
            a = np.clip(tr["amu"][b, t, tr["act"][b, t]].astype(np.float64), -1, 1)
            rew = float(tr["rew"][b, t])
            if t + 1 < L:
                s2 = tr["obs"][b, t + 1].astype(np.float64)
                pred = np.tanh(A @ s + Bm @ a)
                assert np.abs(s2 - pred).max() < 0.06          # s' = tanh(A s + B a + N(0, 0.01))
                assert abs(s2[0]) <= 0.995 and rew > -100      # the fall rule: no fall, no end
                assert abs(rew - (0.05 * float(wv @ s2) - 0.028 * np.abs(a).sum())) < 1e-4
            else:
                assert (tr["ended"][b] == 1) == (rew == -100.0)
                assert tr["ended"][b] == 1 or L == tr["limit"]


# ------------------------------------------------------------------ 5. trace on / off, sentinels
def test_trace_off_equals_trace_on_and_sentinels(cuda):
    from apex_amd.engine.aql import AQLRolloutBuffers

    tr = _traced(cuda, "cartpole")
    eng, n, seed, limit = tr["eng"], tr["n"], tr["seed"], tr["limit"]
    h, s = eng.hip, torch.cuda.current_stream().cuda_stream
    ro = AQLRolloutBuffers(eng, eng.eval_net, n)
    ro.launch(seed, limit)                                   # trace off
    torch.cuda.synchronize()
    for k in ("returns", "lengths", "ended"):
        assert np.array_equal(getattr(ro, k).cpu().numpy(), tr[k]), k
    # a short trace, buffers two rows longer than N: exactly the first steps, the rest untouched
    short = _trace_bufs(eng, n + 2, 3)
    outs = {"returns": torch.full((n + 2,), SENT, device=eng.device),
            "lengths": torch.full((n + 2,), -7, dtype=torch.int32, device=eng.device),
            "ended": torch.full((n + 2,), -7, dtype=torch.int32, device=eng.device)}
    d = ro.descriptor(seed, limit, short, **{k: v.data_ptr() for k, v in outs.items()})
    h.aql_rollout(h.make_aql_rollout(eng.eval_net, d), s)
    torch.cuda.synchronize()
    for k in ("returns", "lengths", "ended"):
        got = outs[k].cpu().numpy()
        assert np.array_equal(got[:n], tr[k]) and (got[n:] == (SENT if k == "returns" else -7)).all(), k
    for k, v in short.items():
        got = v.cpu().numpy()
        sent = -7 if k == "act" else SENT
        assert (got[n:] == sent).all(), k                    # rows >= N
        for b in range(n):
            L = min(int(tr["lengths"][b]), 3)
            assert np.array_equal(got[b, :L], tr[k][b, :L]), k
            assert (got[b, L:] == sent).all(), k             # steps past the episode's end
    for k in ("obs", "amu", "q", "act", "rew"):              # the long trace: sentinels past each end
        sent = -7 if k == "act" else SENT
        for b in range(n):
            assert (tr[k][b, int(tr["lengths"][b]):] == sent).all(), k


# ------------------------------------------------------------------ 6. launcher validation
def test_launcher_validation(cuda):
    from apex_amd.engine.aql import AQLRolloutBuffers

    eng = _shared(cuda, "cartpole")
    h, s = eng.hip, torch.cuda.current_stream().cuda_stream
    n = 4
    ro = AQLRolloutBuffers(eng, eng.eval_net, n)
    tb = _trace_bufs(eng, n, 4)
    for t in (ro.returns, ro.lengths, ro.ended):
        t.fill_(-7)
    fused = eng.learner.fused_on
    ptrs = {k: int(t.data_ptr()) for k, t in fused._tensors.items()}
    ints = dict(obs=eng.obs, adim=eng.adim, cont=int(eng.cont), T=eng.T, na=int(eng.model.num_actions),
                uniform=int(eng.model.uniform_sample), propose=int(eng.model.propose_sample), noisy=0)
    net = lambda **o: h.make_aql_net(dict(ints, **o), ptrs)  # noqa: E731
    good = ro.descriptor(1, 20, tb)
    drop = lambda *ks: {k: v for k, v in good.items() if k not in ks}  # noqa: E731
    bad = [(eng.eval_net, dict(good, N=0)), (eng.eval_net, dict(good, N=1025)),
           (eng.eval_net, dict(good, max_steps=0)), (eng.eval_net, dict(good, max_steps=10001)),
           (eng.eval_net, dict(good, kind=3)), (eng.eval_net, dict(good, kind=-1)),
           (net(obs=0), good), (net(obs=65), good), (net(na=0), good), (net(na=65), good),
           (net(uniform=3), good),                                   # uniform > actions, discrete
           (net(T=1025), good), (net(T=4000), good),                 # a T the LDS layout cannot hold
           (eng.eval_net, dict(good, returns=0)), (eng.eval_net, dict(good, lengths=0)),
           (eng.eval_net, dict(good, ended=0)),
           (eng.eval_net, drop("trace_q")), (eng.eval_net, drop("trace_obs", "trace_amu")),
           (eng.eval_net, drop("trace_rew")), (eng.eval_net, dict(good, trace_T=0))]
    for nt, d in bad:
        with pytest.raises(ValueError):
            h.aql_rollout(h.make_aql_rollout(nt, d), s)
    torch.cuda.synchronize()
    assert (ro.returns == -7).all() and (ro.lengths == -7).all() and (ro.ended == -7).all()
    for k, v in tb.items():
        assert (v == (-7 if k == "act" else SENT)).all(), k
    h.aql_rollout(h.make_aql_rollout(net(T=500, uniform=2, propose=498), drop(
        "trace_obs", "trace_amu", "trace_q", "trace_act", "trace_rew", "trace_T")), s)   # the default 500 fits
    torch.cuda.synchronize()
    assert (ro.lengths >= 1).all()


# ------------------------------------------------------------------ 7. snapshot isolation
def test_async_evaluator_snapshot_isolation(cuda):
    from apex_amd.engine.aql import AQLEvaluator

    eng = _engine(cuda, "Pendulum-v0", fill=512, lr=0.05, **U5P3)
    ev = AQLEvaluator(eng, episodes=3, max_episode_steps=60)
    assert ev.poll() is None and ev.wait() is None
    before = eng.rollout_evaluate(3, seed=11, max_episode_steps=60)
    assert ev.launch(seed=11, tag="snap") is True
    for _ in range(50):                                       # the online weights move on, at a large lr
        eng.learner.step()
    res = ev.wait()
    assert res["tag"] == "snap" and res["returns"] == before
    assert res["lengths"] == [60] * 3 and res["ended"] == [2] * 3
    assert ev.poll() is None and ev.wait() is None            # handed over exactly once
    after = eng.rollout_evaluate(3, seed=11, max_episode_steps=60)
    assert after != before                                    # the weights did change
    flags = [ev.launch(seed=11, tag=k) for k in range(4)]     # back to back: conflated while in flight
    assert flags[0] is True
    got = []
    while (r := ev.wait()) is not None:
        got.append(r)
    assert [r["tag"] for r in got] == [k for k, f in enumerate(flags) if f]
    assert all(r["returns"] == after for r in got)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. no side effects on training
def test_async_evaluator_leaves_training_bit_identical(cuda):
    from apex_amd.engine.aql import AQLEngine, AQLEngineConfig, AQLEvaluator

    def run(with_eval):
        cfg = AQLEngineConfig(env_id="CartPole-v0", n_envs=64, capacity=8192, batch_size=32, propose_sample=3)
        eng = AQLEngine(cfg, cuda)
        eng.fill(512)
        eng.capture()
        ev = AQLEvaluator(eng, episodes=4) if with_eval else None
        for it in range(12):
            eng.iteration()
            if ev is not None and it % 3 == 2:
                ev.launch(tag=it)
        if ev is not None:
            assert ev.wait() is not None
        torch.cuda.synchronize()
        r = eng.replay
        return [eng.learner.flat, eng.learner.tflat, eng.learner.eps, r.leaf_sum, r.leaf_min, r.st, r.a_mu,
                eng.obs_buf, eng.phys, eng.ep_len, r.filled, eng.actor_ctr]

    for x, y in zip(run(False), run(True)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 9. CLI
@pytest.mark.parametrize("mode", ["host", "rollout", "async"])
def test_train_aql_eval_modes(cuda, tmp_path, mode):
    from apex_amd import train_aql

    log = tmp_path / "log.jsonl"
    a = train_aql.parser().parse_args(["--env", "CartPole-v0", "--n-envs", "64", "--capacity", "20000", "--no-tb",
                                       "--save-interval", "1000", "--save-dir", str(tmp_path), "--log-interval", "20",
                                       "--max-step", "60", "--eval-interval", "20", "--eval-episodes", "3",
                                       "--eval-mode", mode, "--json-log", str(log)])
    last = train_aql.train(a)
    recs = [json.loads(x) for x in log.read_text().splitlines()]
    assert [r["iteration"] for r in recs] == [19, 39, 59]
    base = {"iteration", "learner_steps", "loss_q", "loss_proposal", "episodes", "actor_mean_return",
            "sgd_steps_per_s", "target_syncs"}
    for r in recs:
        if mode == "async":
            assert set(r) - {"greedy_mean_return", "greedy_iteration"} == base
            assert ("greedy_mean_return" in r) == ("greedy_iteration" in r)
            if "greedy_iteration" in r:
                assert r["greedy_iteration"] % 20 == 0 and 0 < r["greedy_iteration"] <= r["iteration"]
        else:
            assert set(r) == base | {"greedy_mean_return"}     # exactly today's keys
        if "greedy_mean_return" in r:
            assert 1.0 <= r["greedy_mean_return"] <= 200.0      # CartPole-v0's possible returns
    if mode == "async":
        assert any("greedy_iteration" in r for r in recs)
        assert last["greedy_iteration"] == 60 and 1.0 <= last["greedy_mean_return"] <= 200.0   # drained at the end
