"""One-launch greedy rollouts of the vector engine (``vec_rollout``, ``rollout_evaluate``,
``VectorEvaluator``, ``train_vector --eval-mode``): bit-equality with the stepwise
``evaluate()``, the recorded trace against the host (fp64 net, envs/classic.py, the host Philox
draw), the trace switch, the launcher's validation, the evaluator's snapshot isolation and its
freedom from side effects on training, and the CLI modes.

The policies are the hand-set ones of ``tests/vector_policies.py``; the env seeds below were
chosen on the host (Philox reset draws + ``host_episodes``) so that every case shows what it is
there for: angle / seed 12 gives terminal lengths 25 to 61, two of them (25, 26) below a
limit of 30 in workgroup 0; pump / seed 13 reaches the goal in 8 of 9 episodes and runs one to
the time limit, with all three actions."""
import json

import numpy as np
import pytest
import torch

from apex_amd import envs

from . import vector_policies as vp

pytestmark = pytest.mark.gpu

Q_BOUND = 3e-6  # the project's bound for this forward against fp64 (profiles/vector_engine.md)

# name -> (recipe, env, N, max_episode_steps, policy seed, noise, env seed)
CASES = {
    "balance-v0": ("balance", "CartPole-v0", 8, None, 1, 0.02, 11),
    "angle": ("angle", "CartPole-v0", 20, None, 1, 0.02, 12),
    "pump": ("pump", "MountainCar-v0", 9, None, 20, 0.1, 13),
    "balance-v1": ("balance", "CartPole-v1", 8, None, 1, 0.02, 14),
    "angle-limit30": ("angle", "CartPole-v0", 20, 30, 1, 0.02, 12),
}


def _np(t):
    return t.detach().cpu().numpy()


def _engine(cuda, env_id, **kw):
    from apex_amd.engine.vector import VectorApexEngine, VectorEngineConfig

    cfg = VectorEngineConfig(env_id=env_id, n_envs=64, batch_size=64, replay_capacity=8192, seed=3, **kw)
    return VectorApexEngine(cfg, cuda)


@pytest.fixture(scope="module")
def engines(cuda):
    """One small engine per env, built on first use and shared (its online weights are
    overwritten by each test's policy)."""
    made = {}

    def get(env_id):
        if env_id not in made:
            made[env_id] = _engine(cuda, env_id)
        return made[env_id]

    return get


def _policy_engine(engines, name):
    recipe, env_id, N, limit, pseed, noise, seed = CASES[name]
    eng = engines(env_id)
    model = vp.make_policy(env_id, recipe, pseed, noise)
    vp.load_policy(eng, model)
    return eng, model, N, (eng.limit if limit is None else limit), seed


def _buffers(cuda, rows, T=None, obs=None, A=None):
    """Sentinel-filled outputs (and trace buffers) of ``rows`` episodes."""
    out = {"returns": torch.full((rows,), -7.0, device=cuda),
           "lengths": torch.full((rows,), -1, dtype=torch.int32, device=cuda),
           "ended": torch.full((rows,), -1, dtype=torch.int32, device=cuda)}
    if T is not None:
        out.update(trace_obs=torch.full((rows, T, obs), float("nan"), device=cuda),
                   trace_q=torch.full((rows, T, A), float("nan"), device=cuda),
                   trace_act=torch.full((rows, T), -1, dtype=torch.int32, device=cuda))
    return out


def _launch(eng, N, limit, seed, buf, override=()):
    """``vec_rollout`` straight through the binding, on the engine's online net."""
    d = dict(kind=eng.kind, N=N, obs=eng.obs_dim, max_steps=limit, seed=seed)
    d.update({k: v.data_ptr() for k, v in buf.items()})
    if "trace_obs" in buf:
        d["trace_T"] = buf["trace_obs"].shape[1]
    d.update(override)  # (None drops the entry: a null pointer)
    d = {k: v for k, v in d.items() if v is not None}
    net = d.pop("net", eng.learner.net)
    eng.hip.vec_rollout(eng.hip.make_vec_rollout(net, d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 1. bit-equality with evaluate()
@pytest.mark.parametrize("name,N", [("angle", 1), ("angle", 8), ("angle", 9), ("angle", 20), ("pump", 9),
                                    ("balance-v0", 8)])
def test_rollout_evaluate_equals_stepwise_evaluate(engines, name, N):
    """Same seed, same weights: the one-launch returns equal the stepwise evaluator's exactly.
    (``evaluate()`` explores only if a 24-bit uniform is exactly 0, 6e-8 per step; no seed used
    here hits that.)"""
    eng, _, _, _, seed = _policy_engine(engines, name)
    want = eng.evaluate(N, seed=seed)
    got = eng.rollout_evaluate(N, seed=seed)
    print(f"{name} N={N}: stepwise {want}\n{' ' * len(name)}      rollout {got}")
    assert got == want
    assert len(got) == N
    if name == "angle" and N >= 8:
        assert len(set(got)) > 1  # episodes of different lengths inside one workgroup


def test_rollout_evaluate_default_seed_and_limit(engines):
    eng, _, _, _, _ = _policy_engine(engines, "angle")
    assert eng.rollout_evaluate(5) == eng.evaluate(5)  # the same default seed derivation
    assert eng.rollout_evaluate(5, seed=12, max_episode_steps=30) == [30.0, 30.0, 30.0, 30.0, 30.0]


# ------------------------------------------------------------------ 2. trace against the host
@pytest.fixture(scope="module")
def traced(cuda, engines):
    """Every case played once with a full-length trace: numpy outputs + the policy."""
    out = {}
    for name in CASES:
        eng, model, N, limit, seed = _policy_engine(engines, name)
        buf = _buffers(cuda, N, limit, eng.obs_dim, eng.A)
        _launch(eng, N, limit, seed, buf)
        out[name] = dict({k: _np(v) for k, v in buf.items()}, model=model, N=N, limit=limit, seed=seed,
                         env_id=CASES[name][1])
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_trace_matches_host_teacher_forced(traced, name):
    """Every recorded step re-done on the host from the recorded observation (the convention
    of test_env_single_steps_match_host_dynamics).  A terminal comparison is left out only where
    the host's next state lies within 1e-4 of a threshold, and at most 1 % of the steps may be."""
    c = traced[name]
    env_id, N, limit = c["env_id"], c["N"], c["limit"]
    lengths, ended, obs, q, act = c["lengths"], c["ended"], c["trace_obs"], c["trace_q"], c["trace_act"]
    assert ((lengths >= 1) & (lengths <= limit)).all() and np.isin(ended, (1, 2)).all()
    valid = np.arange(limit)[None, :] < lengths[:, None]
    # rows past an episode's end were never written
    assert np.isnan(obs[~valid]).all() and np.isnan(q[~valid]).all() and (act[~valid] == -1).all()
    assert np.isfinite(obs[valid]).all() and np.isfinite(q[valid]).all()
    # Q at the recorded observation against the fp64 net
    with torch.no_grad():
        q64 = vp.fp64(c["model"])(torch.from_numpy(obs[valid].astype(np.float64))).numpy()
    err = float(np.abs(q[valid] - q64).max() / np.abs(q64).max())
    print(f"{name}: {int(valid.sum())} recorded steps, Q rel err {err:.3e}")
    assert err <= Q_BOUND
    # the action is the first argmax of the recorded Q (exact: np.argmax takes the first maximum)
    assert np.array_equal(act[valid], q[valid].argmax(1))
    # the reset observation is the reset formula on the host Philox draw
    assert np.abs(obs[:, 0] - vp.philox_reset_draws(env_id, c["seed"], N)).max() <= 1e-7
    env = envs.make(env_id)
    bad, left_out = [], 0
    for e in range(N):
        for t in range(lengths[e]):
            nxt, term, margin = vp.host_step(env, obs[e, t], act[e, t])
            last = t == lengths[e] - 1
            if not last and not np.allclose(obs[e, t + 1], nxt, rtol=1e-4, atol=1e-5):
                bad.append(("s'", e, t, obs[e, t + 1], nxt))
            if margin <= vp.NEAR:
                left_out += 1
                continue
            # the length is the first step at which the host says terminal or the limit is reached
            if (term or t + 1 >= limit) != last:
                bad.append(("length", e, t, term, lengths[e]))
            if last and ended[e] != (1 if term else 2):
                bad.append(("ended", e, t, term, ended[e]))
    print(f"{name}: lengths {lengths.tolist()} ended {ended.tolist()} left out {left_out}")
    assert not bad, bad[:5]
    assert left_out <= 0.01 * valid.sum()
    assert np.array_equal(c["returns"], lengths.astype(np.float32) * np.float32(vp.R_STEP[env_id]))


def test_trace_cases_cover_actions_end_kinds_and_masking(traced):
    for name, c in traced.items():
        acts = c["trace_act"][c["trace_act"] >= 0]
        assert set(np.unique(acts)) == set(range(c["trace_q"].shape[2])), name  # every action of the env
    kinds = np.concatenate([c["ended"] for c in traced.values()])
    assert (kinds == 1).any() and (kinds == 2).any()
    assert (traced["balance-v1"]["lengths"] == 500).all() and (traced["balance-v1"]["ended"] == 2).all()
    a = traced["angle"]
    assert (a["ended"] == 1).all()
    for g in range(0, a["N"], 8):  # lengths differ inside every workgroup: rows end while others run on
        assert len(set(a["lengths"][g:g + 8].tolist())) > 1
    b = traced["angle-limit30"]  # both end kinds inside workgroup 0
    assert set(b["ended"][:8].tolist()) == {1, 2} and b["lengths"].max() == 30
    # an episode cut by the limit is the uncut episode's prefix
    n = min(30, a["trace_obs"].shape[1])
    both = np.arange(n)[None, :] < np.minimum(a["lengths"], b["lengths"])[:, None]
    assert np.array_equal(a["trace_obs"][:, :n][both], b["trace_obs"][:, :n][both])


# ------------------------------------------------------------------ 3. trace off and on
def test_trace_switch_short_trace_and_rows_past_n(cuda, engines, traced):
    eng, _, _, limit, seed = _policy_engine(engines, "angle")
    N, rows, T = 9, 16, 10
    full = traced["angle"]  # (same policy, same seed: episode e is the same episode)
    plain = _buffers(cuda, rows)
    _launch(eng, N, limit, seed, plain)
    short = _buffers(cuda, rows, T, eng.obs_dim, eng.A)
    _launch(eng, N, limit, seed, short)
    for k in ("returns", "lengths", "ended"):
        got = _np(plain[k])
        assert np.array_equal(got[:N], full[k][:N]), k            # trace off = trace on
        assert np.array_equal(_np(short[k]), got), k
        assert (got[N:] == (-7.0 if k == "returns" else -1)).all(), k  # rows >= N untouched
    assert (full["lengths"][:N] > T).all()  # every episode outlasts the short trace
    for k in ("trace_obs", "trace_q", "trace_act"):
        got = _np(short[k])
        assert np.array_equal(got[:N], full[k][:N, :T]), k   # exactly the first T steps, each in its own row
        tail = got[N:]
        assert (np.isnan(tail).all() if tail.dtype.kind == "f" else (tail == -1).all()), k


# ------------------------------------------------------------------ 4. validation
@pytest.mark.parametrize("bad", [
    dict(N=0), dict(N=1025), dict(max_steps=0), dict(max_steps=10001), dict(kind=2), dict(kind=-1),
    dict(kind=1), dict(obs=2), dict(returns=None), dict(lengths=None), dict(ended=None),
    dict(trace_q=None), dict(trace_obs=None, trace_act=None), dict(trace_T=0), dict(net="A8"), dict(net="null"),
])
def test_launcher_rejects_before_any_launch(cuda, engines, bad):
    eng, _, _, limit, seed = _policy_engine(engines, "angle")
    buf = _buffers(cuda, 8, 4, eng.obs_dim, eng.A)
    before = {k: v.clone() for k, v in buf.items()}
    if "net" in bad:
        from apex_amd.engine.vector import PARAM_KEYS

        d = {k: p.data_ptr() for k, p in eng.learner.model.named_parameters()}
        if bad["net"] == "null":
            d[PARAM_KEYS[4]] = 0
        bad = dict(net=eng.hip.make_vec_net(dict(d, obs=4, A=8 if bad["net"] == "A8" else 2)))
    with pytest.raises(ValueError):
        _launch(eng, 8, limit, seed, buf, bad)
    torch.cuda.synchronize()
    for k, v in buf.items():  # (the float sentinels are NaN: compare them as a number)
        assert torch.equal(v.float().nan_to_num(nan=123.0), before[k].float().nan_to_num(nan=123.0)), k


# ------------------------------------------------------------------ 5. snapshot isolation
def _sync_rollout(eng, weights, n, seed):
    """Synchronous rollout of ``weights`` (then the engine's own weights are put back)."""
    keep = eng.learner.flat.clone()
    eng.learner.flat.copy_(weights)
    out = eng.rollout_evaluate(n, seed=seed)
    eng.learner.flat.copy_(keep)
    return out


def test_evaluator_plays_its_snapshot_while_training_goes_on(cuda):
    from apex_amd.engine import VectorEvaluator

    # lr: RMSprop moves every weight by about lr per step, so 50 steps at 1e-2 redraw the policy
    eng = _engine(cuda, "CartPole-v0", lr=1e-2)
    vp.load_policy(eng, vp.make_policy("CartPole-v0", "angle", 1, 0.02))
    eng.publish_params()
    eng.fill()
    ev = VectorEvaluator(eng, episodes=10)
    assert ev.poll() is None and ev.wait() is None
    w0 = eng.learner.flat.clone()
    assert ev.launch(seed=12, tag=7) is True
    for _ in range(50):  # at once: the weights change under the running rollout
        eng.train_step()
    res = ev.wait()
    assert ev.poll() is None and ev.wait() is None  # handed over once
    w1 = eng.learner.flat.clone()
    assert not torch.equal(w0, w1)
    want0, want1 = _sync_rollout(eng, w0, 10, 12), _sync_rollout(eng, w1, 10, 12)
    print("snapshot", want0, "after 50 steps", want1, "evaluator", res)
    assert res["tag"] == 7
    assert res["returns"] == want0
    assert want1 != want0 and res["returns"] != want1
    assert res["lengths"] == [int(r) for r in want0] and set(res["ended"]) <= {1, 2}
    # back to back: the second launch may or may not find the first one landed
    snaps = {}
    flags = []
    for tag, seed in (("a", 21), ("b", 22)):
        flags.append(ev.launch(seed=seed, tag=tag))
        snaps[tag] = (eng.learner.flat.clone(), seed)
        for _ in range(3):
            eng.train_step()
    assert flags[0] is True
    got = []
    while (r := ev.wait()) is not None:
        got.append(r)
    assert len(got) == sum(flags)
    assert [r["tag"] for r in got] == [t for t, f in zip("ab", flags) if f]
    for r in got:
        w, seed = snaps[r["tag"]]
        assert r["returns"] == _sync_rollout(eng, w, 10, seed), r["tag"]


# ------------------------------------------------------------------ 6. no side effects on training
def test_evaluator_leaves_training_bit_identical(cuda):
    from apex_amd.engine import VectorEvaluator

    ends = []
    launched = 0
    for with_eval in (False, True):
        eng = _engine(cuda, "CartPole-v0", lr=1e-3)
        eng.fill()
        eng.capture(warmup_iters=3)
        ev = VectorEvaluator(eng, episodes=10) if with_eval else None
        s0 = eng.learn_steps
        while eng.learn_steps < s0 + 40:
            eng.train_step()
            if ev is not None and (eng.learn_steps - s0) % 10 == 0:
                launched += ev.launch(tag=eng.learn_steps)
        if ev is not None:
            landed = 0
            while ev.wait() is not None:
                landed += 1
            assert landed == launched >= 1
        torch.cuda.synchronize()
        ends.append((eng.learner.flat.clone(), eng.replay.leaf_sum.clone(), eng.shard.env_state.clone(),
                     eng.replay.filled.clone()))
    for x, y in zip(*ends):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 7. CLI
TODAY_KEYS = {"step", "loss", "grad_norm", "grad_norm_l2", "lr", "sgd_steps_per_s", "env_steps_per_s", "episodes",
              "actor_mean_return", "greedy_mean_return"}


def _cli(tmp_path, capsys, *extra):
    from apex_amd import train_vector

    args = ["--max-step", "200", "--eval-interval", "50", "--log-interval", "50", "--envs", "64", "--capacity", "8192",
            "--save-dir", str(tmp_path), *extra]
    capsys.readouterr()
    last = train_vector.train(train_vector.parser().parse_args(args))
    recs = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert recs and recs[-1] == last
    return recs


def test_cli_async_mode_reports_snapshot_steps(cuda, tmp_path, capsys):
    recs = _cli(tmp_path, capsys, "--eval-mode", "async")
    assert [r["step"] for r in recs] == [50, 100, 150, 200]  # an evaluation forces no line of its own
    for r in recs:
        assert ("greedy_mean_return" in r) == ("greedy_step" in r)
        if "greedy_step" in r:
            assert r["greedy_step"] % 50 == 0 and 0 < r["greedy_step"] <= r["step"]
            assert -200.0 <= r["greedy_mean_return"] <= -1.0  # MountainCar-v0
            assert set(r) == TODAY_KEYS | {"greedy_step"}
    assert recs[-1]["greedy_step"] == 200


@pytest.mark.parametrize("mode", [(), ("--eval-mode", "rollout")])
def test_cli_step_and_rollout_modes_keep_todays_keys(cuda, tmp_path, capsys, mode):
    recs = _cli(tmp_path, capsys, *mode)
    assert [r["step"] for r in recs] == [50, 100, 150, 200]
    for r in recs:
        assert set(r) == TODAY_KEYS
        assert -200.0 <= r["greedy_mean_return"] <= -1.0
