"""Greedy evaluation on host envs beside the host-env AQL engine (``engine/aql_host_eval.py``):
the one-launch act ``aql_host_eval_act`` against the three stepwise kernels, against ``aql_rollout``'s
trace and against the fp64 eval-mode critic; the two weight sets; the worker pool against the
in-process vector; training left bit-identical; the launcher's limits; the command line."""
import copy
import json
import multiprocessing as mp
import time

import numpy as np
import pytest
import torch

from . import aql_rollout_fixtures as rfx
from .aql_host_fixtures import ScriptedVec

pytestmark = pytest.mark.gpu

STEPS = 12
T51 = dict(uniform_sample=50, propose_sample=1)
# shape: (obs, continuous, action_dim, n_actions, low, high, candidate kwargs); T = 51 is no multiple of the
# kernel's 8 waves, T = 8 is one candidate per wave
SHAPES = {"pendulum": (3, True, 1, 1, [-2.0], [2.0], T51),
          "bipedal": (24, True, 4, 4, [-1.0] * 4, [1.0] * 4, T51),
          "cartpole": (4, False, 1, 2, None, None, dict(uniform_sample=2, propose_sample=49)),
          "mountaincar": (2, True, 1, 1, [-1.0], [1.0], T51),
          "pendulum8": (3, True, 1, 1, [-2.0], [2.0], dict(uniform_sample=5, propose_sample=3)),
          # past 24 observation floats the kernel takes its other instance (wider input layers, one candidate per pass)
          "wide": (33, True, 2, 2, [-1.0, -0.5], [1.0, 0.5], T51)}
_ENGINES = {}


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)


def _cfg(env_id, **kw):
    from apex_amd.engine.aql import AQLEngineConfig

    base = dict(env_id=env_id, n_envs=4, capacity=100, batch_size=8, seed=3, learner_steps=2, max_step=40)
    base.update(kw)
    return AQLEngineConfig(**base)


def _script(shape, n, steps=STEPS, seed=0):
    obs = SHAPES[shape][0]
    rng = np.random.default_rng(100 + seed)
    first = rng.uniform(-1, 1, (n, obs)).astype(np.float32)
    out = []
    for _ in range(steps):
        o = rng.uniform(-1, 1, (n, obs)).astype(np.float32)
        out.append(dict(next_obs=o, reset_obs=o, reward=rng.uniform(-1, 1, n).astype(np.float32),
                        done=np.zeros(n, np.float32), ended=np.zeros(n, np.float32)))
    return first, out


def _vec(shape, first, steps):
    _, cont, adim, na, low, high, _ = SHAPES[shape]
    return ScriptedVec(first, steps, cont, adim, na, low, high)


def _engine(cuda, shape):
    """One host-env engine per shape over a scripted vector (shared; its weights are the rollout
    fixtures': non-zero biases, non-zero NoisyNet sigma and epsilon)."""
    if shape not in _ENGINES:
        from apex_amd.engine.aql_host import AQLHostEngine

        obs = SHAPES[shape][0]
        eng = AQLHostEngine(_cfg("scripted", **SHAPES[shape][6]), _vec(shape, np.zeros((4, obs), np.float32), []), cuda)
        rfx.set_params(eng.model)
        eng.learner.sync_target()
        eng.publish()
        torch.cuda.synchronize()
        _ENGINES[shape] = eng
    return _ENGINES[shape]


def _play(ev, steps=STEPS):
    """``steps`` blocking evaluator steps; the device outputs after each act."""
    tape = []
    for _ in range(steps):
        ev.step_begin()
        ev.stream.synchronize()
        tape.append({k: getattr(ev, k).detach().cpu().clone() for k in ("env_act", "act_idx", "counter", "amu", "q")})
        ev.step_end()
    return tape


def _same(a, b, keys=("env_act", "act_idx", "counter", "amu", "q")):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


# ------------------------------------------------------------------ 1. fused == step
@pytest.mark.parametrize("shape", ["pendulum", "bipedal", "cartpole", "mountaincar", "pendulum8", "wide"])
@pytest.mark.parametrize("n", [1, 3])
def test_fused_equals_step(cuda, shape, n):
    from apex_amd.engine.aql_host_eval import AQLHostEvaluator

    eng = _engine(cuda, shape)
    assert eng.T == (8 if shape == "pendulum8" else 51)
    first, steps = _script(shape, n)
    tapes = {}
    for kernel in ("fused", "step"):
        ev = AQLHostEvaluator(eng, _vec(shape, first, steps), kernel=kernel, seed=11, trace=True)
        tapes[kernel] = _play(ev)
        assert ev.ledger.steps == STEPS and ev.k == STEPS
        ev.close()
        ev.close()
    for t, (a, b) in enumerate(zip(tapes["fused"], tapes["step"])):
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (t, k)
        assert int(a["counter"]) == t + 1
        idx = a["act_idx"].long()
        assert ((0 <= idx) & (idx < eng.T)).all()
        assert torch.equal(a["env_act"], a["amu"][torch.arange(n), idx])      # env_act = cand[arg]
        assert np.array_equal(idx.numpy(), np.argmax(a["q"].numpy(), axis=1))   # eps 0: the first argmax
    assert not torch.equal(tapes["fused"][0]["q"], tapes["fused"][1]["q"])  # the observations matter
    if SHAPES[shape][1]:   # the uniform candidates lie within the action bounds (the proposed ones are not clipped)
        U = int(eng.model.uniform_sample)
        uni = torch.stack([x["amu"][:, :U] for x in tapes["fused"]])
        lo, hi = torch.tensor(SHAPES[shape][4]), torch.tensor(SHAPES[shape][5])
        assert (uni >= lo).all() and (uni <= hi).all()


def test_untraced_fused_act_equals_the_traced_one(cuda):
    from apex_amd.engine.aql_host_eval import AQLHostEvaluator

    eng = _engine(cuda, "pendulum")
    first, steps = _script("pendulum", 3)
    a = AQLHostEvaluator(eng, _vec("pendulum", first, steps), seed=11, trace=True)
    b = AQLHostEvaluator(eng, _vec("pendulum", first, steps), seed=11)
    for x, y in zip(_play(a, 4), _play(b, 4)):
        assert _same(x, y, ("env_act", "act_idx", "counter"))
        assert not y["amu"].any() and not y["q"].any()                       # no trace: never written
    a.close()
    b.close()


# ------------------------------------------------------------------ 2. tape against aql_rollout
def test_tape_equals_aql_rollout_trace(cuda):
    from apex_amd.engine.aql import AQLEngine, AQLEngineConfig, AQLRolloutBuffers
    from apex_amd.engine.aql_host_eval import AQLHostEvaluator
    from apex_amd.engine.host_eval import eval_seed

    n, Tr = 3, STEPS
    cfg = AQLEngineConfig(env_id="CartPole-v0", n_envs=64, capacity=8192, batch_size=32, use_graphs=False,
                          propose_sample=49)
    eng = AQLEngine(cfg, cuda)
    rfx.set_params(eng.model)
    eng.learner.sync_target()
    eng.publish()
    assert eng.T == 51
    f = lambda *s: torch.full(s, -12345.0, dtype=torch.float32, device=cuda)  # noqa: E731
    ro = AQLRolloutBuffers(eng, eng.eval_net, n)
    seed = 0    # (its three greedy episodes last 8, 9 and 10 steps with these weights: aql_rollout's own lengths)
    sd = eval_seed(seed) & 0xFFFFFFFFFFFF
    tr = dict(obs=f(n, Tr, eng.obs), amu=f(n, Tr, eng.T, eng.adim), q=f(n, Tr, eng.T),
              act=torch.full((n, Tr), -7, dtype=torch.int32, device=cuda), rew=f(n, Tr))
    ro.launch(sd, eng.eval_limit, tr)
    torch.cuda.synchronize()
    lengths = ro.lengths.cpu().numpy()
    print("seed", seed, "lengths", lengths.tolist())
    assert lengths.min() >= 8, lengths          # every env contributes at least 8 compared steps
    tr = {k: v.cpu().numpy() for k, v in tr.items()}
    L = np.minimum(lengths, Tr)
    steps = []
    for t in range(Tr):
        nxt = np.zeros((n, eng.obs), np.float32)
        for b in range(n):
            if t + 1 < L[b]:
                nxt[b] = tr["obs"][b, t + 1]
        steps.append(dict(next_obs=nxt, reset_obs=nxt, reward=np.ones(n, np.float32), done=np.zeros(n, np.float32),
                          ended=np.zeros(n, np.float32)))
    vec = ScriptedVec(tr["obs"][:, 0], steps, False, 1, 2)
    ev = AQLHostEvaluator(eng, vec, kernel="fused", seed=seed, trace=True)
    assert ev.sd == sd
    compared = np.zeros(n, np.int64)
    for t, x in enumerate(_play(ev, Tr)):
        for b in range(n):
            if t >= L[b]:
                continue
            compared[b] += 1
            arg = int(tr["act"][b, t])
            assert np.array_equal(_bits(x["amu"][b]), _bits(tr["amu"][b, t])), (t, b)
            assert np.array_equal(_bits(x["q"][b]), _bits(tr["q"][b, t])), (t, b)
            assert int(x["act_idx"][b]) == arg, (t, b)
            assert np.array_equal(_bits(x["env_act"][b]), _bits(tr["amu"][b, t, arg])), (t, b)
    assert (compared >= 8).all(), compared
    ev.close()


# ------------------------------------------------------------------ 3. Q against fp64
@pytest.mark.parametrize("shape", ["bipedal", "cartpole", "wide"])
def test_traced_q_is_the_eval_mode_fp64_q(cuda, shape):
    from apex_amd.engine.aql_host_eval import AQLHostEvaluator

    eng = _engine(cuda, shape)
    n = 3
    first, steps = _script(shape, n)
    ev = AQLHostEvaluator(eng, _vec(shape, first, steps), seed=5, trace=True)
    x = _play(ev, 2)[1]
    ev.close()
    obs = torch.as_tensor(steps[0]["reset_obs"], dtype=torch.float64, device=cuda)
    am = x["amu"].to(device=cuda, dtype=torch.float64)
    q32 = x["q"].to(device=cuda, dtype=torch.float64)
    ref = copy.deepcopy(eng.model).double()
    T = eng.T

    def q64(mode_train):
        ref.q.train(mode_train)
        with torch.no_grad():
            qn = ref.q
            a_out = qn.action_out(am.reshape(n * T, eng.adim)).reshape(n, T, qn.A_OUT)
            q_f = qn.q_feature(obs).repeat(1, T).reshape(n, T, qn.F_OUT)
            return qn.forward(torch.relu(torch.cat([a_out, q_f], dim=2))).reshape(n, T)

    means, noisy = q64(False), q64(True)
    err = float((q32 - means).abs().max() / means.abs().max().clamp_min(1e-30))
    err_noisy = float((q32 - noisy).abs().max() / noisy.abs().max().clamp_min(1e-30))
    print(shape, "rel err vs means", err, "vs noisy", err_noisy)
    assert err < 1e-5, err                      # test_trace_q_is_the_eval_mode_fp64_q's bound for this forward
    assert err_noisy > 1e-3, err_noisy          # the test tells the two apart


# ------------------------------------------------------------------ 4. weight sets
def test_refresh_switches_the_weight_set_between_two_acts(cuda):
    from apex_amd.engine.aql_host_eval import AQLHostEvaluator

    eng = _engine(cuda, "pendulum")
    flat = eng.learner.flat
    old = flat.clone()
    first, steps = _script("pendulum", 3)
    mk = lambda: AQLHostEvaluator(eng, _vec("pendulum", first, steps), seed=2, trace=True)  # noqa: E731
    try:
        ev, ev_old = mk(), mk()
        got = _play(ev, 2)
        rfx.set_params(eng.model, seed=9)              # the online parameters move on
        torch.cuda.synchronize()
        new = flat.clone()
        assert not torch.equal(old, new)
        assert ev.refresh(flat) is True
        got += _play(ev, 1)
        want_old = _play(ev_old, 3)                    # never refreshed: the old parameters throughout
        want_new = _play(mk(), 3)                      # a fresh evaluator on the new parameters
        assert _same(got[0], want_old[0]) and _same(got[1], want_old[1])      # the acts before the refresh
        assert _same(got[2], want_new[2])                                      # the act after it
        assert not _same(got[2], want_old[2], ("q",))
        cur = ev.weights.cur
        assert cur == 1 and ev.weights.refreshes == 1
        assert torch.equal(ev.flats[cur], new) and torch.equal(ev.flats[1 - cur], old)
        assert torch.equal(ev_old.flats[0], old) and torch.equal(ev_old.flats[1], old)
        ev.close()
        ev_old.close()
    finally:
        flat.copy_(old)
        torch.cuda.synchronize()


# ------------------------------------------------------------------ 5. pool == in-process
def test_pool_evaluation_equals_the_in_process_run(cuda):
    from apex_amd.engine.aql_host_eval import AQLHostEvaluation, AQLHostEvaluator, make_pool
    from apex_amd.engine.host_eval import eval_seed
    from apex_amd.envs.host_vector import HostVectorEnv

    eng = _engine(cuda, "pendulum")
    seed, n, cap, want_n = 4, 3, 20, 6
    vec = HostVectorEnv("Pendulum-v0", n, seed=eval_seed(seed), max_episode_length=cap)
    ref = AQLHostEvaluator(eng, vec, seed=seed)
    ref.run(2 * cap)
    want = [e[:3] for e in ref.poll()]
    ref.close()
    vec.close()
    assert len(want) == want_n and all(e[1] == cap and e[2] for e in want)    # Pendulum never terminates: capped
    pool = make_pool("Pendulum-v0", n, 2, seed=seed, max_episode_length=cap, timeout=30.0)
    drv = AQLHostEvaluation(AQLHostEvaluator(eng, pool, seed=seed), pool)
    got, deadline = [], time.monotonic() + 60.0
    try:
        while len(got) < want_n:
            assert time.monotonic() < deadline, (len(got), drv.pumps)
            drv.pump(learn_step=7)
            got += drv.poll()
    finally:
        drv.close()
        drv.close()
    print("pumps", drv.pumps, "evaluator steps", drv.ev.ledger.steps)
    assert [e[:3] for e in got[:want_n]] == want and all(e[3] == 7 for e in got)
    assert all(not p.is_alive() for p in pool.processes)


# ------------------------------------------------------------------ 6. training untouched
def test_evaluator_leaves_training_bit_identical(cuda):
    from apex_amd.engine.aql_host import AQLHostEngine
    from apex_amd.engine.aql_host_eval import AQLHostEvaluation, AQLHostEvaluator, make_pool
    from apex_amd.envs.host_vector import HostVectorEnv

    def run(with_eval):
        vec = HostVectorEnv("Pendulum-v0", 4, seed=3)
        eng = AQLHostEngine(_cfg("Pendulum-v0"), vec, cuda)
        assert eng.K == 2
        eng.fill()
        eng.capture()
        drv = None
        if with_eval:
            pool = make_pool("Pendulum-v0", 2, 1, seed=3, max_episode_length=20, timeout=30.0)
            drv = AQLHostEvaluation(AQLHostEvaluator(eng, pool, seed=3), pool)
        try:
            for it in range(8):
                eng.iteration()
                if drv is not None:
                    if it % 2 == 1:
                        drv.refresh(eng.learner.flat)
                    drv.pump(eng.learner_steps)
            torch.cuda.synchronize()
            if drv is not None:
                print("evaluator steps", drv.ev.ledger.steps, "refreshes", drv.ev.weights.refreshes)
                assert drv.ev.weights.refreshes >= 1 and drv.ev.k >= 1
        finally:
            if drv is not None:
                drv.close()
        r, L = eng.replay, eng.learner
        out = [L.flat, L.m, L.v, L.step_ctr, L.tflat, L.eps, r.st, r.st2, r.action, r.reward, r.done, r.a_mu,
               r.leaf_sum, r.leaf_min, r.node_sum[0], r.node_sum[-1], r.filled, eng.actor_ctr, eng.obs_buf]
        out = [x.detach().cpu().clone() for x in out]
        eng.close()
        return out

    a, b = run(False), run(True)
    assert int(a[3]) == 16                       # 8 iterations of K = 2 SGD steps
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(_bits(x), _bits(y)), i


# ------------------------------------------------------------------ 7. launcher limits
def test_launcher_limits(cuda):
    from apex_amd.engine.aql_host_eval import AQLHostEvaluator

    eng = _engine(cuda, "pendulum")
    h, s = eng.hip, torch.cuda.current_stream().cuda_stream
    n = 3
    first, steps = _script("pendulum", n)
    ev = AQLHostEvaluator(eng, _vec("pendulum", first, steps), seed=1, trace=True)
    outs = (ev.env_act, ev.act_idx, ev.counter, ev.amu, ev.q)
    for t in outs:
        t.fill_(-7)
    ptrs = {k: int(t.data_ptr()) for k, t in ev._fused[0]._tensors.items()}
    ints = dict(obs=eng.obs, adim=eng.adim, cont=1, T=eng.T, na=1, uniform=int(eng.model.uniform_sample),
                propose=int(eng.model.propose_sample), noisy=0)
    net = lambda p=ptrs, **o: h.make_aql_net(dict(ints, **o), p)  # noqa: E731
    good_net = ev.nets[0]
    good = dict(N=n, prop_seed=ev.prop_seed, sel_seed=ev.sel_seed, stage=ev.stage_dev.data_ptr(),
                low=eng.low.data_ptr(), high=eng.high.data_ptr(), var=eng.var.data_ptr(),
                env_act=ev.env_act.data_ptr(), act_idx=ev.act_idx.data_ptr(), counter=ev.counter.data_ptr(),
                amu=ev.amu.data_ptr(), q=ev.q.data_ptr())
    drop = lambda *ks: {k: v for k, v in good.items() if k not in ks}  # noqa: E731
    G = None   # (the evaluator's own handle)
    bad = [(G, dict(good, N=0)), (G, dict(good, N=65)), (G, dict(good, N=-1)),
           (dict(obs=0), good), (dict(obs=65), good), (dict(na=0, adim=0), good), (dict(na=65, adim=65), good),
           (dict(cont=0, na=0), good), (dict(cont=0, na=65), good),          # the action count, discrete
           (dict(adim=0), good), (dict(adim=9, na=9), good),
           (dict(T=1025), good), (dict(T=1000, adim=4, na=4), good),         # 1000 * 5 > 4608 LDS floats
           (dict(cont=0, na=2, uniform=3), good),                            # uniform > actions, discrete
           (G, drop("env_act")), (G, drop("act_idx")), (G, drop("counter")), (G, drop("stage")),
           (G, drop("amu")), (G, drop("q")),                                 # a partial trace
           (dict(p=dict(ptrs, df_w1=ptrs["df_w1"] + 4)), good),              # dist_feature.0 not 16-byte aligned
           (G, drop("low")), (G, drop("high")), (G, drop("var"))]
    for kw, d in bad:
        with pytest.raises((ValueError, RuntimeError)):   # (an action dim of 0 is already refused by make_aql_net)
            h.aql_host_eval_act(h.make_aql_host_eval_act(good_net if kw is None else net(**kw), d), 0, s)
    with pytest.raises((ValueError, RuntimeError)):
        h.aql_host_eval_act(h.make_aql_host_eval_act(good_net, good), -1, s)
    torch.cuda.synchronize()
    for t in outs:
        assert (t == -7).all()                                               # none of them reached the GPU
    h.aql_host_eval_act(h.make_aql_host_eval_act(good_net, good), 0, s)      # the good descriptor runs
    h.aql_host_eval_act(h.make_aql_host_eval_act(net(T=500, uniform=499, propose=1), dict(drop("amu", "q"), N=1)), 0, s)
    torch.cuda.synchronize()
    assert int(ev.counter) == 1 and (ev.act_idx[1:] < eng.T).all() and (ev.act_idx >= 0).all()
    ev.close()
    with pytest.raises(ValueError, match="64"):
        AQLHostEvaluator(eng, _vec("pendulum", np.zeros((65, 3), np.float32), []))
    with pytest.raises(ValueError, match="kernel"):
        AQLHostEvaluator(eng, _vec("pendulum", first, steps), kernel="graph")
    with pytest.raises(ValueError, match="differ"):
        AQLHostEvaluator(eng, _vec("mountaincar", np.zeros((2, 2), np.float32), []))


# ------------------------------------------------------------------ 8. command line
BASE = ["--host-envs", "--env", "Pendulum-v0", "--n-envs", "4", "--eval-envs", "2", "--eval-workers", "1",
        "--eval-interval", "2", "--max-episode-length", "20"]


def test_cli_writes_evaluator_episodes_and_leaves_no_process(cuda, tmp_path, monkeypatch):
    from apex_amd import train_aql

    scalars = []

    class Writer(train_aql.NullWriter):
        def add_scalar(self, tag, value, step=None, *a, **k):
            scalars.append((tag, float(value), step))

    monkeypatch.setattr(train_aql, "NullWriter", Writer)
    monkeypatch.setattr(train_aql, "greedy_eval", lambda *a, **k: pytest.fail("greedy_eval was called"))
    log = tmp_path / "log.jsonl"
    a = train_aql.parser().parse_args(BASE + ["--max-step", "300", "--batch-size", "8", "--capacity", "2000",
                                              "--no-tb", "--save-interval", "1000", "--save-dir", str(tmp_path),
                                              "--log-interval", "50", "--json-log", str(log)])
    assert a.eval_kernel in ("fused", "step")
    last = train_aql.train(a)
    recs = [json.loads(x) for x in log.read_text().splitlines()]
    print([(r["iteration"], r["evaluator_episodes"], r["evaluator_steps"]) for r in recs])
    assert recs[-1]["iteration"] == 299 and last["evaluator_steps"] == recs[-1]["evaluator_steps"]
    rewards = [(v, st) for tag, v, st in scalars if tag == "evaluator/episode_reward"]
    lengths = [v for tag, v, st in scalars if tag == "evaluator/episode_length"]
    assert len(rewards) >= 1 and len(rewards) == len(lengths) == sum(r["evaluator_episodes"] for r in recs)
    assert all(x == 20.0 for x in lengths)                          # Pendulum under the 20-step cap
    assert all(-17.0 * 20 <= v <= 0.0 and 0 <= st <= last["learner_steps"] for v, st in rewards)
    assert all("greedy_mean_return" not in r for r in recs)
    assert mp.active_children() == []                               # the evaluator's workers are gone


@pytest.mark.parametrize("argv", [
    ["--env", "Pendulum-v0", "--eval-envs", "2", "--eval-interval", "2"],                      # no --host-envs
    ["--host-envs", "--eval-envs", "2", "--eval-interval", "2", "--gpus", "2"],
    ["--host-envs", "--eval-envs", "2", "--eval-interval", "2", "--eval-workers", "3"],
    ["--host-envs", "--eval-envs", "2", "--eval-interval", "2", "--eval-workers", "0"],
    ["--host-envs", "--eval-envs", "2", "--eval-interval", "0"],
    ["--host-envs", "--eval-envs", "2"],                                                       # (the default interval is 0)
    ["--host-envs", "--eval-envs", "65", "--eval-interval", "2"],
    ["--host-envs", "--eval-envs", "-1", "--eval-interval", "2"],
    ["--host-envs", "--eval-workers", "1"]])
def test_cli_parser_errors(argv):
    from apex_amd import train_aql

    with pytest.raises(SystemExit):
        train_aql.parser().parse_args(argv)
    ok = train_aql.parser().parse_args(BASE)
    assert (ok.eval_envs, ok.eval_workers, ok.eval_interval) == (2, 1, 2)
    assert train_aql.parser().parse_args(["--host-envs", "--eval-envs", "5", "--eval-interval", "1"]).eval_workers == 2
