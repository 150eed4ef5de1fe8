"""Greedy evaluation on host envs beside the host-env vector engine (``engine/vector_host_eval.py``):
the one-launch act ``vec_host_eval_act`` against the stepwise kernels, against the fp64 net and
against ``vec_rollout``'s trace; the two weight sets; the worker pool against the in-process
vector; training left bit-identical; the launcher's limits; the command line."""
import json
import multiprocessing as mp
import time

import numpy as np
import pytest
import torch

from apex_amd.envs.host_vector import staging_views

from . import vector_policies as vp
from .actor_oracle import select_actions_ref

pytestmark = pytest.mark.gpu

STEPS = 12
Q_BOUND = 3e-6   # tests/test_gpu_vector_engine.py: measured 1.32e-6 for this forward, max|x - ref| / max|ref|
Q_SENT, A_SENT = -12345.0, -77
# (obs, actions): CartPole, MountainCar, Acrobot's shapes, the kernels' limits, the smallest net
SHAPES = [(4, 2), (2, 3), (6, 3), (8, 7), (1, 1)]
_ENGINES = {}


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)


class Tape:
    """The ``HostVectorEnv`` protocol over a list of prepared steps (the style of
    ``vector_host_fixtures.TapeVectorEnv``, with the whole block scripted): a step is a dict with
    ``next_obs`` / ``reset_obs`` [N, obs] and ``reward`` / ``done`` / ``ended`` [N]."""

    continuous = False
    action_dim = 1

    def __init__(self, first_obs, steps, n_actions):
        first_obs = np.asarray(first_obs, dtype=np.float32)
        self.n, self.obs_dim = first_obs.shape
        self.first_obs, self.steps, self.t = first_obs, steps, 0
        self.n_actions = int(n_actions)
        self.staging = np.zeros(self.n * (2 * self.obs_dim + 3), dtype=np.float32)
        self.views = staging_views(self.staging, self.n, self.obs_dim)
        self.received = []

    def __len__(self):
        return self.n

    def reset(self):
        self.views["reset_obs"][:] = self.first_obs
        return self.views["reset_obs"]

    def step(self, actions):
        a = np.asarray(actions)
        assert a.shape == (self.n,) and a.dtype == np.int32
        assert ((0 <= a) & (a < self.n_actions)).all(), a
        self.received.append(a.copy())
        for k, v in self.steps[self.t].items():
            self.views[k][:] = v
        self.t += 1


def _script(obs, n, steps=STEPS, seed=0):
    """Observations uniform in [-1, 1]; every step mixes env ends (``done``), cap resets
    (``ended`` with ``done = 0``) and running episodes; where an episode ended ``reset_obs`` is a
    fresh draw, not ``next_obs``."""
    rng = np.random.default_rng(1000 * obs + 10 * n + seed)
    first = rng.uniform(-1, 1, (n, obs)).astype(np.float32)
    out = []
    for t in range(steps):
        nxt = rng.uniform(-1, 1, (n, obs)).astype(np.float32)
        fresh = rng.uniform(-1, 1, (n, obs)).astype(np.float32)
        kind = (np.arange(n) + t) % 3 if n > 1 else np.full(1, t % 3)   # 0 runs on, 1 done, 2 cap reset
        ended = (kind > 0).astype(np.float32)
        done = (kind == 1).astype(np.float32)
        out.append(dict(next_obs=nxt, reset_obs=np.where(ended[:, None] > 0, fresh, nxt),
                        reward=rng.uniform(-1, 1, n).astype(np.float32), done=done, ended=ended))
    return first, out


def set_params(model, seed=1):
    """Every parameter re-drawn, in place (the flat storage stays): the init's biases are zero."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            fan_in = p.shape[1] if p.dim() == 2 else 4
            s = 0.5 if name.endswith("bias") else 1.0 / fan_in ** 0.5
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * s)


class _Learner:
    def __init__(self, hip, model):
        self.hip, self.model = hip, model
        self.flat = model.flatten_parameters()
        self.P = self.flat.numel()

    def copy_params_to(self, dst_flat):
        self.hip.copy_f32(dst_flat.data_ptr(), self.flat.data_ptr(), self.P, torch.cuda.current_stream().cuda_stream)


class _BareEngine:
    """What the evaluator reads of a ``VectorHostEngine``, for the (1, 1) net: no env in the tree
    has one observation float and one action, and the engine's replay is not what is under test."""

    def __init__(self, cuda, obs, A):
        from apex_amd import ops
        from apex_amd.models.dqn import DuelingDQN

        self.hip, self.device, self.obs_dim, self.A = ops.hip(), torch.device(cuda), obs, A
        self.learner = _Learner(self.hip, DuelingDQN.from_shapes((obs,), A).to(cuda))

    def close(self):
        pass


def _cfg(env_id, E, **kw):
    from apex_amd.engine.vector import VectorEngineConfig

    base = dict(env_id=env_id, n_envs=E, batch_size=16, replay_capacity=4096, lr=1e-3, seed=3,
                publish_param_interval=8, target_update_interval=100)
    base.update(kw)
    return VectorEngineConfig(**base)


def _engine(cuda, obs, A):
    """One host-env engine per shape over an idle tape (shared; non-zero biases)."""
    if (obs, A) not in _ENGINES:
        from apex_amd.engine.vector_host import VectorHostEngine

        if (obs, A) == (1, 1):
            eng = _BareEngine(cuda, obs, A)
        else:
            eng = VectorHostEngine(_cfg("scripted", 4), Tape(np.zeros((4, obs), np.float32), [], A), cuda)
        set_params(eng.learner.model, seed=1 + obs)
        torch.cuda.synchronize()
        _ENGINES[(obs, A)] = eng
    return _ENGINES[(obs, A)]


def _guarded(ev):
    """Re-seat ``q`` and ``actions`` inside sentinel-filled buffers with guard elements behind."""
    qg = torch.full((ev.N + 3, ev.A), Q_SENT, dtype=torch.float32, device=ev.device)
    ag = torch.full((ev.N + 5,), A_SENT, dtype=torch.int32, device=ev.device)
    ev.q, ev.actions = qg[:ev.N], ag[:ev.N]
    ev._bind()
    torch.cuda.synchronize()
    return qg, ag


def _play(ev, steps=STEPS, guards=None):
    """``steps`` blocking evaluator steps; ``q`` and ``actions`` after each act."""
    tape = []
    for _ in range(steps):
        ev.step_begin()
        ev.stream.synchronize()
        tape.append(dict(q=ev.q.detach().cpu().clone(), actions=ev.actions.detach().cpu().clone()))
        if guards is not None:
            qg, ag = guards
            assert (qg[ev.N:] == Q_SENT).all() and (ag[ev.N:] == A_SENT).all()
        ev.step_end()
    return tape


def _same(a, b, keys=("q", "actions")):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


# ------------------------------------------------------------------ 1. fused == step
@pytest.mark.parametrize("obs,A", SHAPES)
@pytest.mark.parametrize("n", [1, 8, 9, 64])       # 9: the smallest N with a ragged second workgroup
def test_fused_equals_step(cuda, obs, A, n):
    from apex_amd.engine.vector_host_eval import VectorHostEvaluator

    eng = _engine(cuda, obs, A)
    first, steps = _script(obs, n)
    assert any((s["ended"] > s["done"]).any() for s in steps) and any(s["done"].any() for s in steps)
    assert any((s["next_obs"] != s["reset_obs"]).any() for s in steps)
    tapes, vecs = {}, {}
    for kernel in ("fused", "step"):
        vecs[kernel] = vec = Tape(first, steps, A)
        ev = VectorHostEvaluator(eng, vec, kernel=kernel, seed=11)
        tapes[kernel] = _play(ev, guards=_guarded(ev))
        assert ev.ledger.steps == STEPS and ev.k == STEPS
        if kernel == "step":
            assert int(ev.counter) == STEPS - 1
        ev.close()
        ev.close()
    seed = ev.act_seed
    for t, (a, b) in enumerate(zip(tapes["fused"], tapes["step"])):
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (t, k)
        assert torch.isfinite(a["q"]).all()
        want = select_actions_ref(a["q"].numpy(), np.zeros(n, np.float32), seed, t)
        assert np.array_equal(a["actions"].numpy(), want), t
        assert np.array_equal(want, a["q"].numpy().argmax(1))    # (no key of this run draws u0 == 0)
    assert not torch.equal(tapes["fused"][0]["q"], tapes["fused"][1]["q"])       # the observations matter
    assert all(np.array_equal(x, y) for x, y in zip(vecs["fused"].received, vecs["step"].received))
    # the ledger saw the tape's ends: capped = ended without done
    n_end = int(sum(s["ended"].sum() for s in steps))
    n_cap = int(sum((s["ended"] > s["done"]).sum() for s in steps))
    assert (ev.ledger.episodes, ev.ledger.capped) == (n_end, n_cap)
    assert sum(e[2] for e in ev.poll()) == n_cap


# ------------------------------------------------------------------ 2. Q against fp64
@pytest.mark.parametrize("obs,A", SHAPES[:4])
def test_q_is_the_fp64_q_of_the_staged_reset_obs(cuda, obs, A):
    """(4, 2) and (2, 3): within the project's bound for this forward.  (6, 3) and (8, 7) have no
    recorded figure: the error of ``vec_act`` (the step form) on the same inputs is printed, and
    bit-equality with that form carries the bound."""
    from apex_amd.engine.vector_host_eval import VectorHostEvaluator

    eng = _engine(cuda, obs, A)
    n = 9
    first, steps = _script(obs, n, seed=5)
    ref = vp.fp64(eng.learner.model)
    errs = {}
    got = {}
    for kernel in ("fused", "step"):
        ev = VectorHostEvaluator(eng, Tape(first, steps, A), kernel=kernel, seed=5)
        got[kernel] = _play(ev, 3)
        ev.close()
        worst = 0.0
        for t, x in enumerate(got[kernel]):
            staged = first if t == 0 else steps[t - 1]["reset_obs"]
            with torch.no_grad():
                q64 = ref(torch.from_numpy(staged.astype(np.float64))).numpy()
            worst = max(worst, float(np.abs(x["q"].numpy().astype(np.float64) - q64).max() / np.abs(q64).max()))
        errs[kernel] = worst
    print(f"obs {obs} A {A}: rel err vs fp64 fused {errs['fused']:.3e} step (vec_act) {errs['step']:.3e}")
    assert all(_same(a, b) for a, b in zip(got["fused"], got["step"]))
    if (obs, A) in ((4, 2), (2, 3)):
        assert errs["fused"] <= Q_BOUND, errs
    # the wrong staging rows would be far off: next_obs differs from reset_obs where an episode ended
    with torch.no_grad():
        q_next = ref(torch.from_numpy(steps[0]["next_obs"].astype(np.float64))).numpy()
    off = float(np.abs(got["fused"][1]["q"].numpy() - q_next).max() / np.abs(q_next).max())
    assert off > 1e-3, off


# ------------------------------------------------------------------ 3. against vec_rollout's trace
def test_tape_equals_vec_rollout_trace(cuda):
    from apex_amd.engine.vector_host_eval import VectorHostEvaluator

    eng = _engine(cuda, 4, 2)
    n, Tr, seed = 3, 24, 7
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=cuda)  # noqa: E731
    buf = dict(returns=f(n), lengths=torch.full((n,), -1, dtype=torch.int32, device=cuda),
               ended=torch.full((n,), -1, dtype=torch.int32, device=cuda), trace_obs=f(n, Tr, 4), trace_q=f(n, Tr, 2),
               trace_act=torch.full((n, Tr), -1, dtype=torch.int32, device=cuda))
    d = dict(kind=0, N=n, obs=4, max_steps=200, seed=seed, trace_T=Tr)
    d.update({k: v.data_ptr() for k, v in buf.items()})
    eng.hip.vec_rollout(eng.hip.make_vec_rollout(eng.learner.net, d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tr = {k: v.cpu().numpy() for k, v in buf.items()}
    lengths = tr["lengths"]
    print("vec_rollout lengths", lengths.tolist())
    L = np.minimum(lengths, Tr)
    steps = []
    for t in range(Tr):
        nxt = np.zeros((n, 4), np.float32)
        for b in range(n):
            if t + 1 < L[b]:
                nxt[b] = tr["trace_obs"][b, t + 1]
        steps.append(dict(next_obs=nxt, reset_obs=nxt, reward=np.ones(n, np.float32), done=np.zeros(n, np.float32),
                          ended=np.zeros(n, np.float32)))
    ev = VectorHostEvaluator(eng, Tape(tr["trace_obs"][:, 0], steps, 2), kernel="fused", seed=seed)
    compared = np.zeros(n, np.int64)
    for t, x in enumerate(_play(ev, Tr)):
        for b in range(n):
            if t >= L[b]:
                continue
            compared[b] += 1
            assert np.array_equal(_bits(x["q"][b]), _bits(tr["trace_q"][b, t])), (t, b)
            assert int(x["actions"][b]) == int(tr["trace_act"][b, t]), (t, b)
    ev.close()
    assert (compared >= 8).all(), compared       # CartPole's shortest episode under a constant push


# ------------------------------------------------------------------ 4. weight sets
def test_refresh_switches_the_weight_set_between_two_acts(cuda):
    from apex_amd.engine.vector_host_eval import VectorHostEvaluator

    eng = _engine(cuda, 2, 3)
    flat = eng.learner.flat
    old = flat.clone()
    first, steps = _script(2, 3)
    mk = lambda: VectorHostEvaluator(eng, Tape(first, steps, 3), seed=2)  # noqa: E731
    try:
        ev, ev_old = mk(), mk()
        got = _play(ev, 2)
        set_params(eng.learner.model, seed=9)          # the online parameters move on
        torch.cuda.synchronize()
        new = flat.clone()
        assert not torch.equal(old, new)
        assert ev.refresh() is True
        got += _play(ev, 1)
        want_old = _play(ev_old, 3)                    # never refreshed: the old parameters throughout
        fresh = mk()
        want_new = _play(fresh, 3)                     # a fresh evaluator on the new parameters
        assert _same(got[0], want_old[0]) and _same(got[1], want_old[1])      # the acts before the refresh
        assert _same(got[2], want_new[2])                                      # the act after it
        assert not _same(got[2], want_old[2], ("q",))
        cur = ev.weights.cur
        assert cur == 1 and ev.weights.refreshes == 1
        assert torch.equal(ev.flats[cur], new) and torch.equal(ev.flats[1 - cur], old)
        assert torch.equal(ev_old.flats[0], old) and torch.equal(ev_old.flats[1], old)
        assert ev_old.weights.cur == 0 and ev_old.weights.refreshes == 0
        for e in (ev, ev_old, fresh):
            e.close()
    finally:
        flat.copy_(old)
        torch.cuda.synchronize()


# ------------------------------------------------------------------ 5. pool == in-process
def test_pool_evaluation_equals_the_in_process_run(cuda):
    from apex_amd.engine.host_eval import eval_seed
    from apex_amd.engine.vector_host_eval import VectorHostEvaluation, VectorHostEvaluator, make_pool
    from apex_amd.envs.host_vector import HostVectorEnv

    eng = _engine(cuda, 4, 2)
    seed, n, cap, want_n = 4, 3, 12, 6
    vec = HostVectorEnv("CartPole-v0", n, seed=eval_seed(seed), max_episode_length=cap)
    ref = VectorHostEvaluator(eng, vec, seed=seed)
    ref.run(2 * cap)                                   # every env ends at least two episodes
    want = [e[:3] for e in ref.poll()][:want_n]
    ref.close()
    vec.close()
    assert len(want) == want_n and all(1 <= e[1] <= cap and e[0] == e[1] and e[2] <= (e[1] == cap) for e in want)
    pool = make_pool("CartPole-v0", n, 2, seed=seed, max_episode_length=cap, timeout=30.0)
    drv = VectorHostEvaluation(VectorHostEvaluator(eng, pool, seed=seed), pool)
    got, deadline = [], time.monotonic() + 60.0
    try:
        while len(got) < want_n:
            assert time.monotonic() < deadline, (len(got), drv.pumps)
            drv.pump(learn_step=7)
            got += drv.poll()
    finally:
        drv.close()
        drv.close()
    print("pumps", drv.pumps, "evaluator steps", drv.ev.ledger.steps, "episodes", want)
    assert [e[:3] for e in got[:want_n]] == want and all(e[3] == 7 for e in got)
    assert all(not p.is_alive() for p in pool.processes)


# ------------------------------------------------------------------ 6. training untouched
def _state(eng):
    torch.cuda.synchronize()
    r, L, sh = eng.replay, eng.learner, eng.shard
    t = dict(s_ids=r.s_ids, s2_ids=r.s2_ids, action=r.action, reward=r.reward, done=r.done, ring=r.frames,
             leaf_sum=r.leaf_sum, leaf_min=r.leaf_min, max_prio=r.max_prio, filled=r.filled, flat=L.flat,
             tflat=L.tflat, actor_flat=eng.actor_flat, opt_s1=L.opt_s1, opt_s2=L.opt_s2, idx=L.idx, beta=L.beta,
             loss=L.loss, ep_log=sh.ep_log, hist=sh.st["hist"], new_frame=sh.new_frame, shard_step=sh.step_counter,
             learner_step=L.step_counter)
    t.update({f"node_sum{i}": x for i, x in enumerate(r.node_sum)})
    t.update({f"node_min{i}": x for i, x in enumerate(r.node_min)})
    return {k: v.detach().cpu().clone() for k, v in t.items()}


def test_evaluator_leaves_training_bit_identical(cuda):
    from apex_amd.engine.vector_host import VectorHostEngine
    from apex_amd.engine.vector_host_eval import VectorHostEvaluation, VectorHostEvaluator, make_pool
    from apex_amd.envs.host_vector import HostVectorEnv

    def run(with_eval):
        vec = HostVectorEnv("CartPole-v0", 4, seed=3)
        eng = VectorHostEngine(_cfg("CartPole-v0", 4), vec, cuda, learner_steps=2)
        eng.fill()
        eng.capture()
        assert eng._g_learn is not None
        drv = None
        if with_eval:
            pool = make_pool("CartPole-v0", 2, 1, seed=3, max_episode_length=20, timeout=30.0)
            drv = VectorHostEvaluation(VectorHostEvaluator(eng, pool, seed=3), pool)
        try:
            for it in range(8):
                eng.train_step()
                if drv is not None:
                    if it % 2 == 1:
                        drv.refresh()
                    drv.pump(eng.learn_steps)
            torch.cuda.synchronize()
            if drv is not None:
                print("evaluator steps", drv.ev.ledger.steps, "refreshes", drv.ev.weights.refreshes)
                assert drv.ev.weights.refreshes >= 1 and drv.ev.k >= 1
        finally:
            if drv is not None:
                drv.close()
        out = _state(eng)
        steps = eng.learn_steps
        eng.close()
        return out, steps

    (a, sa), (b, sb) = run(False), run(True)
    assert sa == sb == 2 * (3 + 8) and int(a["learner_step"]) == sa     # capture's 3 warm-up iterations + 8
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


# ------------------------------------------------------------------ 7. launcher limits
def test_launcher_limits(cuda):
    from apex_amd.engine.vector_host_eval import VectorHostEvaluator

    eng = _engine(cuda, 4, 2)
    h, s = eng.hip, torch.cuda.current_stream().cuda_stream
    n = 3
    first, steps = _script(4, n)
    ev = VectorHostEvaluator(eng, Tape(first, steps, 2), seed=1)
    ev.q.fill_(Q_SENT)
    ev.actions.fill_(A_SENT)
    ev.vec.reset()
    ev.ship()
    ptrs = {k: p.data_ptr() for k, p in ev.models[0].named_parameters()}
    net = lambda **o: h.make_vec_net(dict(dict(ptrs, obs=4, A=2), **o))  # noqa: E731
    good_net = ev.nets[0]
    good = dict(N=n, seed=ev.act_seed, stage=ev.stage_dev.data_ptr(), q=ev.q.data_ptr(), actions=ev.actions.data_ptr())
    drop = lambda *ks: {k: v for k, v in good.items() if k not in ks}  # noqa: E731
    G = None   # (the evaluator's own handle)
    bad = [(G, dict(good, N=0)), (G, dict(good, N=65)), (G, dict(good, N=-1)),
           (dict(obs=0), good), (dict(obs=9), good), (dict(A=0), good), (dict(A=8), good),
           (G, drop("stage")), (G, drop("q")), (G, drop("actions")),
           ({"features.0.weight": 0}, good), ({"value.2.bias": 0}, good)]
    for kw, d in bad:
        with pytest.raises(ValueError):
            h.vec_host_eval_act(h.make_vec_host_eval_act(good_net if kw is None else net(**kw), d), 0, s)
    with pytest.raises(ValueError):
        h.vec_host_eval_act(h.make_vec_host_eval_act(good_net, good), -1, s)
    torch.cuda.synchronize()
    assert (ev.q == Q_SENT).all() and (ev.actions == A_SENT).all()           # none of them reached the GPU
    h.vec_host_eval_act(h.make_vec_host_eval_act(good_net, good), 0, s)      # the good descriptor runs
    torch.cuda.synchronize()
    assert torch.isfinite(ev.q).all() and (ev.q != Q_SENT).all()
    assert ((0 <= ev.actions) & (ev.actions < 2)).all()
    ev.close()
    with pytest.raises(ValueError, match="64"):
        VectorHostEvaluator(eng, Tape(np.zeros((65, 4), np.float32), [], 2))
    with pytest.raises(ValueError, match="kernel"):
        VectorHostEvaluator(eng, Tape(first, steps, 2), kernel="graph")
    with pytest.raises(ValueError, match="differ"):
        VectorHostEvaluator(eng, Tape(np.zeros((2, 2), np.float32), [], 3))
    with pytest.raises(ValueError, match="differ"):
        VectorHostEvaluator(eng, Tape(np.zeros((2, 4), np.float32), [], 3))
    box = Tape(np.zeros((2, 4), np.float32), [], 2)
    box.continuous = True
    with pytest.raises(ValueError, match="discrete"):
        VectorHostEvaluator(eng, box)


# ------------------------------------------------------------------ 8. command line
def test_cli_writes_evaluator_records_and_leaves_no_process(cuda, tmp_path, monkeypatch):
    from apex_amd import train_vector
    from apex_amd.engine import vector_host_eval as vhe
    from apex_amd.engine.vector_host import VectorHostEngine

    cap, polled = 30, []
    real_poll = vhe.VectorHostEvaluation.poll

    def poll(self):
        out = real_poll(self)
        polled.extend(out)
        return out

    monkeypatch.setattr(vhe.VectorHostEvaluation, "poll", poll)
    monkeypatch.setattr(VectorHostEngine, "evaluate", lambda *a, **k: pytest.fail("evaluate was called"))
    log = tmp_path / "log.jsonl"
    a = train_vector.parser().parse_args(
        ["--host-envs", "--env", "CartPole-v0", "--envs", "4", "--eval-envs", "2", "--eval-workers", "1",
         "--eval-interval", "2", "--max-episode-length", str(cap), "--max-step", "400", "--capacity", "4096",
         "--save-interval", "1000", "--save-dir", str(tmp_path), "--log-interval", "50", "--json-log", str(log)])
    assert a.eval_kernel == "fused"
    last = train_vector.train(a)
    recs = [json.loads(x) for x in log.read_text().splitlines()]
    print([(r["step"], r["evaluator_episodes"], r["evaluator_mean_return"], r["evaluator_steps"]) for r in recs])
    assert [r["step"] for r in recs] == list(range(50, 401, 50)) and last == recs[-1]
    assert all({"evaluator_episodes", "evaluator_mean_return", "evaluator_steps"} <= set(r) for r in recs)
    assert all("greedy_mean_return" not in r for r in recs)
    assert sum(r["evaluator_episodes"] for r in recs) == len(polled) >= 1
    assert all(1 <= e[1] <= cap and e[0] == e[1] and 0 <= e[3] <= 400 for e in polled)   # CartPole: +1 a step
    for r in recs:
        if r["evaluator_episodes"] == 0:
            assert r["evaluator_mean_return"] is None
        else:
            assert 1.0 <= r["evaluator_mean_return"] <= cap
    steps = [r["evaluator_steps"] for r in recs]
    assert steps == sorted(steps) and steps[-1] >= 1
    assert mp.active_children() == []                               # the evaluator's workers are gone
