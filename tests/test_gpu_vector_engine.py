"""GPU vector-observation Ape-X engine (engine/vector.py, ops/csrc/vector_kernels.hip): the
classic-control env kernels against envs/classic.py, the acting forward and its epsilon-greedy
draw, the n-step batcher over the observation ring against BatchStorage, the learner step
against fp64 PyTorch, and the engine's determinism / graph / bookkeeping invariants.

fp64 comparisons: the error figure of a tensor is max|x - ref| / max|ref| (gradients: the
relative L2 norm).  Bounds are 2x the maxima measured on an MI355X (profiles/vector_engine.md),
rounded up to one significant digit."""
import numpy as np
import pytest
import torch

from apex_amd import envs
from apex_amd.algo.losses import compute_loss_device
from apex_amd.algo.schedules import beta_by_frame, step_scheduler_early
from apex_amd.models.dqn import DuelingDQN

from . import actor_oracle as ao

pytestmark = pytest.mark.gpu

# measured maxima (profiles/vector_engine.md) x 2, rounded up to one significant digit
Q_BOUND = 3e-6     # measured 1.32e-6 (acting, CartPole E = 64); learner Q rows 4.7e-7
LOSS_BOUND = 8e-7  # measured 3.6e-7
PRIO_BOUND = 2e-6  # measured 7.9e-7
GRAD_BOUND = 2e-6  # measured 6.8e-7 (relative L2 norm, worst tensor)


def _np(t):
    return t.detach().cpu().numpy()


def _rel(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-30))


def _shard(cuda, env_id, E, n=3, C=4096, mode="reference", **kw):
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.vector import VECTOR_ENVS, VectorActorShard

    obs = VECTOR_ENVS[env_id][1]
    rp = HBMReplay(C, n_envs=E, n_step=n, device=cuda, frame_bytes=4 * obs)
    return rp, VectorActorShard(rp, E, env_id, n_step=n, mode=mode, **kw)


def _biased_model(env_id, cuda, seed):
    """The env's MLP dueling net with non-zero biases (the init's are zero)."""
    from apex_amd.engine.vector import make_model

    torch.manual_seed(seed)
    m = make_model(env_id)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.2)
    return m.to(cuda)


def _host_step(env, s, a):
    """envs/classic.py from fp32 state ``s`` (exact in fp64): (s' fp64, terminal)."""
    u = env.unwrapped
    u.state = tuple(float(v) for v in s)
    u.steps_beyond_done = None
    u.step(int(a))
    nxt = np.asarray(u.state, dtype=np.float64)
    if hasattr(u, "x_threshold"):
        term = bool(nxt[0] < -u.x_threshold or nxt[0] > u.x_threshold or nxt[2] < -u.theta_threshold_radians
                    or nxt[2] > u.theta_threshold_radians)
        margin = min(abs(abs(nxt[0]) - u.x_threshold), abs(abs(nxt[2]) - u.theta_threshold_radians))
    else:
        term = bool(nxt[0] >= u.goal_position)
        margin = abs(nxt[0] - u.goal_position)
    return nxt, term, margin


# ------------------------------------------------------------------ env kernels
@pytest.mark.parametrize("env_id", ["CartPole-v0", "MountainCar-v0"])
def test_env_single_steps_match_host_dynamics(cuda, env_id):
    """Every recorded (s, a, s') of 300 random-action steps of 64 envs, re-stepped through
    envs/classic.py from s: s' within rtol 1e-4 / atol 1e-5 (the bound of
    test_cartpole_env_matches_host_dynamics for the same arithmetic), the terminal flag equal
    wherever s' is further than 1e-4 from a threshold, reward, TimeLimit and ring bookkeeping."""
    E, T = 64, 300
    rp, sh = _shard(cuda, env_id, E, C=32768, seed=5)
    obs, A, limit = sh.obs_dim, sh.A, sh.max_episode_steps
    L = sh.layout
    env = envs.make(env_id)
    g = torch.Generator(device="cpu").manual_seed(1)
    bad, n_term, n_time = [], 0, 0
    for t in range(T):
        st0 = _np(sh.env_state)
        a = torch.randint(0, A, (E,), generator=g, dtype=torch.int32)
        sh.actions.copy_(a)
        sh.act_and_step(selected=True)
        torch.cuda.synchronize()
        st1, d, r, nf = _np(sh.env_state), _np(sh.done), _np(sh.reward), _np(sh.new_frame)
        ring = _np(sh.ring)
        assert np.array_equal(nf, ((t + 1) * E + np.arange(E)) % rp.frame_capacity)
        assert np.all(r == (1.0 if obs == 4 else -1.0))
        for e in range(E):
            want, term, margin = _host_step(env, st0[e, :obs], a[e])
            got = st1[e, L["LAST"]:L["LAST"] + obs]
            if not np.allclose(got, want, rtol=1e-4, atol=1e-5):
                bad.append(("s'", t, e, got, want))
            time_up = st0[e, L["EPLEN"]] + 1 >= limit
            if margin > 1e-4 and bool(d[e] > 0.5) != (term or time_up):
                bad.append(("done", t, e, d[e], term, time_up))
            n_term += term
            n_time += bool(time_up and not term)
            if d[e] > 0.5:  # the ring row and the state hold the reset observation
                if not (np.array_equal(ring[nf[e]], st1[e, :obs]) and st1[e, L["EPLEN"]] == 0):
                    bad.append(("reset", t, e))
            elif not (np.array_equal(ring[nf[e]], got) and np.array_equal(st1[e, :obs], got)
                      and st1[e, L["EPLEN"]] == st0[e, L["EPLEN"]] + 1):
                bad.append(("carry", t, e))
    print(f"{env_id}: {T * E} steps, {n_term} terminals, {n_time} time limits, {len(bad)} mismatches")
    assert not bad, bad[:5]
    assert (n_term if obs == 4 else n_time) >= E  # the episode ends this env produces did occur
    _, lens, count = sh.episode_stats()
    assert (count > 0).all() and (lens >= 1).all() and (lens <= limit).all()
    assert int(rp.filled.item()) == T * E


def _crafted(env_id):
    """(state rows, actions): every value >= 0.005 from its threshold, far above fp32 error."""
    rows, acts = [], []
    if env_id.startswith("CartPole"):
        for x in (0.0, 2.39, -2.39, 2.41, -2.41):
            for th in (0.0, 0.2, -0.2, 0.215, -0.215):
                for a in (0, 1):
                    rows.append((x, 0.0, th, 0.0))
                    acts.append(a)
    else:
        for s in ((-1.2, -0.01), (0.495, 0.07), (0.40, 0.0)):
            for a in (0, 1, 2):
                rows.append((s[0], s[1], 0.0, 0.0))
                acts.append(a)
    return np.asarray(rows, dtype=np.float32), np.asarray(acts, dtype=np.int32)


@pytest.mark.parametrize("env_id", ["CartPole-v0", "CartPole-v1", "MountainCar-v0"])
def test_env_crafted_states_and_time_limit(cuda, env_id):
    rows, acts = _crafted(env_id)
    E = len(rows) + 1  # + one env forced to the step before its TimeLimit
    rp, sh = _shard(cuda, env_id, E, seed=9)
    obs, limit, L = sh.obs_dim, sh.max_episode_steps, sh.layout
    torch.cuda.synchronize()
    # reset draws: inside their ranges, MountainCar's velocity exactly 0, ring row = state
    st = _np(sh.env_state)
    ring = _np(sh.ring)
    assert np.array_equal(_np(sh.new_frame), np.arange(E))
    assert np.array_equal(ring[:E], st[:, :obs])
    if obs == 4:
        assert (np.abs(st[:, :4]) <= 0.05).all() and np.unique(st[:, :4]).size > 2 * E
    else:
        assert (st[:, 0] >= -0.6).all() and (st[:, 0] <= -0.4).all() and (st[:, 1] == 0).all()
        assert np.unique(st[:, 0]).size > E // 2
    state = torch.zeros(E, L["STRIDE"])
    state[:E - 1, :4] = torch.from_numpy(rows)
    state[E - 1, :4] = torch.from_numpy(st[E - 1, :4])
    state[E - 1, L["EPLEN"]] = limit - 1
    state[E - 1, L["EPRET"]] = 7.0
    sh.env_state.copy_(state)
    sh.actions.copy_(torch.from_numpy(np.append(acts, 1).astype(np.int32)))
    sh.env_step()
    torch.cuda.synchronize()
    st1, d = _np(sh.env_state), _np(sh.done)
    env = envs.make(env_id)
    n_done = 0
    for e in range(E - 1):  # no case skipped: the done flag must equal the host's exactly
        want, term, margin = _host_step(env, rows[e, :obs], acts[e])
        assert margin >= 0.005, (e, rows[e], margin)  # far above fp32 error
        assert bool(d[e] > 0.5) == term, (e, rows[e], acts[e], want)
        np.testing.assert_allclose(st1[e, L["LAST"]:L["LAST"] + obs], want, rtol=1e-4, atol=1e-5)
        n_done += term
    if obs == 4:
        assert n_done == 2 * (25 - 9)  # every case with |x| = 2.41 or |theta| = 0.215
    else:
        assert n_done == 3  # the goal case, every action
        assert (st1[0:3, L["LAST"]] == np.float32(-1.2)).all() and (st1[0:3, L["LAST"] + 1] == 0).all()  # the wall
    # TimeLimit: done = 1, the logged length is the limit, the env is reset
    assert d[E - 1] == 1.0
    log = _np(sh.ep_log)[E - 1]
    assert log[1] == limit and log[2] == 1 and log[0] == 7.0 + (1.0 if obs == 4 else -1.0)
    assert st1[E - 1, L["EPLEN"]] == 0 and st1[E - 1, L["EPRET"]] == 0
    # every env that ended holds a fresh reset draw, in range
    for e in np.flatnonzero(d > 0.5):
        s = st1[e, :obs]
        if obs == 4:
            assert (np.abs(s) <= 0.05).all()
        else:
            assert -0.6 <= s[0] <= -0.4 and s[1] == 0
        assert np.array_equal(_np(sh.ring)[_np(sh.new_frame)[e]], s)


# ------------------------------------------------------------------ acting forward + draw
@pytest.mark.parametrize("E", [1, 64, 300])
@pytest.mark.parametrize("env_id", ["CartPole-v0", "MountainCar-v0"])
def test_act_q_and_draw(cuda, env_id, E):
    rp, sh = _shard(cuda, env_id, E, C=max(1024, 4 * E), seed=2)
    model = _biased_model(env_id, cuda, seed=E)
    sh.set_policy(model)
    for _ in range(3):  # a few steps: the counter is non-zero and the observations have moved
        sh.act_and_step()
    sh.act()
    torch.cuda.synchronize()
    obs = sh.observe()
    assert obs.shape == (E, sh.obs_dim)
    ref = DuelingDQN.from_shapes((sh.obs_dim,), sh.A).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        q64 = ref(obs.double().cpu()).numpy()
    q = _np(sh.q)
    err = _rel(q, q64)
    print(f"act {env_id} E={E}: Q rel err {err:.3e}")
    assert err <= Q_BOUND
    want = ao.select_actions_ref(q, _np(sh.eps), sh.seed ^ 0x5E1EC7, int(sh.step_counter.item()))
    assert np.array_equal(_np(sh.actions), want)
    if E >= 64:  # both branches of the draw occur
        greedy = q.argmax(1)
        assert (want != greedy).any() and (want == greedy).sum() > E // 2


# ------------------------------------------------------------------ n-step over the vector ring
@pytest.mark.parametrize("mode", ["reference", "textbook"])
@pytest.mark.parametrize("n", [1, 3])
def test_nstep_through_vector_ring_matches_batchstorage(cuda, mode, n):
    """250 steps of 32 CartPole envs under a high epsilon (many short episodes), recorded from
    the device buffers and replayed through BatchStorage: rows match in emission order."""
    from apex_amd.replay.nstep import BatchStorage

    E, T, gamma = 32, 250, 0.99
    rp, sh = _shard(cuda, "CartPole-v0", E, n=n, C=16384, mode=mode, gamma=gamma, eps_base=0.8, eps_alpha=1.0,
                    seed=11)
    sh.set_policy(_biased_model("CartPole-v0", cuda, seed=4))
    oracles = [BatchStorage(n, gamma, mode=mode) for _ in range(E)]
    emitted = [[] for _ in range(E)]
    for t in range(T):
        obs = _np(sh.observe())
        sh.act_and_step()
        torch.cuda.synchronize()
        a, r, d, q = _np(sh.actions), _np(sh.reward), _np(sh.done), _np(sh.q)
        slot, prio = _np(sh.slot), _np(sh.prio)
        for e in range(E):
            oracles[e].add(obs[e].tobytes(), float(r[e]), int(a[e]), bool(d[e] > 0.5), q[e].copy())
            if prio[e] > 0:
                emitted[e].append((slot[e], prio[e]))
    ring = _np(sh.ring)
    s_ids, s2_ids = _np(rp.s_ids), _np(rp.s2_ids)
    acts, rews, dones = _np(rp.action), _np(rp.reward), _np(rp.done)
    pending = _np(sh.st["drain_meta"])[:, 1]
    total = 0
    for e in range(E):
        o = oracles[e]
        prios = o.compute_priorities()
        assert len(emitted[e]) + int(pending[e]) == len(o), (e, len(emitted[e]), pending[e], len(o))
        for k, (sl, pr) in enumerate(emitted[e]):
            assert ring[s_ids[sl, 3]].tobytes() == o.states[k], (e, k)
            assert ring[s2_ids[sl, 3]].tobytes() == o.next_states[k], (e, k)
            assert acts[sl] == o.actions[k] and dones[sl] == o.dones[k], (e, k)
            np.testing.assert_allclose(rews[sl], o.rewards[k], rtol=1e-5)
            np.testing.assert_allclose(pr, prios[k], rtol=1e-5)
        total += len(emitted[e])
        assert sum(o.dones) >= 3  # several episodes per env ended
    assert total > T * E * 0.6
    assert int(rp.filled.item()) == T * E


# ------------------------------------------------------------------ learner step vs fp64
def _learner_engine(cuda, env_id, B, **kw):
    from apex_amd.engine.vector import VectorApexEngine, VectorEngineConfig

    cfg = VectorEngineConfig(env_id=env_id, n_envs=64, batch_size=B, replay_capacity=8192, **kw)
    eng = VectorApexEngine(cfg, cuda)
    torch.manual_seed(100 + B)
    with torch.no_grad():  # non-zero biases, and a target that differs from the online net
        for name, p in eng.learner.model.named_parameters():
            if name.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.2)
        eng.learner.tflat.add_(torch.randn_like(eng.learner.tflat) * 0.05)
    eng.publish_params()
    for _ in range(40):
        eng.actor_step()
    return eng


def _double(model):
    m = DuelingDQN.from_shapes(model.input_shape, model.num_actions).double()
    m.load_state_dict({k: v.detach().double().cpu() for k, v in model.state_dict().items()})
    return m


@pytest.mark.parametrize("B", [16, 48, 64])
@pytest.mark.parametrize("env_id", ["CartPole-v0", "MountainCar-v0"])
def test_learner_step_matches_fp64(cuda, env_id, B):
    """Three SGD steps.  Each: Q(s), Q(s'), Q_target(s'), loss, priorities and every tensor's
    gradient against fp64 PyTorch (compute_loss_device + autograd) on the engine's own idx / w;
    the kernel's own flat gradient fed to torch's centered RMSprop with an early StepLR step
    reproduces the parameters at rtol 1e-5 / atol 1e-6 (test_rmsprop_clip_matches_torch's
    bound, same optimizer kernel)."""
    eng = _learner_engine(cuda, env_id, B, lr=1e-4, lr_step_size=2, lr_gamma=0.5)
    L, rp, cfg = eng.learner, eng.replay, eng.cfg
    ref_p = [p.detach().clone().requires_grad_(True) for p in L.model.parameters()]
    opt = torch.optim.RMSprop(ref_p, lr=cfg.lr, alpha=cfg.rms_alpha, eps=cfg.rms_eps, centered=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=cfg.lr_step_size, gamma=cfg.lr_gamma)
    worst = {"q": 0.0, "loss": 0.0, "prio": 0.0, "grad": 0.0}
    knee = [0, 0]
    # Q(s, a) is moved to about 0.4, 2.0 and 1.0 from the n-step target (|R| ~ 3.94, Q_target ~ 0), step
    # by step, so the TD errors fall on both sides of the Huber knee (the same fp32 add on both sides;
    # an SGD step at this lr moves Q by far less than the gaps)
    sign = 1.0 if env_id.startswith("CartPole") else -1.0
    for it in range(3):
        with torch.no_grad():
            shift = sign * (3.54, -1.6, 1.0)[it]
            L.model.value[2].bias.add_(shift)
            ref_p[-1].add_(shift)
        assert float(L.beta.item()) == pytest.approx(beta_by_frame(it, cfg.beta, cfg.beta_horizon), rel=1e-6)
        L.sample()
        L.forward_backward()
        torch.cuda.synchronize()
        idx = L.idx.long()
        assert int(idx.min()) >= 0 and int(idx.max()) < len(rp)
        ring = L.ring
        s = ring[rp.s_ids[idx, 3].long()].double().cpu()
        s2 = ring[rp.s2_ids[idx, 3].long()].double().cpu()
        batch = (s, rp.action[idx].long().cpu(), rp.reward[idx].double().cpu(), s2, rp.done[idx].double().cpu(),
                 L.w.double().cpu())
        on, tg = _double(L.model), _double(L.target)
        loss64, prio64 = compute_loss_device(on, tg, batch, cfg.n_step, cfg.gamma)
        loss64.backward()
        with torch.no_grad():
            worst["q"] = max(worst["q"], _rel(_np(L.q_s), on(s).numpy()), _rel(_np(L.q_s2), on(s2).numpy()),
                             _rel(_np(L.qt_s2), tg(s2).numpy()))
        grad = L.flat_grad.clone()
        knee[0] += int((L.delta < 1).sum())
        knee[1] += int((L.delta >= 1).sum())
        for (name, o, k), p64 in zip(L.segments, on.parameters()):
            g64 = p64.grad.reshape(-1).numpy()
            gk = _np(grad[o:o + k]).astype(np.float64)
            worst["grad"] = max(worst["grad"], float(np.linalg.norm(gk - g64) / max(np.linalg.norm(g64), 1e-30)))
            assert np.linalg.norm(g64) > 0, name
        # the reference optimizer on the kernel's own gradient
        off = 0
        for p in ref_p:
            p.grad = grad[off:off + p.numel()].view_as(p).clone()
            off += p.numel()
        l2 = torch.nn.utils.clip_grad_norm_(ref_p, cfg.max_norm)
        step_scheduler_early(sched)
        opt.step()
        L.optimize()
        L.write_priorities()
        torch.cuda.synchronize()
        l64 = float(loss64.detach())
        worst["loss"] = max(worst["loss"], abs(float(L.loss.item()) - l64) / abs(l64))
        worst["prio"] = max(worst["prio"], _rel(_np(L.prio), prio64.numpy()))
        torch.testing.assert_close(L.norms[0], l2, rtol=1e-5, atol=1e-5)
        assert float(L.norms[3].item()) == pytest.approx(opt.param_groups[0]["lr"], rel=1e-6)
        assert int(L.step_counter.item()) == it + 1
    print(f"learner {env_id} B={B}: |td| < 1 / >= 1: {knee}; " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert knee[0] > 0 and knee[1] > 0  # both branches of the Huber loss were taken
    assert opt.param_groups[0]["lr"] == pytest.approx(cfg.lr * 0.5)  # the StepLR boundary was crossed, early
    torch.testing.assert_close(L.flat, torch.cat([p.detach().reshape(-1) for p in ref_p]), rtol=1e-5, atol=1e-6)
    assert worst["q"] <= Q_BOUND and worst["loss"] <= LOSS_BOUND and worst["prio"] <= PRIO_BOUND
    assert worst["grad"] <= GRAD_BOUND
    st = L.stats()
    assert set(st) == {"loss", "grad_norm_l2", "grad_norm", "clip", "lr"} and all(v == v for v in st.values())


def test_grad_norm_partials_match_grad_sumsq(cuda):
    """The gradient launch's fp64 partials carry the norm grad_sumsq computes."""
    eng = _learner_engine(cuda, "CartPole-v0", 64)
    L = eng.learner
    L.sample()
    L.forward_backward()
    L.hip.grad_sumsq(L.flat_grad.data_ptr(), L.P, L.partials.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert float(L.part.sum()) == pytest.approx(float(L.partials.sum()), rel=1e-12)
    assert float(L.part.sum()) == pytest.approx(float(L.flat_grad.double().pow(2).sum()), rel=1e-12)


# ------------------------------------------------------------------ determinism, graphs, bookkeeping
@pytest.fixture(scope="module")
def runs(cuda):
    """Engine ``a`` eager, engine ``b`` through hipGraphs, same seed, 50 train steps each;
    snapshots of the parameters at 30 and of the acting copy right after the publish at 32."""
    from apex_amd.engine.vector import VectorApexEngine, VectorEngineConfig

    out = {}
    for name in ("a", "b"):
        cfg = VectorEngineConfig(env_id="CartPole-v0", n_envs=64, batch_size=64, replay_capacity=8192, lr=1e-3,
                                 seed=3)
        eng = VectorApexEngine(cfg, cuda)
        eng.fill()
        filled0, steps0 = int(eng.replay.filled.item()), eng.actor_steps
        if name == "b":
            eng.capture(warmup_iters=3)
        snap = {}
        while eng.learn_steps < 50:
            eng.train_step()
            if eng.learn_steps == 30:
                snap["p30"] = eng.learner.flat.clone()
            if eng.learn_steps == 32:
                snap["pub"] = (eng.actor_flat.clone(), eng.learner.flat.clone())
            if eng.learn_steps == 33:
                snap["after"] = (eng.actor_flat.clone(), eng.learner.flat.clone())
        torch.cuda.synchronize()
        out[name] = (eng, snap, filled0, steps0)
    return out


def test_same_seed_bit_identical_and_graph_equals_eager(runs):
    (a, sa, _, _), (b, sb, _, _) = runs["a"], runs["b"]
    assert b._g_learn is not None and a._g_learn is None
    assert torch.equal(sa["p30"], sb["p30"])
    assert torch.equal(a.learner.flat, b.learner.flat)
    assert torch.equal(a.replay.leaf_sum, b.replay.leaf_sum)
    assert torch.equal(a.shard.env_state, b.shard.env_state)
    assert not torch.equal(sa["p30"], a.learner.flat)  # (training went on after the snapshot)


def test_tree_fill_and_episode_invariants(runs):
    for name in ("a", "b"):
        eng, _, filled0, steps0 = runs[name]
        rp = eng.replay
        assert float(rp.node_sum[-1][0]) == pytest.approx(float(rp.leaf_sum.double().sum()), rel=1e-9)
        assert filled0 == steps0 * 64 and filled0 > eng.cfg.batch_size
        assert int(rp.filled.item()) == eng.actor_steps * 64 == filled0 + 50 * 64
        assert int(eng.learner.step_counter.item()) == 50
        _, lens, count = eng.shard.episode_stats()
        lens = lens[count > 0]
        assert lens.numel() > 0 and (lens >= 1).all() and (lens <= 200).all()
        assert float(eng.learner.beta.item()) == pytest.approx(beta_by_frame(50, 0.4, 1000.0), rel=1e-6)


def test_publish_cadence(runs):
    for name in ("a", "b"):
        _, snap, _, _ = runs[name]
        actor, learner = snap["pub"]
        assert torch.equal(actor, learner)  # right after the publish step
        actor, learner = snap["after"]
        assert torch.equal(actor, snap["pub"][0]) and not torch.equal(actor, learner)  # stale until the next


def test_save_and_evaluate(runs, tmp_path):
    eng = runs["b"][0]
    filled = int(eng.replay.filled.item())
    path = eng.save(str(tmp_path / "model50.pth"))
    m = DuelingDQN.from_shapes((4,), 2)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert list(sd) == list(m.state_dict())
    m.load_state_dict(sd)
    assert torch.equal(torch.cat([p.reshape(-1) for p in m.parameters()]), eng.learner.flat.cpu())
    ret = eng.evaluate(5)
    assert len(ret) == 5 and all(1 <= r <= 200 and r == int(r) for r in ret)
    assert int(eng.replay.filled.item()) == filled  # evaluation writes nothing to the replay
    assert eng.evaluate(5, seed=1) == eng.evaluate(5, seed=1)
