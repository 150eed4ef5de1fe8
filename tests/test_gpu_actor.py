"""GPU actor shard: n-step emission vs the host BatchStorage oracle, env invariants, and the
env / eps-greedy / n-step kernels against the host models of ``tests/actor_oracle.py``."""
from collections import Counter

import numpy as np
import pytest
import torch

from . import actor_oracle as ao

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["reference", "textbook"])
def test_nstep_kernel_matches_batchstorage(cuda, mode):
    from apex_amd.engine.actor_shard import ActorShard
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.replay.nstep import BatchStorage

    E, A, n, T, C = 16, 18, 3, 60, 4096
    rp = HBMReplay(C, n_envs=E, n_step=n, device=cuda)
    act = ActorShard(rp, E, A, n_step=n, gamma=0.9, seed=3, mode=mode, max_episode_steps=7)
    oracles = [BatchStorage(n, 0.9, mode=mode) for _ in range(E)]
    g = torch.Generator(device="cpu").manual_seed(0)
    emitted = [[] for _ in range(E)]
    for t in range(T):
        hist = act.st["hist"].cpu().numpy().copy()
        q = torch.randn(E, A, generator=g)
        act.act_and_step(q.to(cuda))
        torch.cuda.synchronize()
        a = act.actions.cpu().numpy()
        r = act.reward.cpu().numpy()
        d = act.done.cpu().numpy()
        slot = act.slot.cpu().numpy()
        prio = act.prio.cpu().numpy()
        for e in range(E):
            oracles[e].add(tuple(hist[e]), float(r[e]), int(a[e]), bool(d[e] > 0.5), q[e].numpy())
            if prio[e] > 0:
                emitted[e].append((t, slot[e], prio[e]))
    s_ids = rp.s_ids.cpu().numpy()
    s2_ids = rp.s2_ids.cpu().numpy()
    acts = rp.action.cpu().numpy()
    rews = rp.reward.cpu().numpy()
    dones = rp.done.cpu().numpy()
    for e in range(E):
        o = oracles[e]
        prios = o.compute_priorities()
        # every oracle emission appears exactly once (textbook flushes may be deferred by the drain)
        assert len(emitted[e]) == len(o), (e, len(emitted[e]), len(o))
        for k, (t, sl, pr) in enumerate(emitted[e]):
            assert tuple(s_ids[sl]) == tuple(o.states[k])
            if not o.dones[k]:
                assert tuple(s2_ids[sl]) == tuple(o.next_states[k])
            assert acts[sl] == o.actions[k]
            assert rews[sl] == pytest.approx(o.rewards[k], rel=1e-5, abs=1e-6)
            assert dones[sl] == o.dones[k]
            assert pr == pytest.approx(prios[k], rel=1e-4, abs=1e-5)


def test_env_frames_and_episodes(cuda):
    from apex_amd.engine.actor_shard import ActorShard
    from apex_amd.engine.hbm_replay import HBMReplay

    E = 32
    rp = HBMReplay(8192, n_envs=E, device=cuda)
    act = ActorShard(rp, E, 18, seed=1, max_episode_steps=50)
    for _ in range(120):
        act.act_and_step(torch.randn(E, 18, device=cuda))
    torch.cuda.synchronize()
    obs = act.observe()
    assert obs.dtype == torch.uint8 and obs.shape == (E, 4, 84, 84)
    assert obs.float().std() > 5  # something is rendered
    _, lens, count = act.episode_stats()
    assert (count > 0).all()  # 50-step time limit forces episode ends
    assert int(rp.filled.item()) == 120 * E
    # all emitted slots have positive mass
    assert rp.total_priority() > 0


def test_fused_eps_greedy_epilogue_matches_select_actions(cuda):
    """heads_fwd's eps-greedy epilogue == the standalone select_actions kernel on the same Q
    (first argmax, same Philox draw), and the staged n-step launch advances the counter."""
    from apex_amd import ops
    from apex_amd.engine.actor_shard import ActorShard
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.models.dqn import DuelingDQN
    from apex_amd.models.fused import HipDuelingNet, NetWorkspace

    E, A = 256, 18
    rp = HBMReplay(8192, n_envs=E, device=cuda)
    act = ActorShard(rp, E, A, seed=5, staged=2)
    net = HipDuelingNet(DuelingDQN.from_shapes((4, 84, 84), A).to(cuda))
    ws = NetWorkspace(E, A, cuda)
    ws.q = act.q
    h = ops.hip()
    s = torch.cuda.current_stream().cuda_stream
    for t in range(6):
        net(rp.frames, ws, act.st["hist"], act=act.act_args())
        fused = act.actions.clone()
        ref = torch.empty_like(fused)
        h.select_actions(act.q.data_ptr(), E, A, act.eps.data_ptr(), act.seed ^ 0x5E1EC7, act.step_counter.data_ptr(),
                         ref.data_ptr(), s)
        torch.cuda.synchronize()
        assert torch.equal(fused, ref), (t, (fused != ref).sum().item())
        c0 = int(act.step_counter.item())
        act.act_and_step(None, t % 2, selected=True)
        torch.cuda.synchronize()
        assert int(act.step_counter.item()) == c0 + 1
    # exploratory actions happen (eps ladder up to 0.4) and the greedy ones follow Q
    net(rp.frames, ws, act.st["hist"], act=act.act_args())
    torch.cuda.synchronize()
    agree = (act.actions == act.q.argmax(1).to(torch.int32)).float().mean().item()
    assert 0.5 < agree < 1.0, agree


# ---------------------------------------------------------------------------------------------
# The env, eps-greedy and n-step kernels against the host models of tests/actor_oracle.py.
# The tests call the bindings directly on an ActorShard's own tensors and supply every input.
TABLES = ("s_ids", "s2_ids", "action", "reward", "done")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _np(t):
    return t.detach().cpu().numpy()


def _shard(dev, E, A, n=3, C=None, F=None, mode="reference", gamma=0.99, seed=5, life=1, clip=1, repeat=4,
           max_steps=0, staged=0):
    from apex_amd.engine.actor_shard import ActorShard
    from apex_amd.engine.hbm_replay import HBMReplay

    rp = HBMReplay(C or 8 * E, n_envs=E, n_step=n, device=dev, frame_capacity=F)
    act = ActorShard(rp, E, A, n_step=n, gamma=gamma, seed=seed, mode=mode, clip_rewards=bool(clip),
                     episode_life=bool(life), max_episode_steps=max_steps, action_repeat=repeat, staged=staged)
    torch.cuda.synchronize()
    return rp, act


def _env_oracle(rp, act, cfg, seed):
    """The oracle for this shard, with the fma switch decided once by which rounding of
    4 + 72 u and 0.4 + 0.8 u the shard's construction-time reset (step 0) matches; every later
    reset and respawn is then held to that one rounding."""
    A, life, clip, repeat, max_steps = cfg
    dev = _np(act.env_state)
    match = []
    for fused in (True, False):
        env = ao.VecEnvOracle(act.E, A, rp.frame_capacity, repeat, clip, life, max_steps, fused=fused)
        want = np.stack([env.reset(e, seed, 1) for e in range(act.E)])
        match.append(np.array_equal(want[:, :ao.S_DEFINED], dev[:, :ao.S_DEFINED]))
    assert match[0] != match[1], ("the reset draws match neither or both roundings", match)
    return ao.VecEnvOracle(act.E, A, rp.frame_capacity, repeat, clip, life, max_steps, fused=match[0])


def _reset(rp, act, seed):
    act.hip.vec_env_reset(act.env_state.data_ptr(), seed, rp.frames.data_ptr(), act.env_params,
                          act.step_counter.data_ptr(), act.new_frame.data_ptr(), act.st["hist"].data_ptr(),
                          act.ep_log.data_ptr(), _stream())
    torch.cuda.synchronize()


def _check_reset(rp, act, env, seed):
    step = int(act.step_counter.item())
    st, nf, hist, log = _np(act.env_state), _np(act.new_frame), _np(act.st["hist"]), _np(act.ep_log)
    frames = _np(rp.frames[act.new_frame.long()]).reshape(act.E, 84, 84)
    for e in range(act.E):
        want = env.reset(e, seed, step * 16 + 1)
        assert np.array_equal(want[:ao.S_DEFINED], st[e, :ao.S_DEFINED]), (e, want, st[e])
        assert nf[e] == env.frame_slot(step, e, reset=True)
        assert (hist[e] == nf[e]).all() and (log[e] == 0).all()
        assert np.array_equal(env.render(want), frames[e]), (e, np.argwhere(env.render(want) != frames[e])[:4])


def _check_env_step(rp, act, env, seed, actions):
    """One teacher-forced agent step of every env (then the evaluator's observation-stack
    advance): the oracle starts from the device's own pre-step state and the given actions,
    and everything the kernels wrote is compared exactly.  Returns the oracle's results."""
    h, E = act.hip, act.E
    actions = np.asarray(actions, dtype=np.int32)
    act.actions.copy_(torch.from_numpy(actions))
    st0, log0, hist0 = _np(act.env_state), _np(act.ep_log), _np(act.st["hist"])
    step = int(act.step_counter.item())
    h.vec_env_step(act.env_state.data_ptr(), act.actions.data_ptr(), seed, act.step_counter.data_ptr(),
                   rp.frames.data_ptr(), act.env_params, act.reward.data_ptr(), act.done.data_ptr(),
                   act.new_frame.data_ptr(), act.ep_log.data_ptr(), _stream())
    h.frame_hist_step(act.st["hist"].data_ptr(), act.new_frame.data_ptr(), act.done.data_ptr(), E,
                      act.step_counter.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert int(act.step_counter.item()) == step + 1
    st1, log1, hist1 = _np(act.env_state), _np(act.ep_log), _np(act.st["hist"])
    r, d, nf = _np(act.reward), _np(act.done), _np(act.new_frame)
    frames = _np(rp.frames[act.new_frame.long()]).reshape(E, 84, 84)
    outs = []
    for e in range(E):
        o = env.step(st0[e], actions[e], e, seed, step, log0[e])
        tag = (step, e, int(actions[e]))
        assert nf[e] == env.frame_slot(step, e), (tag, nf[e])
        assert np.array_equal(o.state[:ao.S_DEFINED], st1[e, :ao.S_DEFINED]), (tag, o.state, st1[e])
        assert r[e] == o.reward and d[e] == o.done, (tag, r[e], o.reward, d[e], o.done)
        assert np.array_equal(o.ep_log[:3], log1[e, :3]), (tag, o.ep_log, log1[e])
        assert np.array_equal(o.frame, frames[e]), (tag, np.argwhere(o.frame != frames[e])[:4])
        want_hist = [nf[e]] * 4 if o.done else list(hist0[e, 1:]) + [nf[e]]
        assert list(hist1[e]) == want_hist, (tag, hist1[e], want_hist)
        outs.append(o)
    return outs


ENV_CONFIGS = [(18, 1, 1, 4, 9), (18, 0, 0, 4, 0), (6, 1, 1, 4, 0), (4, 0, 0, 1, 0)]  # A, life, clip, repeat, limit


# On gfx950 the device's draws match the fused rounding (one fma for 4 + 72 u and for
# 0.4 + 0.8 u): hipcc contracts both expressions.  _env_oracle decides it from the first reset.
@pytest.mark.parametrize("cfg", ENV_CONFIGS, ids=lambda c: "A%d-life%d-clip%d-rep%d-max%d" % c)
def test_env_step_matches_host_oracle(cuda, cfg):
    """150 teacher-forced steps of 33 envs under random actions: state, reward, done, the frame
    and its ring slot (the ring of 40 E frames wraps three times), ep_log and the observation
    stack are bit-exact against the host game."""
    A, life, clip, repeat, max_steps = cfg
    E, T, seed = 33, 150, 5
    rp, act = _shard(cuda, E, A, F=40 * E, seed=seed, life=life, clip=clip, repeat=repeat, max_steps=max_steps)
    env = _env_oracle(rp, act, cfg, seed)
    print("env oracle rounding of the Philox draws:", "fused (fma)" if env.fused else "unfused")
    _check_reset(rp, act, env, seed)
    rng = np.random.default_rng(1000 + 10 * A + life)
    hits = dones = resets = 0
    for _ in range(T):
        outs = _check_env_step(rp, act, env, seed, rng.integers(0, A, E))
        hits += sum(o.reward > 0 for o in outs)
        dones += sum(bool(o.done) for o in outs)
        resets += sum(o.reset_happened for o in outs)
    assert (T + 1) * E > 3 * rp.frame_capacity
    assert hits > 0  # enemies respawned through the step kernel's own draw
    if max_steps:    # the time limit ended every env's episodes, each with a full reset draw
        assert resets >= E * (T // max_steps) and dones >= resets


def _crafted_cases(cfg):
    """(name, {state field: value}, action, check(o, env, e, seed, step)) for the branches random
    play almost never reaches.  Base state: player at (40, 70), enemies in their rows at columns
    4 14 24 50 60 70 moving +-0.5, no bullet, 3 lives, episode return 5 after 17 steps."""
    X, Y, VX = ao.S_EX, ao.S_EY, ao.S_EVX
    overlap = {X: 39, Y: 70, VX: 0}                         # enemy 0 on top of the player
    bullet_hit = {ao.S_BACT: 1, ao.S_BX: 27, ao.S_BY: 24.5, VX + 2: 0}  # one step below enemy 2 (row 20), at rest
    rows = 8 + 6 * np.arange(6)
    NOOP, FIRE, UP, RIGHT, LEFT, DOWN = 0, 1, 2, 3, 4, 5

    def respawned(o, env, e, seed, step):
        return (o.state[X + 2] == env.spawn_x(ao.uniform4(seed, e * 64 + 2, step * 16 + 2)[0]) and o.state[Y + 2] == 8
                and o.state[ao.S_BACT] == 0)

    if cfg == (18, 1, 1, 4, 0):
        return [
            ("descent_then_crash_past_78", {Y + 5: 77, ao.S_T: 63}, NOOP,
             lambda o, *_: o.done == 1 and not o.reset_happened and o.state[ao.S_LIVES] == 2 and o.state[ao.S_T] == 67
             and (o.state[Y:Y + 6] == rows).all()),
            ("enemy_on_player", overlap, NOOP,
             lambda o, *_: o.done == 1 and not o.reset_happened and o.state[ao.S_LIVES] == 2 and o.reward == 0),
            ("last_life_game_over", {**overlap, ao.S_LIVES: 1}, NOOP,
             lambda o, *_: o.done == 1 and o.reset_happened and o.state[ao.S_LIVES] == 3 and o.state[ao.S_T] == 0
             and list(o.ep_log[:3]) == [5, 18, 5]),
            ("bullet_hit_respawn", bullet_hit, NOOP,
             lambda o, *a: o.reward == 1 and o.done == 0 and respawned(o, *a)),
            ("bullet_leaves_screen", {ao.S_BACT: 1, ao.S_BX: 41.5, ao.S_BY: 2}, NOOP,
             lambda o, *_: o.state[ao.S_BACT] == 0 and o.state[ao.S_BY] == -1 and o.reward == 0),
            ("left_wall", {ao.S_PX: 0}, LEFT, lambda o, *_: o.state[ao.S_PX] == 0),
            ("right_wall", {ao.S_PX: 80}, RIGHT, lambda o, *_: o.state[ao.S_PX] == 80),
            ("top_wall", {ao.S_PY: 42}, UP, lambda o, *_: o.state[ao.S_PY] == 42),
            ("bottom_wall", {ao.S_PY: 76}, DOWN, lambda o, *_: o.state[ao.S_PY] == 76),
        ]
    if cfg == (18, 0, 0, 4, 0):
        return [
            ("life_lost_is_not_done", {**overlap, **bullet_hit}, NOOP,
             lambda o, *_: o.done == 0 and o.state[ao.S_LIVES] == 2 and o.reward == 20 and o.state[ao.S_EPRET] == 25
             and o.state[ao.S_EPLEN] == 18 and o.ep_log[2] == 4),
            # the bullet fired now would hit enemy 4 in frame 2 (+20, see the control below): the
            # game over in frame 1 stops the repeat loop before that
            ("game_over_in_frame_1_of_4", {ao.S_LIVES: 1, ao.S_PY: 42, X: 39, Y: 42, VX: 0, X + 4: 38.5, VX + 4: 0},
             FIRE,
             lambda o, *_: o.done == 1 and o.reset_happened and o.reward == 0 and list(o.ep_log[:3]) == [5, 18, 5]),
            ("control_two_lives_frame_2_hit", {ao.S_LIVES: 2, ao.S_PY: 42, X: 39, Y: 42, VX: 0, X + 4: 38.5, VX + 4: 0},
             FIRE, lambda o, *_: o.done == 0 and o.reward == 20 and o.state[ao.S_LIVES] == 1),
        ]
    if cfg == (6, 1, 1, 4, 0):
        return [
            ("pong_game_ends_at_21", {**overlap, ao.S_POINTS: 20}, NOOP,
             lambda o, *_: o.done == 1 and o.reset_happened and o.reward == -1 and o.state[ao.S_POINTS] == 0
             and list(o.ep_log[:3]) == [4, 18, 5]),
            ("pong_point_lost", {**overlap, ao.S_POINTS: 3}, NOOP,
             lambda o, *_: o.done == 0 and o.reward == -1 and o.state[ao.S_POINTS] == 4 and o.state[ao.S_LIVES] == 3),
            ("hit_scores_one", bullet_hit, NOOP, lambda o, *a: o.reward == 1 and o.done == 0 and respawned(o, *a)),
            ("leftfire_at_the_wall", {ao.S_PX: 0}, 5,
             lambda o, *_: o.state[ao.S_PX] == 0 and o.state[ao.S_BACT] == 1 and o.state[ao.S_BY] == 56),
        ]
    assert cfg == (4, 0, 0, 1, 0)  # Breakout's four actions go through the a % 6 decode, one frame per step
    return [
        ("left_at_the_wall", {ao.S_PX: 0}, 3, lambda o, *_: o.state[ao.S_PX] == 0 and o.state[ao.S_T] == 1),
        ("right", {}, 2, lambda o, *_: o.state[ao.S_PX] == 41 and o.state[ao.S_BACT] == 0),
        ("fire", {}, 1, lambda o, *_: o.state[ao.S_PX] == 40 and o.state[ao.S_BACT] == 1 and o.state[ao.S_BY] == 65),
        ("noop", {}, 0, lambda o, *_: o.state[ao.S_PX] == 40 and o.state[ao.S_BACT] == 0),
    ]


@pytest.mark.parametrize("cfg", [(18, 1, 1, 4, 0), (18, 0, 0, 4, 0), (6, 1, 1, 4, 0), (4, 0, 0, 1, 0)],
                         ids=lambda c: "A%d-life%d-clip%d-rep%d-max%d" % c)
def test_env_crafted_states_match_host_oracle(cuda, cfg):
    """States written into env_state so that one step takes the rare branches (crash by descent
    and by overlap, game over with its full reset drawn at counter step 16 + 7, the Pong-style
    game end, bullet hit with its respawn draw, bullet leaving, walls, a lost life without
    episode_life, game over in the first of four frames).  Each case is compared exactly with
    the oracle and the oracle's result is checked to be the branch the case is named after.
    Run at a small step counter, at one above 2^32 and with a seed above 2^32."""
    cases = _crafted_cases(cfg)
    E = 12
    assert len(cases) <= E
    rp, act = _shard(cuda, E, cfg[0], F=40 * E, seed=5, life=cfg[1], clip=cfg[2], repeat=cfg[3], max_steps=cfg[4])
    env = _env_oracle(rp, act, cfg, 5)
    rng = np.random.default_rng(7)
    for seed, step in ((5, 3), (5, 2 ** 32 + 5), (2 ** 33 + 3, 9)):
        act.step_counter.fill_(step)
        _reset(rp, act, seed)
        _check_reset(rp, act, env, seed)
        states = _np(act.env_state).copy()
        actions = rng.integers(0, cfg[0], E)
        for e in range(E):
            states[e, ao.S_EX:ao.S_EX + 6] = [4, 14, 24, 50, 60, 70]
            states[e, ao.S_EVX:ao.S_EVX + 6] = [0.5, -0.5, 0.5, -0.5, 0.5, -0.5]
            states[e, ao.S_EPRET], states[e, ao.S_EPLEN] = 5, 17
        for e, (_, fields, action, _) in enumerate(cases):
            for k, v in fields.items():
                states[e, k] = v
            actions[e] = action
        act.env_state.copy_(torch.from_numpy(states))
        act.ep_log[:, 2] = 4
        outs = _check_env_step(rp, act, env, seed, actions)
        for e, (name, _, _, check) in enumerate(cases):
            assert check(outs[e], env, e, seed, step), (name, seed, step, outs[e])


@pytest.mark.parametrize("A", [1, 6, 18, 63])
def test_select_actions_matches_host(cuda, A):
    """select_actions_k == the host rule and the host Philox draw, over two blocks of 256
    threads, with exact eps 0 and 1 among the Ape-X ladder, Q rows with ties, a seed with a high
    word and a counter above 2^32."""
    from apex_amd import ops
    from apex_amd.algo.schedules import actor_epsilon

    h, E, seed = ops.hip(), 300, (7 << 32) | 0x1234
    rng = np.random.default_rng(A)
    q = rng.standard_normal((E, A)).astype(np.float32)
    q[20:120] = np.round(q[20:120])              # many ties
    for base in (0, 1, 2):                       # under eps = 0, eps = 1 and a ladder eps
        q[base] = 0.25                           # all equal -> action 0
        q[base + 5] = np.arange(A)               # the maximum at the last index
        q[base + 10] = 0
        q[base + 10, [A // 2, A - 1]] = 3        # a tie between the middle and the last index
    eps = np.asarray(actor_epsilon(np.arange(E, dtype=np.float64), E, 0.4, 7.0), dtype=np.float32)
    eps[0::5], eps[1::5] = 0.0, 1.0
    counters = (0, 7, 2 ** 32 + 1)
    for k, c in enumerate(counters):             # eps equal to the env's own u0: "not (u0 > eps)" explores
        for e in range(200 + 10 * k, 210 + 10 * k):
            eps[e] = ao.uniform4(seed, e, c)[0]
    qd, qneg, epsd = (torch.from_numpy(x).to(cuda) for x in (q, -q, eps))
    out, out_neg = (torch.full((E,), -1, dtype=torch.int32, device=cuda) for _ in range(2))
    ctr = torch.zeros(1, dtype=torch.int64, device=cuda)
    refs = {}
    for k, c in enumerate(counters):
        ctr.fill_(c)
        h.select_actions(qd.data_ptr(), E, A, epsd.data_ptr(), seed, ctr.data_ptr(), out.data_ptr(), _stream())
        h.select_actions(qneg.data_ptr(), E, A, epsd.data_ptr(), seed, ctr.data_ptr(), out_neg.data_ptr(), _stream())
        torch.cuda.synchronize()
        got, got_neg = _np(out), _np(out_neg)
        refs[c] = ao.select_actions_ref(q, eps, seed, c)
        assert np.array_equal(got, refs[c]), (c, np.flatnonzero(got != refs[c])[:8])
        assert np.array_equal(got[eps == 1], got_neg[eps == 1])          # eps = 1: Q plays no part
        assert np.array_equal(got[eps == 0], q.argmax(1)[eps == 0])      # eps = 0: the first argmax
        assert np.array_equal(got_neg[eps == 0], (-q).argmax(1)[eps == 0])
        for e in range(200 + 10 * k, 210 + 10 * k):                      # u0 == eps: the random action
            assert got[e] == min(int(ao.uniform4(seed, e, c)[1] * np.float32(A)), A - 1), (c, e)
    if A > 1:  # the counter's high word and the seed's high word reach the draw
        assert not np.array_equal(refs[2 ** 32 + 1], ao.select_actions_ref(q, eps, seed, 1))
        assert not np.array_equal(refs[7], ao.select_actions_ref(q, eps, seed & 0xFFFFFFFF, 7))
        assert not np.array_equal(refs[0], refs[7])


def test_fused_eps_greedy_epilogue_tie_goes_to_lower_index(cuda):
    """The heads_fwd epilogue's wave (value, index) reduction on Q rows with a three-way tie for
    the maximum (advantage rows 3, 7 and 17 made identical): the host rule's first argmax."""
    from apex_amd.models.dqn import DuelingDQN
    from apex_amd.models.fused import HipDuelingNet, NetWorkspace

    E, A = 256, 18
    rp, act = _shard(cuda, E, A, C=8192, seed=5, staged=2)
    model = DuelingDQN.from_shapes((4, 84, 84), A).to(cuda)
    with torch.no_grad():
        w, b = model.advantage[2].weight, model.advantage[2].bias
        w[7].copy_(w[3])
        w[17].copy_(w[3])
        b[3] = b[7] = b[17] = 1000.0  # far above any advantage of the freshly initialised net
    net = HipDuelingNet(model)
    ws = NetWorkspace(E, A, cuda)
    ws.q = act.q
    net(rp.frames, ws, act.st["hist"], act=act.act_args())
    torch.cuda.synchronize()
    q = _np(act.q)
    assert (q[:, 3] == q[:, 7]).all() and (q[:, 3] == q[:, 17]).all() and (q.max(1) == q[:, 3]).all()
    want = ao.select_actions_ref(q, _np(act.eps), act.seed ^ 0x5E1EC7, int(act.step_counter.item()))
    got = _np(act.actions)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert (got == 3).sum() > E // 2 and (got == 7).sum() + (got == 17).sum() < E // 8


def _episode_ends(rng, n, T, E):
    """done[t, e] for episode lengths drawn from 1 .. 2n+1; env e starts with a long episode
    (2n+1) followed directly by one of length e mod (n+1) + 1, so every length from 1 to n+1
    occurs right behind a full window / a full drain backlog."""
    done = np.zeros((T, E), dtype=bool)
    for e in range(E):
        lengths = [2 * n + 1, e % (n + 1) + 1]
        while sum(lengths) < T:
            lengths.append(int(rng.integers(1, 2 * n + 2)))
        ends = np.cumsum(lengths) - 1
        done[ends[ends < T], e] = True
    return done


@pytest.mark.parametrize("mode", ["reference", "textbook"])
@pytest.mark.parametrize("A,n", [(18, 3), (6, 1), (18, 5)])
def test_nstep_controlled_episodes_match_oracle(cuda, mode, A, n):
    """nstep_emit_k on inputs the test controls (random rewards in [-2, 2], a running frame
    counter, episodes of every length from 1 to 2n+1, the ring of 8 E slots rewritten five
    times): each step, each env against NStepOracle -- whether a row was emitted, its slot,
    s_ids / action / done (and s2_ids when not done) exactly, the observation stack exactly,
    return and priority within the float32 bound of the oracle row
    ((n + 6) 2^-23 (sum gamma^i |r_i| + gamma^n |max Q| + |Q(s0, a0)| + 1e-6): one rounding per
    float32 operation plus powf's few ulp).  Reference mode must show the stale-Q window (Q3)
    and the first-step terminal (Q4); textbook mode must conserve BatchStorage's transitions."""
    E, T, gamma = 16, 40, 0.99
    C = 8 * E
    rp, act = _shard(cuda, E, A, n=n, C=C, mode=mode, gamma=gamma)
    h = act.hip
    rng = np.random.default_rng(10 * n + A)
    plan = _episode_ends(rng, n, T, E)
    orcs = [ao.NStepOracle(n, gamma, mode, hist) for hist in _np(act.st["hist"])]
    mirror = {k: _np(getattr(rp, k)).copy() for k in TABLES}
    errors, emitted = [], []

    def check(ok, *what):
        if not ok:
            errors.append(what)

    for t in range(T):
        q = rng.standard_normal((E, A)).astype(np.float32)
        a = rng.integers(0, A, E).astype(np.int32)
        r = rng.uniform(-2, 2, E).astype(np.float32)
        nf = ((t + 1) * E + np.arange(E)).astype(np.int32)
        for dst, src in ((act.q, q), (act.actions, a), (act.reward, r), (act.done, plan[t].astype(np.float32)),
                         (act.new_frame, nf)):
            dst.copy_(torch.from_numpy(src))
        h.nstep_emit(act.nstep, act.q.data_ptr(), act.actions.data_ptr(), act.reward.data_ptr(), act.done.data_ptr(),
                     act.new_frame.data_ptr(), act.step_counter.data_ptr(), act.slot.data_ptr(), act.prio.data_ptr(),
                     _stream(), False)
        h.bump_counter(act.step_counter.data_ptr(), 1, 1, _stream())
        torch.cuda.synchronize()
        slot, prio, hist = _np(act.slot), _np(act.prio), _np(act.st["hist"])
        dev = {k: _np(getattr(rp, k)) for k in TABLES}
        for e in range(E):
            row = orcs[e].add(a[e], r[e], bool(plan[t, e]), q[e], nf[e])
            sl = (t * E + e) % C
            check(slot[e] == sl, "slot", t, e, slot[e])
            check((prio[e] > 0) == (row is not None), "emitted", t, e, prio[e], row)
            check(tuple(hist[e]) == orcs[e].hist, "hist", t, e, hist[e], orcs[e].hist)
            if not prio[e] > 0:
                continue
            emitted.append((tuple(dev["s_ids"][sl]), int(dev["action"][sl]), float(dev["done"][sl])))
            for k in TABLES:
                mirror[k][sl] = dev[k][sl]
            if row is None:
                continue
            check(tuple(dev["s_ids"][sl]) == row.s_ids, "s_ids", t, e, dev["s_ids"][sl], row.s_ids)
            check(dev["action"][sl] == row.action, "action", t, e)
            check(dev["done"][sl] == row.done, "done", t, e)
            if not row.done:
                check(tuple(dev["s2_ids"][sl]) == row.s2_ids, "s2_ids", t, e, dev["s2_ids"][sl], row.s2_ids)
            check(abs(float(dev["reward"][sl]) - row.reward) <= row.bound, "return", t, e, dev["reward"][sl], row)
            check(abs(float(prio[e]) - row.prio) <= row.bound, "prio", t, e, prio[e], row)
        for k in TABLES:  # an env that emitted nothing left its slot alone
            check(np.array_equal(mirror[k], dev[k]), "untouched rows", k, t)
    assert int(act.step_counter.item()) == T
    rows = [r for o in orcs for r in o.rows]
    in_flight = _np(act.st["drain_meta"])[:, 1]
    lost = len(rows) - len(emitted) - int(in_flight.sum())
    print(f"nstep {mode} n={n}: {len(rows)} oracle rows, {len(emitted)} emitted, {int(in_flight.sum())} in flight, "
          f"{lost} lost, {len(errors)} mismatches")
    assert lost == 0, (lost, errors[:4])
    assert not errors, (len(errors), errors[:6])
    if mode == "reference":
        assert sum(o.first_step_terminal for o in orcs) > 0                 # Q4 occurred
        assert n == 1 or sum(o.stale_q for o in orcs) > 0                   # Q3 (impossible for n = 1)
    else:
        # conservation: what was emitted plus what is still queued (<= n per env) is exactly
        # BatchStorage's multiset -- every (s, a) of a finished episode once, nothing dropped
        assert (in_flight <= n).all() and list(in_flight) == [len(o.pending) for o in orcs]
        key = lambda r: (r.s_ids, r.action, r.done)  # noqa: E731
        assert Counter(emitted) + Counter(key(r) for o in orcs for r in o.pending) == Counter(key(r) for r in rows)
        assert max(len(o.pending) for o in orcs) > 0 or n == 1


@pytest.mark.parametrize("mode", ["reference", "textbook"])
def test_nstep_bump_path_equals_grid_path(cuda, mode):
    """E = 1100 envs, more than the 1024 threads of the single workgroup that advances the step
    counter itself: that launch (bump=True, strided) leaves window state, rows, slots,
    priorities and observation stacks bit-identical to the grid launch followed by
    bump_counter, and a staged handle followed by apply_staged_rows gives the same tables."""
    E, A, n, T = 1100, 18, 3, 6
    shards = [_shard(cuda, E, A, n=n, C=4 * E, F=2 * E, mode=mode, staged=2 if i == 2 else 0) for i in range(3)]
    for rp, _ in shards:
        rp.action.fill_(99)
        rp.reward.fill_(-7.0)
    rp0, a0 = shards[0]
    h, s = a0.hip, _stream()
    g = torch.Generator(device="cpu").manual_seed(11)
    n_emitted = n_idle = max_queue = 0
    for t in range(T):
        inputs = {"q": torch.randn(E, A, generator=g), "actions": torch.randint(0, A, (E,), generator=g).int(),
                  "reward": torch.rand(E, generator=g) * 4 - 2, "done": (torch.rand(E, generator=g) < 0.3).float(),
                  "new_frame": (torch.arange(E) + (t + 1) * E).int()}
        before = {k: getattr(rp0, k).clone() for k in TABLES}
        p = t % 2
        for i, (rp, act) in enumerate(shards):
            for k, v in inputs.items():
                getattr(act, k).copy_(v)
            args = (act.q.data_ptr(), act.actions.data_ptr(), act.reward.data_ptr(), act.done.data_ptr(),
                    act.new_frame.data_ptr(), act.step_counter.data_ptr())
            if i == 0:
                h.nstep_emit(act.nstep, *args, act.slot.data_ptr(), act.prio.data_ptr(), s, False)
                h.bump_counter(act.step_counter.data_ptr(), 1, 1, s)
            elif i == 1:
                h.nstep_emit(act.nstep, *args, act.slot.data_ptr(), act.prio.data_ptr(), s, True)
            else:
                h.nstep_emit(act.stage_nstep[p], *args, act.stage_slot[p].data_ptr(), act.stage_prio[p].data_ptr(), s,
                             True)
                act.apply_rows(p)
        torch.cuda.synchronize()
        for i in (1, 2):
            rp, act = shards[i]
            assert int(act.step_counter.item()) == int(a0.step_counter.item()) == t + 1
            for k in a0.st:
                assert torch.equal(a0.st[k], act.st[k]), (k, t, i)
            slot, prio = (act.slot, act.prio) if i == 1 else (act.stage_slot[p], act.stage_prio[p])
            assert torch.equal(a0.slot, slot) and torch.equal(a0.prio, prio), (t, i)
            for k in TABLES:
                assert torch.equal(getattr(rp0, k), getattr(rp, k)), (k, t, i)
        assert torch.equal(a0.slot.long(), (torch.arange(E, device=cuda) + t * E) % (4 * E))
        idle = a0.slot[~(a0.prio > 0)].long()
        for k in TABLES:  # envs that emitted nothing left their slot as it was
            assert torch.equal(getattr(rp0, k)[idle], before[k][idle]), (k, t)
        n_idle += idle.numel()
        n_emitted += E - idle.numel()
        max_queue = max(max_queue, int(a0.st["drain_meta"][:, 1].max()))
    assert n_idle > 0 and n_emitted > E  # both kinds of env occurred
    assert (max_queue > 0) == (mode == "textbook")


def test_frame_hist_step_matches_host(cuda):
    """The evaluator's observation-stack advance over two blocks of 256 threads: shifted by the
    new frame, or collapsed to it where done; the counter goes up by one per launch."""
    from apex_amd import ops

    h, E, start = ops.hip(), 300, 2 ** 32 + 9
    rng = np.random.default_rng(3)
    hist = rng.integers(0, 100000, (E, 4)).astype(np.int32)
    hist_d = torch.from_numpy(hist).to(cuda)
    ctr = torch.full((1,), start, dtype=torch.int64, device=cuda)
    for k in range(3):
        nf = rng.integers(0, 100000, E).astype(np.int32)
        done = (rng.random(E) < 0.3).astype(np.float32)
        done[[0, 255, 256, 299]] = [1, 0, 1, 1]
        nf_d, done_d = torch.from_numpy(nf).to(cuda), torch.from_numpy(done).to(cuda)
        h.frame_hist_step(hist_d.data_ptr(), nf_d.data_ptr(), done_d.data_ptr(), E, ctr.data_ptr(), _stream())
        torch.cuda.synchronize()
        hist = np.where(done[:, None] > 0, np.repeat(nf[:, None], 4, 1), np.concatenate([hist[:, 1:], nf[:, None]], 1))
        assert np.array_equal(_np(hist_d), hist), k
        assert int(ctr.item()) == start + k + 1
