"""atari_rollout (one launch = n greedy steps of every evaluator env), GPUEvaluator.rollout /
poll_ring, AtariEvaluator and train.py --eval-mode against the stepwise evaluator, the host
game (tests/actor_oracle.py) and the fp64 module.  Shapes: <= 8 envs, <= 24 steps (60 once for
the episode ring's overflow)."""
import re

import numpy as np
import pytest
import torch

from . import actor_oracle as ao
from . import atari_rollout_fixtures as fx

pytestmark = pytest.mark.gpu

BUFFERS = ("env_state", "hist", "frames", "new_frame", "ep_log", "reward", "done", "actions", "counter")


def _evaluator(dev, model, A, E=fx.E, seed=fx.ENV_SEED, life=fx.EPISODE_LIFE, max_steps=fx.MAX_EPISODE_STEPS, eps=0.0,
               **kw):
    from apex_amd.engine.evaluator import GPUEvaluator

    return GPUEvaluator(model, n_envs=E, n_actions=A, device=dev, seed=seed, episode_life=bool(life),
                        max_episode_steps=max_steps, epsilon=eps, **kw)


def _trace(dev, E, T, A, fill=0.0):
    return {"q": torch.full((E, T, A), fill, device=dev), "act": torch.full((E, T), -7, dtype=torch.int32, device=dev),
            "rew": torch.full((E, T), fill, device=dev), "done": torch.full((E, T), fill, device=dev)}


def _assert_same(a, b, names=BUFFERS, what=""):
    torch.cuda.synchronize()
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        assert torch.equal(x, y), (what, n, int((x != y).sum()))


def _need_gap(case, E=fx.E, steps=fx.STEPS):
    ok, g = fx.gap_ok(case, E, steps)   # recomputed on the CPU; a free-running comparison needs it
    assert ok, f"fixture {case}: top-2 Q gap {g:.3e} < {fx.GAP} x max|Q| -- the comparison is not meaningful"


def _stepwise_env(ev, actions):
    """vec_env_step + frame_hist_step of GPUEvaluator.step() under given actions."""
    h, s = ev.hip, ev._stream()
    ev.actions.copy_(actions)
    h.vec_env_step(ev.env_state.data_ptr(), ev.actions.data_ptr(), ev.seed, ev.counter.data_ptr(),
                   ev.frames.data_ptr(), ev.params, ev.reward.data_ptr(), ev.done.data_ptr(),
                   ev.new_frame.data_ptr(), ev.ep_log.data_ptr(), s)
    h.frame_hist_step(ev.hist.data_ptr(), ev.new_frame.data_ptr(), ev.done.data_ptr(), ev.E, ev.counter.data_ptr(), s)


@pytest.fixture(scope="module", params=sorted(fx.CASES))
def traced(request, cuda):
    """rollout(24, trace) of a fixture case + the teacher-forced stepwise replay of its actions
    (computed once, shared, not modified)."""
    from apex_amd.engine.hbm_replay import FRAME_BYTES

    case = request.param
    A, ms = fx.CASES[case]
    model = fx.make_model(A, ms).to(cuda)
    ev_r, ev_s = _evaluator(cuda, model, A), _evaluator(cuda, model, A)
    tr = _trace(cuda, fx.E, fx.STEPS, A)
    counter0 = int(ev_r.counter.item())
    ev_r.rollout(fx.STEPS, tr)
    torch.cuda.synchronize()
    obs, rews, dones = [], [], []
    for k in range(fx.STEPS):
        o = torch.empty(fx.E, 4, 84, 84, dtype=torch.uint8, device=cuda)
        ev_s.hip.gather_frames(ev_s.frames.data_ptr(), FRAME_BYTES, ev_s.hist.data_ptr(), fx.E, 4, o.data_ptr(),
                               ev_s._stream())
        obs.append(o)
        _stepwise_env(ev_s, tr["act"][:, k])
        rews.append(ev_s.reward.clone())
        dones.append(ev_s.done.clone())
    torch.cuda.synchronize()
    return dict(case=case, A=A, model=model, ev_r=ev_r, ev_s=ev_s, tr=tr, counter0=counter0,
                obs=torch.stack(obs, 1), rews=torch.stack(rews, 1), dones=torch.stack(dones, 1))


def test_teacher_forced_env_and_bookkeeping(traced):
    """With the traced actions replayed through vec_env_step / frame_hist_step, every evaluator
    buffer is bit-equal after 24 steps (3 time-limit dones with reset draws per env, 3 wraps of
    the frame ring), the traced rewards / dones are the per-step values and the traced action is
    select_actions' choice on the traced Q."""
    t = traced
    ev_r, ev_s, tr = t["ev_r"], t["ev_s"], t["tr"]
    assert int(ev_r.counter.item()) == t["counter0"] + fx.STEPS and ev_r.steps == fx.STEPS
    _assert_same(ev_r, ev_s, [n for n in BUFFERS if n != "actions"])
    assert torch.equal(ev_r.actions, tr["act"][:, -1])
    assert torch.equal(tr["rew"], t["rews"]) and torch.equal(tr["done"], t["dones"])
    assert float(tr["done"].sum()) >= 3 * fx.E
    q = tr["q"].cpu().numpy()
    eps = np.zeros(fx.E, np.float32)
    for k in range(fx.STEPS):
        want = ao.select_actions_ref(q[:, k], eps, fx.ENV_SEED ^ fx.ACT_XOR, t["counter0"] + k)
        assert np.array_equal(tr["act"][:, k].cpu().numpy(), want), k


def test_trace_q_is_the_fp64_q(traced):
    """The rollout's Q on the observations it acted on, against the fp64 module: within the
    project's Q bound (rtol 1e-4, atol 1e-4 x max|Q|) and its scaled error max|q - q64| / max|q64|
    at most 2x the larger of the stepwise F32DuelingNet's and the torch fp32 module's on the
    same observations (another accumulation order of the same precision class).
    Measured on MI355X: see profiles/atari_eval.md."""
    from apex_amd.models.fused_f32 import F32DuelingNet, F32Workspace

    t = traced
    A, dev = t["A"], t["model"].features[0].weight.device
    x = t["obs"].reshape(fx.E * fx.STEPS, 4, 84, 84).contiguous()     # row e * STEPS + k
    with torch.no_grad():
        q64 = fx.make_model(*fx.CASES[t["case"]]).double()(x.cpu().double())
        q_torch = t["model"](x.float()).cpu()
    net = F32DuelingNet(t["model"])
    ws = F32Workspace(x.shape[0], A, dev)
    q_step = net(x, ws).clone().cpu()
    q_roll = t["tr"]["q"].reshape(fx.E * fx.STEPS, A).cpu()
    scale = float(q64.abs().max())
    err = {n: float((v.double() - q64).abs().max()) / scale
           for n, v in (("rollout", q_roll), ("stepwise", q_step), ("torch", q_torch))}
    print(f"{t['case']}: scaled Q error vs fp64: " + ", ".join(f"{n} {e:.3e}" for n, e in err.items()))
    torch.testing.assert_close(q_roll.double(), q64, rtol=fx.Q_RTOL, atol=fx.Q_ATOL * scale)
    assert err["rollout"] <= 2.0 * max(err["stepwise"], err["torch"]), err


@pytest.mark.parametrize("case", sorted(fx.CASES))
@pytest.mark.parametrize("E,n", [(1, 1), (1, 24), (3, 5), (3, 24), (8, 1), (8, 5), (8, 24)])
def test_free_running_equals_stepwise(cuda, case, E, n):
    """From one reset, run(n) and rollout(n) (and, at 24 steps, run(5); rollout(11); run(8)) leave
    every buffer and the poll() results bit-equal."""
    _need_gap(case, E, n)
    A, ms = fx.CASES[case]
    model = fx.make_model(A, ms).to(cuda)
    ev_a, ev_b = _evaluator(cuda, model, A, E=E), _evaluator(cuda, model, A, E=E)
    ev_a.run(n)
    ev_b.rollout(n)
    _assert_same(ev_a, ev_b, what="rollout")
    assert ev_a.steps == ev_b.steps == n
    pa = ev_a.poll()
    assert pa == ev_b.poll() and ev_a.episodes == ev_b.episodes
    if n == 24:
        assert len(pa) == E
        ev_c = _evaluator(cuda, model, A, E=E)
        ev_c.run(5)
        ev_c.rollout(11)
        ev_c.run(8)
        _assert_same(ev_a, ev_c, what="mixed")
        assert ev_c.poll() == pa


def _crafted(A, which, lives=3):
    """State fields that make the first agent step take a named branch (player at (40, 70))."""
    f = {ao.S_PX: 40, ao.S_PY: 70, ao.S_LIVES: lives, ao.S_BACT: 0, ao.S_T: 0}
    for k in range(6):
        f[ao.S_EX + k], f[ao.S_EY + k], f[ao.S_EVX + k] = 4 + 12 * k, 8 + 6 * k, 0.5
    if which == "crash":      # enemy 0 one frame from the player
        f[ao.S_EX], f[ao.S_EY], f[ao.S_EVX] = 38.5, 70, 0.5
    else:                     # a bullet one frame under enemy 0
        f[ao.S_EX], f[ao.S_EY], f[ao.S_EVX] = 20, 8, 0.0
        f[ao.S_BACT], f[ao.S_BX], f[ao.S_BY] = 1, 23, 12.5
    return f


@pytest.mark.parametrize("A,life", [(18, 1), (18, 0), (6, 1)])
def test_crafted_states_match_host_oracle(cuda, A, life):
    """States written into env_state before the launch: a life loss (done with episode_life, none
    without; the game goes on), game over at lives = 1 with the reset draw at word + 7, a bullet
    hit (20 points, 1 at A = 6) with its respawn draw.  Three steps under a constant-argmax model
    (NOOP) equal VecEnvOracle exactly."""
    E, favour, seed = 3, 0, fx.ENV_SEED
    model = fx.constant_argmax_model(A, favour).to(cuda)
    ev = _evaluator(cuda, model, A, E=E, life=life, max_steps=0)
    host = fx.HostEvaluator(A, E, seed, episode_life=life, max_episode_steps=0)
    torch.cuda.synchronize()
    assert np.array_equal(ev.env_state.cpu().numpy()[:, :ao.S_DEFINED], host.state[:, :ao.S_DEFINED])
    cases = [_crafted(A, "crash"), _crafted(A, "crash", lives=1), _crafted(A, "bullet")]
    st = host.state.copy()
    for e, fields in enumerate(cases):
        for k, v in fields.items():
            st[e, k] = v
    host.state = st.copy()
    ev.env_state.copy_(torch.from_numpy(st))
    tr = _trace(cuda, E, 3, A)
    ev.rollout(3, tr)
    torch.cuda.synchronize()
    first = None
    for k in range(3):
        host.step(actions=np.full(E, favour))
        if k == 0:
            first = (host.reward.copy(), host.done.copy(), host.state.copy())
    # the branches the cases are named after happened (on the host model)
    r0, d0, s0 = first
    if A == 18:
        assert d0[0] == float(life) and s0[0, ao.S_LIVES] == 2 and s0[0, ao.S_T] == 4          # life lost, game on
        assert d0[1] == 1 and s0[1, ao.S_LIVES] == 3 and s0[1, ao.S_T] == 0                    # game over + reset
        want_ex = [host.env.spawn_x(ao.uniform4(seed, 1 * 64 + 32 + j, 0 * 16 + 7)[0]) for j in range(6)]
        assert np.array_equal(s0[1, ao.S_EX:ao.S_EX + 6], np.asarray(want_ex, np.float32))
        assert r0[2] == 20
    else:
        assert r0[0] == -1 and s0[0, ao.S_POINTS] == 1 and r0[2] == 1
    assert s0[2, ao.S_BACT] == 0 and s0[2, ao.S_EY] == 8
    assert s0[2, ao.S_EX] == host.env.spawn_x(ao.uniform4(seed, 2 * 64 + 0, 0 * 16 + 2 + 0)[0])  # the respawn draw
    assert np.array_equal(tr["act"].cpu().numpy(), np.full((E, 3), favour))
    assert np.array_equal(tr["rew"][:, 0].cpu().numpy(), r0) and np.array_equal(tr["done"][:, 0].cpu().numpy(), d0)
    assert np.array_equal(ev.env_state.cpu().numpy()[:, :ao.S_DEFINED], host.state[:, :ao.S_DEFINED])
    assert np.array_equal(ev.ep_log.cpu().numpy(), host.ep_log)
    assert np.array_equal(ev.reward.cpu().numpy(), host.reward) and np.array_equal(ev.done.cpu().numpy(), host.done)
    assert np.array_equal(ev.hist.cpu().numpy(), host.hist)
    assert np.array_equal(ev.frames.cpu().numpy().reshape(-1, 84, 84), host.frames)
    assert int(ev.counter.item()) == 3


@pytest.mark.parametrize("A", [18, 6])
def test_eps_one_takes_the_host_random_actions(cuda, A):
    E, n = 8, 8
    ev = _evaluator(cuda, fx.make_model(A, 1).to(cuda), A, eps=1.0)
    tr = _trace(cuda, E, n, A)
    ev.rollout(n, tr)
    torch.cuda.synchronize()
    got = tr["act"].cpu().numpy()
    q = tr["q"].cpu().numpy()
    for k in range(n):
        want = ao.select_actions_ref(q[:, k], np.ones(E, np.float32), fx.ENV_SEED ^ fx.ACT_XOR, k)
        rand = [min(int(ao.uniform4(fx.ENV_SEED ^ fx.ACT_XOR, e, k)[1] * np.float32(A)), A - 1) for e in range(E)]
        assert np.array_equal(got[:, k], want) and np.array_equal(want, rand), k
    assert len(np.unique(got)) > 2


def _episodes_stepwise(ev, n):
    """Per env, the (return, length) of every episode n stepwise steps end, in order."""
    eps = [[] for _ in range(ev.E)]
    for _ in range(n):
        ev.step()
        done, log = ev.done.cpu(), ev.ep_log.cpu()
        for e in range(ev.E):
            if done[e] > 0:
                eps[e].append((float(log[e, 0]), float(log[e, 1])))
    return eps


@pytest.mark.parametrize("n", [24, 60])
def test_episode_ring(cuda, n):
    """max_episode_steps = 3: poll_ring() returns every episode of a 24-step rollout per env in
    order (poll() one per env, as always); after 60 steps the newest 16 per env."""
    A, E, FIRE = 18, 8, 1
    model = fx.constant_argmax_model(A, FIRE).to(cuda)
    ev_s, ev_r = (_evaluator(cuda, model, A, max_steps=3) for _ in range(2))
    want = _episodes_stepwise(ev_s, n)
    ev_r.rollout(n)
    _assert_same(ev_s, ev_r)
    assert all(len(w) >= n // 3 for w in want)
    R = ev_r.RING
    assert ev_r.poll_ring() == [ep for w in want for ep in w[-R:]]
    assert ev_r.episodes == sum(len(w) for w in want)
    assert ev_r.poll_ring() == []
    assert ev_r.poll() == ev_s.poll() == [w[-1] for w in want]
    assert torch.equal(ev_s.ep_ring, torch.zeros_like(ev_s.ep_ring)), "only the rollout writes the ring"


def test_trace_off_equals_trace_on_and_guards(cuda):
    case = "a18"
    _need_gap(case, fx.E, 8)
    A, ms = fx.CASES[case]
    model = fx.make_model(A, ms).to(cuda)
    ev_off, ev_on, ev_short = (_evaluator(cuda, model, A) for _ in range(3))
    ev_off.rollout(8)
    full = _trace(cuda, fx.E, 8, A)
    ev_on.rollout(8, full)
    _assert_same(ev_off, ev_on)
    SENT = -12345.0
    short = _trace(cuda, fx.E + 1, 5, A, fill=SENT)   # a guard row past E; steps 5..7 are past trace_T
    ev_short.rollout(8, short)
    _assert_same(ev_off, ev_short)
    for k in ("q", "rew", "done"):
        assert torch.equal(short[k][:fx.E], full[k][:, :5]), k
        assert bool((short[k][fx.E] == SENT).all()), k
    assert torch.equal(short["act"][:fx.E], full["act"][:, :5]) and bool((short["act"][fx.E] == -7).all())


def test_launcher_validation(cuda):
    from apex_amd.engine.hbm_replay import FRAME_BYTES

    A = 18
    model = fx.make_model(A, 0).to(cuda)
    ev = _evaluator(cuda, model, A)
    h = ev.hip
    good = ev._rollout_args()
    good["n_steps"] = 1

    def params(E=8, A=18, fb=FRAME_BYTES, F=None):
        return h.VecEnvParams(E, A, fb, 8 * E if F is None else F, 4, 0, 1, 7)

    def bad(p=None, **kw):
        d = dict(good)
        for k, v in kw.items():
            if v is None:
                d.pop(k, None)
            else:
                d[k] = v
        with pytest.raises(ValueError):
            h.atari_rollout(h.make_atari_rollout(params() if p is None else p, d), ev._stream())

    bad(n_steps=0)
    bad(n_steps=10001)
    bad(params(E=0, F=0))
    bad(params(E=65))
    bad(params(A=7))
    bad(params(A=0))
    bad(params(F=8 * 8 + 1))
    bad(params(fb=FRAME_BYTES - 4))
    for key in ("w1", "b1", "w2p", "b2", "w3p", "b3", "wfc1p", "ba1", "bv1", "wa2", "ba2", "wv2", "bv2", "eps",
                "counter", "env_state", "hist", "frames", "new_frame", "ep_log", "reward", "done", "actions"):
        bad(**{key: None})
    tr = _trace(cuda, 8, 4, A)
    full = dict(trace_q=tr["q"].data_ptr(), trace_act=tr["act"].data_ptr(), trace_rew=tr["rew"].data_ptr(),
                trace_done=tr["done"].data_ptr(), trace_T=4)
    for key in ("trace_q", "trace_act", "trace_rew", "trace_done"):
        bad(**{**full, key: None})
    bad(**{**full, "trace_T": 0})
    torch.cuda.synchronize()
    assert int(ev.counter.item()) == 0 and ev.steps == 0      # nothing ran
    # the one-launch rollout is the fp32 HIP forward's
    with pytest.raises(ValueError, match="bf16"):
        _evaluator(cuda, model, A, dtype="bf16").rollout(1)
    with pytest.raises(ValueError, match="torch"):
        _evaluator(cuda, model, A, forward="torch").rollout(1)
    h.atari_rollout(h.make_atari_rollout(params(), {**good, **full}), ev._stream())   # and the good one runs
    torch.cuda.synchronize()


def test_snapshot_isolation(cuda):
    """The source weights overwritten on the training stream right after launch(): the landed
    result equals a synchronous rollout with the original weights."""
    from apex_amd.engine.evaluator import AtariEvaluator
    from apex_amd.models.fused import make_hip_net

    case = "a18"
    _need_gap(case)
    A, ms = fx.CASES[case]
    src = fx.make_model(A, ms).to(cuda)
    src_flat, src_net = src.flatten_parameters(), None
    src_net = make_hip_net(src, "fp32")
    keep_flat = src_flat.clone()
    other = fx.make_model(A, ms + 7).to(cuda)
    ev = _evaluator(cuda, other, A)
    ae = AtariEvaluator(ev)
    assert ae.launch(src_flat, src_net, fx.STEPS, tag=3) is True
    src_flat.zero_()
    src_net.arena.zero_()
    res = ae.wait()
    assert res["tag"] == 3 and ae.poll() is None
    ref_model = fx.make_model(A, ms).to(cuda)
    ref = _evaluator(cuda, ref_model, A)
    ref.rollout(fx.STEPS)
    _assert_same(ev, ref)
    assert torch.equal(ev.flat, keep_flat)
    assert res["episodes"] == ref.poll_ring() and len(res["episodes"]) >= 3 * fx.E
    run_ret, run_len = ref.running()
    assert res["running_return"] == run_ret.tolist() and res["running_length"] == run_len.tolist()
    assert res["total_episodes"] == ref.episodes


def test_training_left_bit_identical(cuda):
    """N engine steps with AtariEvaluator launches interleaved == N steps without."""
    from apex_amd.engine.apex import ApexEngine, EngineConfig
    from apex_amd.engine.evaluator import AtariEvaluator
    from apex_amd.engine.learner import LearnerConfig

    def engine():
        cfg = EngineConfig(n_envs=64, replay_capacity=4096, threshold_size=2048, overlap=True, use_graphs=True,
                           publish_param_interval=4, target_update_interval=6,
                           learner=LearnerConfig(batch_size=256, forward="hip"))
        torch.manual_seed(0)
        eng = ApexEngine(cfg, cuda)
        eng.fill()
        eng.capture()
        return eng

    eng_a, eng_b = engine(), engine()
    src_model = eng_a.actor_model if hasattr(eng_a, "actor_model") else eng_a.learner.model
    ae = AtariEvaluator(_evaluator(cuda, src_model, 18, max_steps=50))
    launched = 0
    for i in range(12):
        eng_a.train_step()
        eng_b.train_step()
        if i % 3 == 0:
            flat, net = ((eng_a.actor_flat, eng_a.actor_net) if hasattr(eng_a, "actor_flat")
                         else (eng_a.learner.flat, eng_a.learner.net))
            launched += bool(ae.launch(flat, net, 12, tag=i))
    res = ae.wait()
    torch.cuda.synchronize()
    assert launched >= 1 and res is not None
    la, lb = eng_a.learner, eng_b.learner
    assert eng_a.learn_steps == eng_b.learn_steps
    for name in ("flat", "tflat", "opt_s1", "opt_s2"):
        assert torch.equal(getattr(la, name), getattr(lb, name)), name
    for name in ("leaf_sum", "leaf_min", "max_prio", "filled"):
        assert torch.equal(getattr(eng_a.replay, name), getattr(eng_b.replay, name)), name


def test_train_cli_eval_modes(cuda, tmp_path, capsys):
    """train.py with each --eval-mode exits 0 and prints evaluator/ tags; step and rollout print
    identical evaluator numbers for the same seed."""
    from apex_amd import train

    common = ["--n-envs", "64", "--replay_buffer_size", "16384", "--threshold_size", "2048", "--bps_interval", "10",
              "--save_interval", "0", "--target_update_interval", "15", "--no-tb", "--max-step", "20",
              "--eval-interval", "5", "--eval-steps", "6"]
    tags = {}
    for mode in ("step", "rollout", "async"):
        assert train.main(common + ["--save-path", str(tmp_path / f"{mode}.pth"), "--eval-mode", mode]) == 0
        out = capsys.readouterr().out
        rows = []
        for line in out.splitlines():
            if line.startswith("Step: "):
                ev = dict(re.findall(r"(evaluator/\w+)=(\S+)", line))
                if ev:
                    rows.append((line.split()[1], ev))
        assert rows, (mode, out)
        tags[mode] = rows
    assert tags["step"] == tags["rollout"]
    assert all("evaluator/running_return" in ev for _, ev in tags["step"] + tags["async"])
