"""The host-env vector engine (``engine/vector_host.py``, ``vec_host_tail``) on the GPU.

Small shapes throughout: the tail runs at 1 .. 2400 (env, component) elements (one partial
workgroup up to ten), the engines at E = 5 .. 8 envs, batch 16, capacity <= 4096."""
import json

import numpy as np
import pytest
import torch

from apex_amd.envs.host_vector import HostVectorEnv, staging_views
from apex_amd.models.dqn import DuelingDQN

from . import vector_host_fixtures as fx

pytestmark = pytest.mark.gpu

NAN = float("nan")
I_GUARD = -12345


def _bits(t):
    """A tensor's bytes as int32 (NaN guards compare equal to themselves)."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------ 1. the tail against the numpy model
class _TailRig:
    """Every output buffer of ``vec_host_tail`` between two guard rows, on the device, beside the
    numpy model's state; the interiors start from the same random / sentinel values."""

    def __init__(self, hip, dev, E, obs, F, step, rng):
        self.hip, self.E, self.obs, self.F = hip, E, obs, F
        st = fx.tail_state(E, obs, F, step)
        st["ring"][:] = -7.5                                            # an unwritten row must keep this
        st["reward"][:] = 55.0
        st["done"][:] = 66.0
        st["new_frame"][:] = 777
        st["hist"][:] = rng.randint(0, F, size=(E, 4))
        st["ep_log"][:] = rng.uniform(-3, 3, size=(E, 4)).astype(np.float32)
        st["ep_log"][:, 2] = rng.randint(0, 5, size=E)
        st["ep_ret"][:] = rng.uniform(-9, 9, size=E).astype(np.float32)
        st["ep_len"][:] = rng.randint(0, 40, size=E)
        self.model = st
        self.dev = {}
        for k in ("ring", "reward", "done", "new_frame", "hist", "ep_log", "ep_ret", "ep_len"):
            a = st[k]
            g = np.full((1,) + a.shape[1:], I_GUARD if a.dtype == np.int32 else NAN, dtype=a.dtype)
            self.dev[k] = torch.from_numpy(np.concatenate([g, a, g])).to(dev)
        self.step = torch.tensor([step], dtype=torch.int64, device=dev)
        self.stage = torch.zeros(E * (2 * obs + 3), dtype=torch.float32, device=dev)
        ptr = {k: v[1:].data_ptr() for k, v in self.dev.items()}       # (the interior: past the first guard row)
        self.args = dict(E=E, obs=obs, F=F, stage=self.stage.data_ptr(), step=self.step.data_ptr(), **ptr)
        self.tail = hip.make_vec_host_tail(self.args)

    def run(self, block, reset):
        self.stage.copy_(torch.from_numpy(block))
        self.hip.vec_host_tail(self.tail, reset, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        fx.tail_model(self.model, staging_views(block, self.E, self.obs), reset=reset)

    def bump(self):
        self.step += 1
        self.model["step"] += 1

    def check(self, tag):
        for k, d in self.dev.items():
            a = self.model[k]
            g = np.full((1,) + a.shape[1:], I_GUARD if a.dtype == np.int32 else NAN, dtype=a.dtype)
            want = np.concatenate([g, a, g])
            assert np.array_equal(_bits(d), want.view(np.int32) if want.dtype == np.float32 else want), (tag, k)


def _block(rng, E, obs, t):
    """A staged step: random observations and rewards, terminals (done = ended = non-zero), cap
    resets (ended alone) and running envs mixed."""
    b = np.zeros(E * (2 * obs + 3), np.float32)
    v = staging_views(b, E, obs)
    v["next_obs"][:] = rng.uniform(-1, 1, size=(E, obs))
    v["reset_obs"][:] = rng.uniform(-1, 1, size=(E, obs))
    v["reward"][:] = rng.uniform(-2, 2, size=E)
    kind = (np.arange(E) + t) % 4           # 0 runs on, 1 terminal, 2 cap reset, 3 runs on
    v["done"][:] = np.where(kind == 1, 1.0 + (np.arange(E) % 2) * 2.0, 0.0)   # (1.0 or 3.0: stored as 1.f)
    v["ended"][:] = np.where((kind == 1) | (kind == 2), 1.0, 0.0)
    return b


@pytest.mark.parametrize("step0", [0, 2 ** 31 + 5])
@pytest.mark.parametrize("E,obs", [(1, 1), (5, 2), (9, 6), (67, 8), (300, 4)])
def test_tail_matches_numpy_model_bit_for_bit(cuda, E, obs, step0):
    """Both forms, F = 2E + 3 (the slots wrap, no ring row is aligned), the step counter at 0 and
    where (step + 1) E is past 2^31: ring, reward, done, new_frame, hist, ep_log and the running
    pair equal the model's bit for bit, guard rows and unwritten rows included."""
    from apex_amd import ops

    rng = np.random.RandomState(1000 * E + obs)
    rig = _TailRig(ops.hip(), cuda, E, obs, 2 * E + 3, step0, rng)
    assert (step0 + 1) * E > 2 ** 31 or step0 == 0
    rig.run(_block(rng, E, obs, 0), reset=True)
    rig.check("reset")
    assert (rig.model["hist"] == rig.model["new_frame"][:, None]).all() and not rig.model["ep_log"].any()
    hist0 = rig.model["hist"].copy()
    caps = 0
    for t in range(4):   # (every env meets a terminal, a cap reset and two running steps)
        b = _block(rng, E, obs, t)
        v = staging_views(b, E, obs)
        caps += int(((v["ended"] != 0) & (v["done"] == 0)).sum())
        rig.run(b, reset=False)
        rig.check(("step", t))
        rig.bump()
    assert caps == E and np.array_equal(rig.model["hist"], hist0)     # the step form leaves hist alone
    assert (rig.model["ep_log"][:, 2] == 2).all() and set(np.unique(rig.model["done"])) <= {0.0, 1.0}
    # a second reset, at the moved counter
    rig.run(_block(rng, E, obs, 9), reset=True)
    rig.check("reset 2")


# ------------------------------------------------------------------ 2. launcher limits
def test_launcher_limits(cuda):
    """E = 0, E = 4097, obs = 9, F < 2E and a null pointer each raise, and none of them launches:
    no buffer changes."""
    from apex_amd import ops

    h = ops.hip()
    rig = _TailRig(h, cuda, 6, 4, 15, 3, np.random.RandomState(0))
    rig.stage.copy_(torch.from_numpy(_block(np.random.RandomState(1), 6, 4, 0)))
    s = torch.cuda.current_stream().cuda_stream
    bad = [dict(E=0), dict(E=4097, F=3 * 4097), dict(obs=9), dict(obs=0), dict(F=11)]
    bad += [{k: 0} for k in ("stage", "ring", "step", "reward", "done", "new_frame", "hist", "ep_log", "ep_ret",
                             "ep_len")]
    for change in bad:
        for reset in (False, True):
            with pytest.raises(ValueError, match="vec_host_tail"):
                h.vec_host_tail(h.make_vec_host_tail(dict(rig.args, **change)), reset, s)
    torch.cuda.synchronize()
    rig.check("nothing ran")
    h.vec_host_tail(h.make_vec_host_tail(dict(rig.args, F=12)), False, s)   # F = 2E is allowed
    torch.cuda.synchronize()


# ------------------------------------------------------------------ engines
def _cfg(env_id, E, **kw):
    from apex_amd.engine.vector import VectorEngineConfig

    base = dict(env_id=env_id, n_envs=E, batch_size=16, replay_capacity=4096, lr=1e-3, seed=3,
                publish_param_interval=8, target_update_interval=100)
    base.update(kw)
    return VectorEngineConfig(**base)


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


def _same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------ 3. tape equivalence
EAGER, GRAPHED, WARM = 150, 145, 3   # 298 SGD steps: past the target syncs at 100 and 200, short of 300's


@pytest.mark.parametrize("env_id", ["CartPole-v0", "MountainCar-v0"])
def test_tape_equivalence(cuda, env_id):
    """A tape env that plays back what the device envs of ``VectorApexEngine`` did (and checks
    that it is handed the same actions) leaves ``VectorHostEngine(host_overlap=False,
    learner_steps=1)`` with the same transition tables, frame ring, tree, parameters, optimizer
    state, episode log and counters, bit for bit: after the eager steps and after the captured
    ones."""
    from apex_amd.engine.vector import VectorApexEngine
    from apex_amd.engine.vector_host import VectorHostEngine

    E = 8
    ref = VectorApexEngine(_cfg(env_id, E), cuda)
    sh = ref.shard
    torch.cuda.synchronize()
    first = sh.ring[sh.new_frame.long()].cpu().numpy().copy()
    steps = []
    step = ref.actor_step

    def recorded():
        step()
        torch.cuda.synchronize()
        steps.append(dict(obs=sh.ring[sh.new_frame.long()].cpu().numpy().copy(), reward=sh.reward.cpu().numpy().copy(),
                          done=sh.done.cpu().numpy().copy(), actions=sh.actions.cpu().numpy().copy()))

    ref.actor_step = recorded
    ref.fill()
    n_fill = len(steps)
    for _ in range(EAGER):
        ref.train_step()
    want_eager = _state(ref)
    ref.capture(warmup_iters=WARM)
    for _ in range(GRAPHED):
        ref.train_step()
    want = _state(ref)
    assert len(steps) == n_fill + EAGER + WARM + GRAPHED and ref.learn_steps == EAGER + WARM + GRAPHED
    n_done = int(sum(s["done"].sum() for s in steps))
    assert n_done >= E                                              # (a condition on the input: episodes ended)

    vec = fx.TapeVectorEnv(first, steps, sh.A, sh.max_episode_steps)
    eng = VectorHostEngine(_cfg(env_id, E), vec, cuda, learner_steps=1, host_overlap=False)
    eng.fill()
    assert vec.t == n_fill
    for _ in range(EAGER):
        eng.train_step()
    _same(_state(eng), want_eager)
    eng.capture(warmup_iters=WARM)
    assert eng._g_learn is not None
    for _ in range(GRAPHED):
        eng.train_step()
    got = _state(eng)
    _same(got, want)
    assert vec.t == len(steps) and eng.env_steps == E * len(steps) and eng.learn_steps == ref.learn_steps
    assert float(got["ep_log"][:, 2].sum()) == n_done
    assert not torch.equal(got["flat"], want_eager["flat"]) and not torch.equal(got["tflat"], got["flat"])
    eng.close()
    assert vec.closed
    eng.close()   # idempotent


# ------------------------------------------------------------------ 4. overlap is race-free
def test_overlap_is_race_free(cuda):
    """host_overlap=True as is == the same run with a device synchronize after every enqueue:
    the one-stream order alone protects the staging block, the action buffer and the published
    weights.  200 iterations of 3 learner steps, the second half through the captured graph."""
    from apex_amd.engine.vector_host import VectorHostEngine

    class Synced(VectorHostEngine):
        syncs = 0

        def _enqueued(self):
            torch.cuda.synchronize()
            self.syncs += 1

    out, seen = [], []
    for cls in (VectorHostEngine, Synced):
        vec = HostVectorEnv([fx.acrobot_like] * 5, seed=21)
        eng = cls(_cfg("scripted-6x3", 5, publish_param_interval=4, target_update_interval=50), vec, cuda,
                  learner_steps=3)
        assert eng.host_overlap and eng.K == 3 and (eng.obs_dim, eng.A) == (6, 3)
        eng.fill()
        for _ in range(100):
            eng.train_step()
        eng.capture(warmup_iters=0)
        for _ in range(100):
            eng.train_step()
        out.append(_state(eng))
        seen.append([list(e.seen) for e in vec.envs])
        assert eng.learn_steps == 600
        if cls is Synced:
            assert eng.syncs > 200 * (2 + 3 + 4)   # acting 2 + 4 enqueues, one per learner step, the cadences
        eng.close()
    _same(out[0], out[1])
    assert seen[0] == seen[1] and len(seen[0][0]) > 200
    assert float(out[0]["ep_log"][:, 2].sum()) >= 5 * (200 // 13)    # episodes ended all along


# ------------------------------------------------------------------ 5. cap reset
def test_cap_reset_keeps_done_zero(cuda):
    """Under a cap of 7 (the scripted env ends itself only at 13): the stored done stays 0, the
    next action is chosen from the reset observation (hist's newest entry is its ring row), and
    ep_log counts the episode with the length of the cap."""
    from apex_amd.engine.vector_host import VectorHostEngine

    E, cap, n_steps = 4, 7, 30
    vec = HostVectorEnv([fx.acrobot_like] * E, seed=2, max_episode_length=cap)
    eng = VectorHostEngine(_cfg("scripted-6x3", E), vec, cuda, host_overlap=False)
    sh = eng.shard
    torch.cuda.synchronize()
    assert np.array_equal(sh.observe().cpu().numpy(), vec.reset_obs)
    ret = np.zeros(E, np.float32)
    for t in range(1, n_steps + 1):
        eng.actor_step()
        torch.cuda.synchronize()
        ret += vec.reward
        hist, nf = sh.st["hist"].cpu().numpy(), sh.new_frame.cpu().numpy()
        assert not sh.done.any() and not vec.done.any()
        assert np.array_equal(hist[:, 3], nf) and np.array_equal(sh.observe().cpu().numpy(), vec.reset_obs)
        log = sh.ep_log.cpu().numpy()
        if t % cap == 0:    # every env was reset at the cap: a fresh draw, not the step's own observation
            assert vec.ended.all() and (np.abs(vec.reset_obs) <= 0.1).all() and (np.abs(vec.next_obs) > 0.1).any()
            assert np.array_equal(log[:, 0], ret) and (log[:, 1] == cap).all() and (log[:, 2] == t // cap).all()
            ret[:] = 0
        else:
            assert not vec.ended.any() and np.array_equal(vec.reset_obs, vec.next_obs)
            assert (log[:, 2] == t // cap).all()
    filled = int(eng.replay.filled)
    assert filled == E * n_steps and not eng.replay.done[:filled].any()
    assert int(sh.step_counter) == n_steps and eng.env_steps == E * n_steps
    # the device-env evaluators are refused, and say where to go
    from apex_amd.engine.vector import VectorEvaluator

    with pytest.raises(RuntimeError, match="evaluate"):
        eng.rollout_evaluate(2)
    with pytest.raises(TypeError, match="evaluate"):
        VectorEvaluator(eng, 2)
    eng.close()


# ------------------------------------------------------------------ 6. the widest shapes
def test_widest_shapes_train(cuda):
    """obs 8 / 7 actions (kVecMaxObs, kVecMaxA): 50 iterations with a finite loss, every action
    reaches the envs, the greedy evaluator plays the same env."""
    from apex_amd.engine.vector_host import VectorHostEngine

    vec = HostVectorEnv([fx.widest] * 6, seed=8)
    eng = VectorHostEngine(_cfg("scripted-8x7", 6, eps_base=0.8, eps_alpha=1.0), vec, cuda, learner_steps=2,
                           eval_env=fx.widest)
    assert (eng.obs_dim, eng.A, eng.limit) == (8, 7, None)
    eng.fill()
    losses = []
    for _ in range(50):
        eng.train_step()
        losses.append(float(eng.learner.loss.item()))
    assert eng.learn_steps == 100 and np.isfinite(losses).all() and max(losses) > 0
    assert all(np.isfinite(v) for v in eng.learner.stats().values())
    seen = {a for e in vec.envs for a in e.seen}
    assert seen == set(range(7))
    ret = eng.evaluate(3, seed=1)
    assert len(ret) == 3 and np.isfinite(ret).all() and ret == eng.evaluate(3, seed=1)
    assert all(-0.125 * 13 <= r <= 0.875 * 13 for r in ret)
    eng.close()


# ------------------------------------------------------------------ 7. CLI
def test_cli_trains_and_checkpoints(cuda, tmp_path, capsys):
    from apex_amd import train_vector

    log = tmp_path / "log.jsonl"
    assert train_vector.main(["--host-envs", "--env", "CartPole-v0", "--envs", "4", "--learner-steps", "2",
                              "--max-step", "60", "--save-interval", "30", "--eval-interval", "30",
                              "--capacity", "4096", "--save-dir", str(tmp_path), "--json-log", str(log)]) == 0
    for t in (30, 60):
        m = DuelingDQN.from_shapes((4,), 2)
        sd = torch.load(str(tmp_path / f"model{t}.pth"), map_location="cpu", weights_only=True)
        assert list(sd) == list(m.state_dict())
        m.load_state_dict(sd)
        assert all(torch.isfinite(p).all() for p in m.parameters())
    recs = [json.loads(x) for x in log.read_text().splitlines()]
    assert [r["step"] for r in recs] == [30, 60]
    printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert printed == recs
    for r in recs:
        assert 1.0 <= r["greedy_mean_return"] <= 200.0 and r["sgd_steps_per_s"] > 0 and r["env_steps_per_s"] > 0
        assert set(r) == {"step", "loss", "grad_norm", "grad_norm_l2", "lr", "sgd_steps_per_s", "env_steps_per_s",
                          "episodes", "actor_mean_return", "greedy_mean_return"}
