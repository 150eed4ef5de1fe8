"""GPU tests of the host-env front end: the ingest kernel's warp byte for byte against the fp64
host pipeline (ring wrap, reset, rounding ties), its bookkeeping against a host model, the
shard against the twin ``AtariPreprocess`` and a host ``BatchStorage``, the engine's invariants
and determinism, and the ``train_host`` CLI."""
import functools
import os

import numpy as np
import pytest
import torch

from .host_env_util import near_half, twins, warp_plane, warp_pre

pytestmark = pytest.mark.gpu

FB = 7056


class _Rig:
    """Bare tensors around one ``host_env_ingest`` launch."""

    def __init__(self, dev, E, H, W, F, clip=True, step=0):
        from apex_amd.engine.host_env import Ingest

        self.E, self.F, self.dev = E, F, dev
        self.ingest = Ingest(E, H, W, FB, F, clip, dev)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        self.frames = torch.full((F, FB), 0xAB, dtype=torch.uint8, device=dev)
        self.raw = z(E, 2, H, W, 3, dt=torch.uint8)
        self.reward_in, self.done_in, self.reward, self.done = z(E), z(E), z(E), z(E)
        self.new_frame, self.hist = z(E, dt=torch.int32), z(E, 4, dt=torch.int32)
        self.acc, self.ep_log = z(E, 4), z(E, 4)
        self.step = torch.full((1,), step, dtype=torch.int64, device=dev)

    def launch(self, reset=False):
        self.ingest(self.raw, self.reward_in, self.done_in, self.frames, self.step, reset, self.reward, self.done,
                    self.new_frame, self.hist, self.acc, self.ep_log)
        torch.cuda.synchronize()


def _tie_free_pairs(rng, E, H, W):
    """Seeded random RGB pairs and their fp64 pre-rounding values.  Where one input pixel makes
    one output pixel (84 x 84) the grey value 0.299 R + 0.587 G + 0.114 B is an exact half for
    about one pixel in a thousand; the input pixels under such an output pixel are drawn again
    (decided on the host oracle alone) until no tie is left."""
    pairs = rng.integers(0, 256, (E, 2, H, W, 3), dtype=np.uint8)
    for _ in range(50):
        pre = np.stack([warp_pre(p) for p in pairs])
        ties = np.argwhere(near_half(pre))
        if not len(ties):
            break
        for e, h, w in ties:
            i0, i1 = h * H // 84, -(-(h + 1) * H // 84)
            j0, j1 = w * W // 84, -(-(w + 1) * W // 84)
            pairs[e, :, i0:i1, j0:j1] = rng.integers(0, 256, (2, i1 - i0, j1 - j0, 3), dtype=np.uint8)
    return pairs, pre


@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("H,W", [(210, 160), (250, 160), (84, 84)])
def test_ingest_warp_is_byte_exact(cuda, H, W, reset):
    E, F, step = 3, 16, 4
    rng = np.random.default_rng(1000 * H + W)
    pairs, pre = _tie_free_pairs(rng, E, H, W)
    assert not np.array_equal(pairs[:, 0], pairs[:, 1])
    assert not near_half(pre).any()  # precondition: no rounding tie, every fp64 order gives these bytes
    rig = _Rig(cuda, E, H, W, F, step=step)
    rig.raw.copy_(torch.from_numpy(pairs))
    rig.ep_log.fill_(9.0)
    rig.acc.fill_(9.0)
    rig.launch(reset)
    slots = [((step + (0 if reset else 1)) * E + e) % F for e in range(E)]
    assert slots == ([12, 13, 14] if reset else [15, 0, 1])  # the step's slots wrap inside one launch
    frames = rig.frames.cpu().numpy()
    for e in range(E):
        assert np.array_equal(frames[slots[e]], warp_plane(pairs[e])), e
    assert rig.new_frame.tolist() == slots
    others = [s for s in range(F) if s not in slots]
    assert (frames[others] == 0xAB).all()
    if reset:
        assert rig.hist.tolist() == [[s] * 4 for s in slots]
        assert not rig.ep_log.any() and not rig.acc.any()
    else:
        assert not rig.hist.any()


def test_ingest_ties_differ_by_at_most_one(cuda):
    """Grey inputs put exact halves before the rounding; there the summation order decides.
    Outside the host's near-tie set the planes are byte-equal, inside they differ by <= 1."""
    E, H, W = 3, 210, 160
    rng = np.random.default_rng(7)
    v = rng.integers(0, 256, (E, 2, H, W, 1), dtype=np.uint8)
    pairs = np.ascontiguousarray(np.broadcast_to(v, (E, 2, H, W, 3)))
    pre = np.stack([warp_pre(p) for p in pairs])
    tie = near_half(pre)
    assert tie.mean() < 0.02
    rig = _Rig(cuda, E, H, W, 16, step=0)
    rig.raw.copy_(torch.from_numpy(pairs))
    rig.launch()
    frames = rig.frames.cpu().numpy()
    for e in range(E):
        got = frames[(E + e) % 16].reshape(84, 84).T.astype(np.int64)   # back to [h, w]
        want = warp_plane(pairs[e]).reshape(84, 84).T.astype(np.int64)
        assert np.array_equal(got[~tie[e]], want[~tie[e]])
        assert np.abs(got - want)[tie[e]].max(initial=0) <= 1


@pytest.mark.parametrize("clip", [True, False])
def test_ingest_bookkeeping_matches_host_model(cuda, clip):
    E = 3
    table = [([2.0, -3.0, 0.0], [0, 0, 0]), ([0.5, 0.0, -0.25], [0, 1, 0]), ([0.0, 20.0, 1.0], [1, 0, 0]),
             ([-1.5, 0.0, 0.0], [0, 0, 1]), ([7.0, -0.5, 3.0], [1, 1, 0]), ([0.0, 0.0, 0.0], [0, 0, 1])]
    rig = _Rig(cuda, E, 84, 84, 64, clip=clip)
    rig.launch(reset=True)
    ret, raw_ret, length = np.zeros(E, np.float32), np.zeros(E, np.float32), np.zeros(E, np.float32)
    log = np.zeros((E, 4), np.float32)
    for t, (r_in, d_in) in enumerate(table):
        r_in = np.asarray(r_in, np.float32)
        rig.reward_in.copy_(torch.from_numpy(r_in))
        rig.done_in.copy_(torch.tensor(d_in, dtype=torch.float32))
        rig.step.fill_(t)
        rig.launch()
        r = np.sign(r_in) if clip else r_in                      # the host model
        ret, raw_ret, length = ret + r, raw_ret + r_in, length + 1
        for e in range(E):
            if d_in[e]:
                log[e] = (ret[e], length[e], log[e, 2] + 1, raw_ret[e])
                ret[e] = raw_ret[e] = length[e] = 0
        assert np.array_equal(rig.reward.cpu().numpy(), r.astype(np.float32)), t
        assert rig.done.tolist() == [float(x) for x in d_in]
        acc = rig.acc.cpu().numpy()
        assert np.array_equal(acc[:, 0], ret) and np.array_equal(acc[:, 1], raw_ret) and np.array_equal(acc[:, 2], length)
        assert np.array_equal(rig.ep_log.cpu().numpy(), log), t
        assert rig.new_frame.tolist() == [((t + 1) * E + e) % 64 for e in range(E)]


def test_ingest_launcher_rejects_bad_geometry_before_launching(cuda):
    """The native launcher's own checks (the Python side refuses the same cases earlier): a
    frame smaller than the output, a tap count above the table width, a misaligned pair
    buffer.  Nothing is launched: the ring keeps its fill."""
    from apex_amd import ops

    hip = ops.hip()
    rig = _Rig(cuda, 3, 84, 84, 16)
    good = rig.ingest.taps
    t = rig.ingest._keep[0]
    wide = hip.make_host_env_taps(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), hip.HOST_ENV_TAPS + 1)

    def launch(raw_ptr, rows, params):
        hip.host_env_ingest(raw_ptr, rig.reward_in.data_ptr(), rig.done_in.data_ptr(), rows, good[1],
                            rig.frames.data_ptr(), params, rig.step.data_ptr(), False, rig.reward.data_ptr(),
                            rig.done.data_ptr(), rig.new_frame.data_ptr(), rig.hist.data_ptr(), rig.acc.data_ptr(),
                            rig.ep_log.data_ptr(), torch.cuda.current_stream().cuda_stream)

    ok = rig.ingest.params
    for raw_ptr, rows, params in [(rig.raw.data_ptr(), good[0], hip.HostEnvParams(3, FB, 16, 1, 83, 84)),
                                  (rig.raw.data_ptr(), good[0], hip.HostEnvParams(3, FB, 16, 1, 84, 80)),
                                  (rig.raw.data_ptr(), wide, ok),
                                  (rig.raw.data_ptr() + 1, good[0], ok)]:
        with pytest.raises(ValueError):
            launch(raw_ptr, rows, params)
    torch.cuda.synchronize()
    assert (rig.frames == 0xAB).all()


# ---------------------------------------------------------------------------- shard
@functools.lru_cache(maxsize=None)
def _shard_run(mode):
    """40 teacher-forced steps of a HostEnvShard beside the twin host pipeline and one host
    BatchStorage per env; everything the shard tests compare, recorded once per n-step mode."""
    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.host_env import HostEnvShard
    from apex_amd.replay.nstep import BatchStorage

    dev = torch.device("cuda:0")
    E, A, n, T, C = 3, 18, 3, 40, 256
    raw, ref = twins("Seaquest", E, seed=21, life_every=37)   # episodes of ~6 agent steps
    rp = HBMReplay(C, n_envs=E, n_step=n, device=dev)
    shard = HostEnvShard(rp, E, A, raw.raw_shape, n_step=n, gamma=0.9, seed=3, mode=mode)
    shard.reset(raw)
    obs = ref.reset()
    oracles = [BatchStorage(n, 0.9, mode=mode) for _ in range(E)]
    g = torch.Generator(device="cpu").manual_seed(0)
    rng = np.random.default_rng(2)
    rec = {"obs_ok": [], "reward": [], "done": [], "emitted": [[] for _ in range(E)], "plane": {}, "n_done": 0}
    rec["obs_ok"].append(np.array_equal(shard.observe().cpu().numpy(), obs))
    for t in range(T):
        hist = shard.st["hist"].cpu().numpy().copy()
        for e in range(E):
            for c in range(4):
                rec["plane"][int(hist[e, c])] = obs[e][c].copy()   # what the twin shows at this frame id
        q = torch.randn(E, A, generator=g)
        acts = rng.integers(0, A, E).astype(np.int32)
        shard.q.copy_(q)
        shard.actions.copy_(torch.from_numpy(acts))                # teacher forcing
        shard.step_host(raw)
        torch.cuda.synchronize()
        obs, r, d, _ = ref.step(acts)
        for e in range(E):
            if d[e]:
                rec["n_done"] += 1
                obs[e] = ref.reset_one(e)
        rec["obs_ok"].append(np.array_equal(shard.observe().cpu().numpy(), obs))
        rec["reward"].append((shard.reward.cpu().numpy().copy(), r.copy()))
        rec["done"].append((shard.done.cpu().numpy().copy(), d.copy()))
        slot, prio = shard.slot.cpu().numpy(), shard.prio.cpu().numpy()
        for e in range(E):
            oracles[e].add(tuple(hist[e]), float(r[e]), int(acts[e]), bool(d[e]), q[e].numpy())
            if prio[e] > 0:
                rec["emitted"][e].append((t, int(slot[e]), float(prio[e])))
    rec["oracles"] = oracles
    rec["tables"] = {k: getattr(rp, k).cpu().numpy() for k in ("s_ids", "s2_ids", "action", "reward", "done")}
    rec["frames"] = rp.frames.cpu().numpy()
    rec["ep_log"] = shard.ep_log.cpu().numpy()
    return rec


def test_shard_matches_the_host_pipeline(cuda):
    rec = _shard_run("reference")
    assert rec["n_done"] >= 1
    assert all(rec["obs_ok"]), [i for i, ok in enumerate(rec["obs_ok"]) if not ok]
    for (r_dev, r_host), (d_dev, d_host) in zip(rec["reward"], rec["done"]):
        assert np.array_equal(r_dev, r_host.astype(np.float32))    # the twin clips: sign_reward
        assert np.array_equal(d_dev > 0.5, d_host)
    assert rec["ep_log"][:, 2].sum() == rec["n_done"]


@pytest.mark.parametrize("mode", ["reference", "textbook"])
def test_shard_replay_rows_match_batchstorage(cuda, mode):
    rec = _shard_run(mode)
    tb, frames, plane = rec["tables"], rec["frames"], rec["plane"]
    n_rows = 0
    for e, o in enumerate(rec["oracles"]):
        prios = o.compute_priorities()
        # textbook mode flushes an ended window one row per step: up to n - 1 rows of the last
        # episode may still wait in the drain queue when the run stops
        pending = len(o) - len(rec["emitted"][e])
        assert 0 <= pending <= (2 if mode == "textbook" else 0), (e, len(rec["emitted"][e]), len(o))
        for k, (t, sl, pr) in enumerate(rec["emitted"][e]):
            assert tuple(tb["s_ids"][sl]) == tuple(o.states[k])
            assert all(np.array_equal(frames[i], plane[int(i)].reshape(-1)) for i in tb["s_ids"][sl])
            if not o.dones[k]:
                assert tuple(tb["s2_ids"][sl]) == tuple(o.next_states[k])
                assert all(np.array_equal(frames[i], plane[int(i)].reshape(-1)) for i in tb["s2_ids"][sl]
                           if int(i) in plane)
            assert tb["action"][sl] == o.actions[k]
            assert tb["reward"][sl] == pytest.approx(o.rewards[k], rel=1e-5, abs=1e-6)
            assert tb["done"][sl] == o.dones[k]
            assert pr == pytest.approx(prios[k], rel=1e-4, abs=1e-5)
            n_rows += 1
    assert n_rows > 60


# ---------------------------------------------------------------------------- engine
def _engine_run(use_graphs, iters=60):
    from apex_amd.engine.host_env import HostEnvConfig, HostEnvEngine
    from apex_amd.engine.learner import LearnerConfig

    raw, _ = twins("Seaquest", 4, seed=5)
    cfg = HostEnvConfig(replay_capacity=4096, threshold_size=64, learner_steps_per_actor_step=2,
                        publish_param_interval=5, target_update_interval=20, use_graphs=use_graphs, seed=7,
                        learner=LearnerConfig(batch_size=32, forward="hip", seed=7))
    eng = HostEnvEngine(cfg, raw, "cuda:0")
    sizes, losses = [], []
    for i in range(iters):
        eng.iteration()
        if i % 10 == 9:
            sizes.append(len(eng.replay))
            if eng.learn_steps:
                losses.append(eng.learner.stats()["loss"])
    torch.cuda.synchronize()
    rp = eng.replay
    return {"sizes": sizes, "losses": losses, "learn_steps": eng.learn_steps,
            "leaves": float(rp.leaf_sum.double().sum()), "root": float(rp.node_sum[-1][0]),
            "flat": eng.learner.flat.clone(), "actor_flat": eng.actor_flat.clone(),
            "tables": [getattr(rp, k).clone() for k in ("s_ids", "s2_ids", "action", "reward", "done", "leaf_sum")],
            "frames": rp.frames.clone(), "stats": eng.stats(), "captured": eng._g_learn is not None}


def test_engine_invariants_and_determinism(cuda):
    a = _engine_run(True)
    assert a["captured"]
    assert a["sizes"] == [4 * 10 * (j + 1) for j in range(6)]      # E rows per iteration
    assert a["losses"] and all(np.isfinite(x) for x in a["losses"])
    # learning starts once 64 rows are held (iteration 17 of 60): warm-up + k per iteration
    assert a["learn_steps"] == 3 + 2 * (60 - 16)
    assert a["root"] == pytest.approx(a["leaves"], rel=1e-9)
    b = _engine_run(True)
    c = _engine_run(False)
    assert not c["captured"]
    for other in (b, c):                                           # graph == graph == eager, bit for bit
        assert other["learn_steps"] == a["learn_steps"]
        assert torch.equal(other["flat"], a["flat"])
        assert torch.equal(other["frames"], a["frames"])
        for x, y in zip(other["tables"], a["tables"]):
            assert torch.equal(x, y)
    assert a["stats"]["replay_size"] == 240 and a["stats"]["actor_steps"] == 60


def test_engine_config_rejects_a_bad_ratio(cuda):
    from apex_amd.engine.host_env import HostEnvConfig, HostEnvEngine

    raw, _ = twins("Pong", 2, seed=1)
    for k in (-1, 1.5):
        with pytest.raises(ValueError):
            HostEnvEngine(HostEnvConfig(replay_capacity=256, learner_steps_per_actor_step=k), raw, "cuda:0")


@pytest.mark.parametrize("use_graphs", [True, False])
def test_engine_torch_forward_acts_learns_and_saves(cuda, tmp_path, use_graphs):
    """The PyTorch-module forward (``forward="torch"``): actions come from the standalone
    eps-greedy kernel; the run learns, and ``save`` writes the reference state_dict."""
    from apex_amd.engine.host_env import HostEnvConfig, HostEnvEngine
    from apex_amd.engine.learner import LearnerConfig
    from apex_amd.models.dqn import DuelingDQN

    raw, _ = twins("Pong", 4, seed=9)
    cfg = HostEnvConfig(replay_capacity=1024, threshold_size=32, learner_steps_per_actor_step=1, use_graphs=use_graphs,
                        publish_param_interval=4, learner=LearnerConfig(batch_size=16, forward="torch"))
    eng = HostEnvEngine(cfg, raw, "cuda:0")
    for _ in range(20):
        eng.iteration()
        a = eng.actor.actions.cpu()
        assert ((a >= 0) & (a < 6)).all()
    st = eng.stats()
    assert st["learn_steps"] == 3 + (20 - 8) and np.isfinite(st["loss"]) and st["replay_size"] == 80
    assert (eng._g_learn is not None) == use_graphs
    path = eng.save(str(tmp_path / "m.pth"))
    m = DuelingDQN.from_shapes((4, 84, 84), 6)
    m.load_state_dict(torch.load(path, map_location="cpu", weights_only=True), strict=True)
    assert all(torch.equal(v.cpu(), eng.state_dict()[k].cpu()) for k, v in m.state_dict().items())


# ---------------------------------------------------------------------------- CLI
def test_train_host_cli_saves_and_resumes(cuda, tmp_path, capsys):
    import json

    from apex_amd import train_host
    from apex_amd.models.dqn import DuelingDQN
    from apex_amd.utils.checkpoint import sidecar_path

    ck = str(tmp_path / "model.pth")
    common = ["--env", "SeaquestNoFrameskip-v4", "--envs", "4", "--replay_buffer_size", "4096", "--threshold_size",
              "40", "--batch_size", "32", "--bps_interval", "5", "--save_interval", "10", "--learner-steps", "1",
              "--save-path", ck, "--log-dir", str(tmp_path / "runs")]
    assert train_host.main(common + ["--max-step", "20"]) == 0
    assert os.path.exists(ck) and os.path.exists(sidecar_path(ck))
    side = torch.load(sidecar_path(ck), map_location="cpu", weights_only=True)
    n1 = side["counters"]["learn_steps"]
    assert 20 <= n1 <= 22 and int(side["step_counter"].item()) == n1
    m = DuelingDQN.from_shapes((4, 84, 84), 18)
    m.load_state_dict(torch.load(ck, map_location="cpu", weights_only=True), strict=True)
    with open(tmp_path / "runs" / "scalars.jsonl") as f:
        tags = {json.loads(line)["tag"] for line in f if line.strip()}
    assert {"learner/loss", "learner/grad_norm", "learner/BPS", "actor/frames_per_sec", "replay/size"} <= tags
    capsys.readouterr()
    assert train_host.main(common + ["--max-step", str(n1 + 10), "--resume", ck, "--no-tb"]) == 0
    assert f"training from step {n1}" in capsys.readouterr().out
    side2 = torch.load(sidecar_path(ck), map_location="cpu", weights_only=True)
    n2 = side2["counters"]["learn_steps"]
    assert n1 + 10 <= n2 <= n1 + 12 and int(side2["step_counter"].item()) == n2
    assert torch.isfinite(side2["opt_s2"]).all()
