"""GPU tests of the host-env evaluator: ``host_eval_act`` against the forward it replaces and the
fp64 module, its stack advance / counter / guard rows / launcher checks, the fused and stepwise
evaluators free-running against each other and the fp64 greedy run on the ``AtariPreprocess`` twin,
the episode cap, snapshot isolation of ``refresh``, training left bit-identical by an evaluator
beside it, the asynchronous driver's progress and shutdown, and the ``train_host`` flags."""
import re
import time

import numpy as np
import pytest
import torch

from . import actor_oracle as ao
from . import atari_rollout_fixtures as rf
from . import host_eval_fixtures as fx
from .host_env_util import twins, warp_plane

pytestmark = pytest.mark.gpu

FB = 7056
STATE = ("frames", "hist", "new_frame", "reward", "done", "acc", "ep_log", "actions", "counter")


# ---------------------------------------------------------------------------- the kernel alone
class _Rig:
    """Bare tensors around one ``host_eval_act`` launch: a crafted ring of random bytes, hist rows
    of 4 distinct slots (slots 0 and F - 1 among them), one sentinel guard row past N in q / actions."""

    def __init__(self, dev, N, A, ms=0, seed=0):
        from apex_amd import ops
        from apex_amd.models.fused_f32 import F32DuelingNet

        self.hip, self.dev, self.N, self.A, self.F = ops.hip(), dev, N, A, 8 * N
        g = torch.Generator().manual_seed(100 * N + A)
        self.model = rf.make_model(A, ms).to(dev)
        self.net = F32DuelingNet(self.model)
        self.frames = torch.randint(0, 256, (self.F, FB), dtype=torch.uint8, generator=g).to(dev)
        hist = torch.stack([torch.randperm(self.F, generator=g)[:4] for _ in range(N)]).to(torch.int32)
        hist[0, 0], hist[N - 1, 3] = 0, self.F - 1
        if N == 1:
            hist[0] = torch.tensor([0, 3, 5, self.F - 1])
        for e in range(N):
            assert len(set(hist[e].tolist())) == 4
        self.hist = hist.to(dev)
        self.new_frame = torch.randint(0, self.F, (N,), generator=g).to(torch.int32).to(dev)
        self.done = (torch.arange(N) % 2 == 1).float().to(dev)        # a mixed done pattern
        self.eps = torch.zeros(N, device=dev)
        self.counter = torch.full((1,), 41, dtype=torch.int64, device=dev)
        self.q = torch.full((N + 1, A), -77.0, device=dev)
        self.actions = torch.full((N + 1,), -7, dtype=torch.int32, device=dev)
        self.act_seed = seed ^ rf.ACT_XOR

    def args(self, **over):
        m, f, net = self.model, self.model.features, self.net
        t = {"w1": f[0].weight, "b1": f[0].bias, "w2p": net.w2p, "b2": f[2].bias, "w3p": net.w3p, "b3": f[4].bias,
             "wfc1p": net.wfc1p, "ba1": m.advantage[0].bias, "bv1": m.value[0].bias, "wa2": m.advantage[2].weight,
             "ba2": m.advantage[2].bias, "wv2": m.value[2].weight, "bv2": m.value[2].bias, "eps": self.eps,
             "frames": self.frames, "hist": self.hist, "new_frame": self.new_frame, "done": self.done,
             "counter": self.counter, "q": self.q, "actions": self.actions}
        d = {k: v.data_ptr() for k, v in t.items()}
        d.update(N=self.N, A=self.A, F=self.F, frame_bytes=FB, act_seed=self.act_seed, advance=0, step=0)
        d.update(over)
        return d

    def launch(self, **over):
        self.hip.host_eval_act(self.hip.make_host_eval_act(self.args(**over)), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()

    def obs(self):
        return self.frames[self.hist.long()].view(self.N, 4, 84, 84).contiguous()


@pytest.mark.parametrize("A", [18, 6, 9])
@pytest.mark.parametrize("N", [1, 3, 8])
def test_kernel_q_is_the_fp64_q_and_state_advances(cuda, N, A):
    """q within the project's Q bound of the fp64 module, its scaled error at most 2x the larger of
    the stepwise F32DuelingNet's and torch fp32's on the same observations; advance off leaves hist
    and counter untouched, advance on equals frame_hist_step and stores counter = step; the guard
    rows past N keep their sentinels.  (A = 9 is a count the GPU game's kernels refuse.)"""
    from apex_amd.models.fused_f32 import F32Workspace

    rig = _Rig(cuda, N, A)
    hist0 = rig.hist.clone()
    x = rig.obs()
    rig.launch(advance=0, step=5)
    assert torch.equal(rig.hist, hist0) and int(rig.counter.item()) == 41
    with torch.no_grad():
        q64 = rf.make_model(A, 0).double()(x.cpu().double())
        q_torch = rig.model(x.float()).cpu()
    q_step = rig.net(x, F32Workspace(N, A, cuda)).clone().cpu()
    q_k = rig.q[:N].cpu()
    scale = float(q64.abs().max())
    err = {n: float((v.double() - q64).abs().max()) / scale
           for n, v in (("fused", q_k), ("stepwise", q_step), ("torch", q_torch))}
    print(f"N={N} A={A}: scaled Q error vs fp64: " + ", ".join(f"{n} {e:.3e}" for n, e in err.items()))
    torch.testing.assert_close(q_k.double(), q64, rtol=rf.Q_RTOL, atol=rf.Q_ATOL * scale)
    assert err["fused"] <= 2.0 * max(err["stepwise"], err["torch"]), err
    want = ao.select_actions_ref(q_k.numpy(), np.zeros(N, np.float32), rig.act_seed, 5)
    assert np.array_equal(rig.actions[:N].cpu().numpy(), want)
    assert (rig.q[N] == -77.0).all() and int(rig.actions[N]) == -7
    # advance on: frame_hist_step's result, counter = step, Q of the advanced stacks
    ref_hist, ref_counter = hist0.clone(), torch.zeros(1, dtype=torch.int64, device=cuda)
    rig.hip.frame_hist_step(ref_hist.data_ptr(), rig.new_frame.data_ptr(), rig.done.data_ptr(), N,
                            ref_counter.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rig.launch(advance=1, step=6)
    assert torch.equal(rig.hist, ref_hist) and not torch.equal(rig.hist, hist0)
    assert int(rig.counter.item()) == 6
    with torch.no_grad():
        q64b = rf.make_model(A, 0).double()(rig.obs().cpu().double())
    torch.testing.assert_close(rig.q[:N].cpu().double(), q64b, rtol=rf.Q_RTOL, atol=rf.Q_ATOL * float(q64b.abs().max()))
    assert (rig.q[N] == -77.0).all() and int(rig.actions[N]) == -7


def test_kernel_epsilon_one_draws_select_actions_numbers(cuda):
    N, A = 3, 18
    rig = _Rig(cuda, N, A, seed=9)
    rig.eps.fill_(1.0)
    seen = set()
    for step in range(8):
        rig.launch(advance=0, step=step)
        want = ao.select_actions_ref(rig.q[:N].cpu().numpy(), np.ones(N, np.float32), rig.act_seed, step)
        got = rig.actions[:N].cpu().numpy()
        assert np.array_equal(got, want), step
        seen |= set(got.tolist())
    assert len(seen) >= 4   # (uniform draws over 18 actions, 24 of them)


def test_launcher_validation(cuda):
    rig = _Rig(cuda, 3, 6)
    rig.q.view(torch.uint8).fill_(0xAB)
    rig.actions.view(torch.uint8).fill_(0xAB)
    q0, a0, h0 = rig.q.clone(), rig.actions.clone(), rig.hist.clone()
    bad = [dict(N=0), dict(N=65, F=8 * 65), dict(A=0), dict(A=19), dict(F=8 * 3 + 1), dict(F=16), dict(frame_bytes=7000),
           dict(frames=rig.frames.data_ptr() + 1), dict(w2p=rig.net.w2p.data_ptr() + 4),
           dict(wfc1p=rig.net.wfc1p.data_ptr() + 8)]
    pointers = ("w1", "b1", "w2p", "b2", "w3p", "b3", "wfc1p", "ba1", "bv1", "wa2", "ba2", "wv2", "bv2", "eps", "frames",
                "hist", "new_frame", "done", "counter", "q", "actions")
    bad += [{k: 0} for k in pointers]
    s = torch.cuda.current_stream().cuda_stream
    for over in bad:
        with pytest.raises(ValueError):
            rig.hip.host_eval_act(rig.hip.make_host_eval_act(rig.args(advance=1, step=3, **over)), s)
    torch.cuda.synchronize()
    assert torch.equal(rig.q.view(torch.uint8), q0.view(torch.uint8)) and torch.equal(rig.actions, a0)
    assert torch.equal(rig.hist, h0) and int(rig.counter.item()) == 41


# ---------------------------------------------------------------------------- free-running
def _need_gap(case, steps=fx.STEPS, cap=0):
    ok, g = fx.gap_ok(case, steps, cap)   # recomputed on the CPU; a free-running comparison needs it
    assert ok, f"fixture {case}: top-2 Q gap {g:.3e} < {fx.GAP} x max|Q| -- the comparison is not meaningful"


def _evaluator(dev, case, kernel, cap=0, model=None, **kw):
    from apex_amd.engine.host_eval import HostEvaluator

    raw, _ = fx.make_twins(case, cap=cap)
    return HostEvaluator(model if model is not None else fx.model(case), raw, dev, kernel=kernel, seed=fx.SEED, **kw)


def _same(a, b, what):
    torch.cuda.synchronize()
    for n in STATE:
        x, y = getattr(a, n), getattr(b, n)
        assert torch.equal(x, y), (what, n, int((x != y).sum()))


@pytest.mark.parametrize("case", sorted(fx.CASES))
def test_free_running_fused_equals_stepwise_equals_fp64_twin(cuda, case):
    """N = 3, 24 steps: after every act both kernels hold bit-equal state; the ring planes are the
    host warp of the pairs; actions and the host-side episode list equal the fp64 greedy run on the
    AtariPreprocess twin; the device ep_log agrees with the host accounting."""
    _need_gap(case)
    want = fx.host_greedy(case)
    ev_f, ev_s = _evaluator(cuda, case, "fused"), _evaluator(cuda, case, "step")
    for k in range(fx.STEPS):
        pairs = None
        for ev in (ev_f, ev_s):
            ev.step_begin()
            ev.acted.synchronize()
            if ev is ev_f:
                pairs = ev.raw_np.copy()          # what this step's ingest warped
        _same(ev_f, ev_s, k)
        assert int(ev_f.counter.item()) == k
        frames, slots = ev_f.frames.cpu().numpy(), ev_f.new_frame.cpu().numpy()
        for e in range(fx.N):
            assert slots[e] == (k * fx.N + e) % ev_f.F
            assert np.array_equal(frames[slots[e]], warp_plane(pairs[e])), (k, e)
        assert np.array_equal(ev_f.actions_host.numpy(), want["actions"][k]), k
        for ev in (ev_f, ev_s):
            ev.step_end()
    for ev in (ev_f, ev_s):
        assert [e[:3] for e in ev.poll()] == list(want["episodes"])
        assert ev.ledger.steps == fx.STEPS and ev.ledger.episodes == len(want["episodes"])
    # the device log has ingested the host steps 0 .. STEPS - 2: last raw return, length, count per env
    log = ev_f.ep_log.cpu().numpy()
    for e in range(fx.N):
        ret = length = count = 0
        last = (0.0, 0.0)
        for k in range(fx.STEPS - 1):
            ret += want["rewards"][k, e]
            length += 1
            if want["dones"][k, e]:
                last, ret, length, count = (ret, length), 0, 0, count + 1
        assert (log[e, 3], log[e, 1], log[e, 2]) == (np.float32(last[0]), last[1], count), e


def test_cap_ends_episodes_at_five_steps(cuda):
    case, cap = "pong", 5
    _need_gap(case, fx.STEPS, cap)
    want = fx.host_greedy(case, fx.STEPS, cap)
    ev = _evaluator(cuda, case, "fused", cap=cap)
    ev.run(fx.STEPS)
    eps = ev.poll()
    assert [e[:3] for e in eps] == list(want["episodes"])
    assert all(e[1] <= cap for e in eps)
    n_capped = sum(e[2] for e in want["episodes"])
    assert ev.ledger.capped == n_capped and 3 <= n_capped < len(eps)   # capped and natural ends both occur


def test_refresh_is_a_snapshot_and_conflates(cuda):
    """refresh(), then the source is zeroed on the training stream: the next 8 steps equal a run
    with the original weights.  A refresh issued while the act that last read its target set is in
    flight returns False and copies nothing (the zeroed source never reaches the evaluator)."""
    from apex_amd.models.fused_f32 import F32DuelingNet

    case = "pong"
    _need_gap(case, 8)
    want = fx.host_greedy(case, 8)
    src, keep = fx.model(case).to(cuda), fx.model(case).to(cuda)
    src_flat, keep_flat = src.flatten_parameters(), keep.flatten_parameters()
    src_net, keep_net = F32DuelingNet(src), F32DuelingNet(keep)
    ev = _evaluator(cuda, case, "fused", model=rf.make_model(6, 5))   # starts from other weights
    assert ev.refresh(src_flat, src_net)             # -> set 1
    src_flat.zero_()
    src_net.arena.zero_()
    busy = torch.randn(4096, 4096, device=cuda)
    torch.cuda.synchronize()
    acts = []
    for k in range(8):
        if k == 3:
            with torch.cuda.stream(ev.stream):       # keep the side stream busy in front of this act
                for _ in range(32):
                    busy @ busy
        ev.step_begin()
        if k == 3:                                   # act 3 (reading set 1) is queued behind that work
            assert not ev.acted.query()
            assert ev.refresh(keep_flat, keep_net) is True    # set 0 has never been read
            assert ev.refresh(src_flat, src_net) is False     # set 1 is being read: refused, nothing copied
            assert ev.weights.conflated == 1
        ev.step_end()
        acts.append(ev.actions_host.numpy().copy())
    assert np.array_equal(np.stack(acts), want["actions"])
    torch.cuda.synchronize()
    assert ev.refresh(keep_flat, keep_net) is True
    ev.close()


# ---------------------------------------------------------------------------- beside training
def _engine_run(mode, iters=60):
    """The engine of test_gpu_host_env.test_engine_invariants_and_determinism (4 envs, 60 iterations,
    batch 32), with no evaluator / the blocking evaluator / the asynchronous driver beside it."""
    from apex_amd.engine.host_env import HostEnvConfig, HostEnvEngine
    from apex_amd.engine.host_eval import HostEnvEvaluation, HostEvaluator, eval_seed
    from apex_amd.engine.learner import LearnerConfig
    from apex_amd.envs.preprocess import PreprocessSpec
    from apex_amd.envs.proc_vector import ProcRawAtariVector

    raw, _ = twins("Seaquest", 4, seed=5)
    cfg = HostEnvConfig(replay_capacity=4096, threshold_size=64, learner_steps_per_actor_step=2,
                        publish_param_interval=5, target_update_interval=20, use_graphs=True, seed=7,
                        learner=LearnerConfig(batch_size=32, forward="hip", seed=7))
    eng = HostEnvEngine(cfg, raw, "cuda:0")
    evaluation, steps, episodes = None, 0, 0
    try:
        if mode == "async":
            pool = ProcRawAtariVector("SeaquestNoFrameskip-v4", 2, PreprocessSpec(), workers=1, seed=eval_seed(7),
                                      factory="tests.proc_vector_fixtures:short", timeout=30.0)
            evaluation = HostEnvEvaluation(HostEvaluator(eng.actor_model, pool, "cuda:0", seed=eval_seed(7)), pool)
        elif mode == "blocking":
            ev_raw, _ = twins("Seaquest", 2, seed=eval_seed(7))
            evaluation = HostEvaluator(eng.actor_model, ev_raw, "cuda:0", seed=eval_seed(7))
        for i in range(iters):
            eng.iteration()
            if evaluation is not None and i % 10 == 9:
                evaluation.refresh(eng.actor_flat, eng.actor_net)
            if mode == "async":
                evaluation.pump(eng.learn_steps)
            elif mode == "blocking":
                evaluation.run(1)
        torch.cuda.synchronize()
        if evaluation is not None:
            core = getattr(evaluation, "ev", evaluation)
            steps, episodes = core.ledger.steps, core.ledger.episodes
        rp = eng.replay
        return {"learn_steps": eng.learn_steps, "flat": eng.learner.flat.clone(), "actor_flat": eng.actor_flat.clone(),
                "tables": [getattr(rp, k).clone() for k in ("s_ids", "s2_ids", "action", "reward", "done", "leaf_sum")],
                "frames": rp.frames.clone(), "captured": eng._g_learn is not None, "eval_steps": steps,
                "eval_episodes": episodes}
    finally:
        if evaluation is not None:
            evaluation.close()
        eng.close()


def test_training_is_bit_identical_with_an_evaluator_beside_it(cuda):
    a, b, c = _engine_run("none"), _engine_run("blocking"), _engine_run("async")
    assert a["captured"] and a["learn_steps"] == 3 + 2 * (60 - 16)
    assert b["eval_steps"] == 60 and c["eval_steps"] >= 1     # both evaluators really ran
    print("evaluator steps beside 60 iterations: blocking", b["eval_steps"], "async", c["eval_steps"])
    for other in (b, c):
        assert other["captured"] and other["learn_steps"] == a["learn_steps"]
        assert torch.equal(other["flat"], a["flat"]) and torch.equal(other["actor_flat"], a["actor_flat"])
        assert torch.equal(other["frames"], a["frames"])
        for x, y in zip(other["tables"], a["tables"]):
            assert torch.equal(x, y)


def test_async_driver_makes_progress_and_shuts_down(cuda):
    from multiprocessing import shared_memory

    from apex_amd.engine.host_eval import HostEnvEvaluation, HostEvaluator
    from apex_amd.envs.preprocess import PreprocessSpec
    from apex_amd.envs.proc_vector import ProcRawAtariVector

    pool = ProcRawAtariVector("SeaquestNoFrameskip-v4", 2, PreprocessSpec(), workers=1, seed=3,
                              factory="tests.proc_vector_fixtures:short", timeout=30.0)
    name, procs = pool.shm_name, pool.processes
    drv = HostEnvEvaluation(HostEvaluator(rf.make_model(18, 0), pool, cuda, seed=3), pool)
    try:
        got, t0 = [], time.monotonic()
        while len(got) < 3:
            assert time.monotonic() - t0 < 60.0, f"{len(got)} episodes after 60 s ({drv.ev.ledger.steps} steps)"
            drv.pump(learn_step=17)
            got += drv.poll()
        assert all(len(e) == 4 and e[1] >= 1 and e[3] == 17 for e in got)
    finally:
        drv.close()
    drv.close()                                              # a second close returns
    assert all(not p.is_alive() for p in procs)
    with pytest.raises(FileNotFoundError):
        shared_memory.SharedMemory(name=name)


# ---------------------------------------------------------------------------- CLI
def _cli(tmp_path, capsys, extra, tag, max_step=20):
    from apex_amd import train_host

    common = ["--env", "SeaquestNoFrameskip-v4", "--envs", "4", "--replay_buffer_size", "4096", "--threshold_size",
              "40", "--batch_size", "32", "--bps_interval", "5", "--save_interval", "0", "--learner-steps", "1",
              "--save-path", str(tmp_path / f"{tag}.pth"), "--no-tb", "--max-step", str(max_step), "--max_episode_length", "6"]
    capsys.readouterr()
    assert train_host.main(common + extra) == 0
    return capsys.readouterr().out


def test_train_host_cli_evaluator_flags(cuda, tmp_path, capsys):
    step = ["--eval-envs", "2", "--eval-mode", "step", "--eval-interval", "5", "--eval-steps", "12"]
    outs = [_cli(tmp_path, capsys, step, f"s{i}") for i in range(2)]
    nums = [re.findall(r"evaluator/\S+=\S+", o) for o in outs]
    assert nums[0] and nums[0] == nums[1]                    # deterministic: identical evaluator numbers
    assert any(n.startswith("evaluator/episode_reward=") for n in nums[0])
    assert any(n.startswith("evaluator/capped_episodes=") for n in nums[0])
    out = _cli(tmp_path, capsys, ["--eval-envs", "2", "--eval-mode", "async", "--eval-workers", "1", "--eval-kernel",
                                  "step"], "a", max_step=80)
    assert "evaluator: 2 greedy host envs, async mode" in out and "evaluator/episode_reward=" in out
    out = _cli(tmp_path, capsys, ["--eval-envs", "0"], "z")
    assert "evaluator" not in out
