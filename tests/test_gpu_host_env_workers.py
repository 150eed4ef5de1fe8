"""GPU tests of the host-env engine over emulator worker processes: the ranged ingest launch
against the whole launch (byte for byte, in both orders, nothing written outside the range, bad
ranges refused before launching), H2D copies out of a registered shared-memory block, the engine
over ``ProcRawAtariVector`` against the engine over ``RawAtariVector`` (banked and whole ingest),
and the ``train_host --workers`` CLI."""
import functools
import os
from multiprocessing import shared_memory

import numpy as np
import pytest
import torch

from . import proc_vector_fixtures as fx

pytestmark = pytest.mark.gpu

FB = 7056
SENTINEL = 0xAB
OUTPUTS = ("frames", "reward", "done", "new_frame", "hist", "acc", "ep_log")


class _Rig:
    """Sentinel-filled tensors around ``host_env_ingest`` / ``host_env_ingest_range`` launches."""

    def __init__(self, dev, E, H, W, F, step, pairs, reward_in, done_in):
        from apex_amd.engine.host_env import Ingest

        self.ingest = Ingest(E, H, W, FB, F, True, dev)
        f32 = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=dev)          # noqa: E731
        i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)              # noqa: E731
        self.frames = torch.full((F, FB), SENTINEL, dtype=torch.uint8, device=dev)
        self.raw = torch.from_numpy(pairs).to(dev)
        self.reward_in = torch.from_numpy(reward_in).to(dev)
        self.done_in = torch.from_numpy(done_in).to(dev)
        self.reward, self.done, self.new_frame, self.hist = f32(E), f32(E), i32(E), i32(E, 4)
        self.acc, self.ep_log = f32(E, 4), f32(E, 4)
        self.acc[:] = torch.arange(E * 4, dtype=torch.float32, device=dev).reshape(E, 4)
        self.ep_log[:] = 100 + torch.arange(E * 4, dtype=torch.float32, device=dev).reshape(E, 4)
        self.step = torch.full((1,), step, dtype=torch.int64, device=dev)

    def _args(self, reset):
        return (self.raw, self.reward_in, self.done_in, self.frames, self.step, reset, self.reward, self.done,
                self.new_frame, self.hist, self.acc, self.ep_log)

    def whole(self, reset):
        self.ingest(*self._args(reset))

    def range(self, e0, n, reset):
        self.ingest.range(e0, n, *self._args(reset))

    def outputs(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in OUTPUTS}


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    E = 5
    rng = np.random.default_rng(100 * H + W)
    pairs = rng.integers(0, 256, (E, 2, H, W, 3), dtype=np.uint8)
    reward_in = np.array([2.0, -3.0, 0.0, 0.5, -0.25], np.float32)
    done_in = np.array([0, 1, 0, 1, 0], np.float32)
    return pairs, reward_in, done_in


E, F = 5, 16


def _step(reset):
    """The step counter at which the launch's slots are 30 .. 34 mod 16 = 14, 15, 0, 1, 2: the ring wraps
    inside the launch, and inside the first range."""
    return 6 if reset else 5


def _slots(reset):
    return [((_step(reset) + (0 if reset else 1)) * E + e) % F for e in range(E)]


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("H,W", [(210, 160), (84, 84)])
def test_ranged_ingest_equals_whole_ingest(cuda, H, W, reset, order):
    want_rig = _Rig(cuda, E, H, W, F, _step(reset), *_inputs(H, W))
    want_rig.whole(reset)
    want = want_rig.outputs()
    slots = _slots(reset)
    assert want["new_frame"].tolist() == slots == [14, 15, 0, 1, 2]
    assert (want["frames"][slots] != SENTINEL).any()
    rig = _Rig(cuda, E, H, W, F, _step(reset), *_inputs(H, W))
    ranges = [(0, 2), (2, 3)]
    for e0, n in (ranges if order == "forward" else ranges[::-1]):
        rig.range(e0, n, reset)
    got = rig.outputs()
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k]), k
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("reset", [False, True])
def test_one_range_leaves_the_other_envs_untouched(cuda, reset):
    H, W = 210, 160
    fresh = _Rig(cuda, E, H, W, F, _step(reset), *_inputs(H, W)).outputs()
    whole = _Rig(cuda, E, H, W, F, _step(reset), *_inputs(H, W))
    whole.whole(reset)
    want = whole.outputs()
    rig = _Rig(cuda, E, H, W, F, _step(reset), *_inputs(H, W))
    rig.range(2, 3, reset)
    got = rig.outputs()
    mine = _slots(reset)[2:]
    others = [s for s in range(F) if s not in mine]
    assert np.array_equal(got["frames"][mine], want["frames"][mine])
    assert (got["frames"][others] == SENTINEL).all()                # slots of envs 0, 1 included
    for k in OUTPUTS[1:]:
        assert np.array_equal(got[k][2:], want[k][2:]), k
        assert np.array_equal(got[k][:2], fresh[k][:2]), k          # rows of envs 0, 1 keep their sentinels


def test_range_launcher_rejects_bad_ranges_before_launching(cuda):
    rig = _Rig(cuda, E, 84, 84, F, 5, *_inputs(84, 84))
    before = rig.outputs()
    for e0, n in [(-1, 2), (0, 0), (2, 4), (5, 1), (0, -1)]:        # e0 = -1, n = 0, e0 + n = 6, ...
        with pytest.raises(ValueError):
            rig.range(e0, n, False)
    after = rig.outputs()
    for k in OUTPUTS:
        assert np.array_equal(after[k], before[k]), k


# ---------------------------------------------------------------------------- registered staging
def test_registered_shared_block_copies_on_a_side_stream(cuda):
    from apex_amd import ops

    hip = ops.hip()
    n = 3 * 2 * 210 * 160 * 3 + 5                                   # not a multiple of the page size
    shm = shared_memory.SharedMemory(create=True, size=n)
    try:
        src = np.ndarray((n,), dtype=np.uint8, buffer=shm.buf)
        src[:] = np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8)
        ptr = int(src.ctypes.data)
        with pytest.raises((ValueError, RuntimeError)):
            hip.host_register(ptr, 0)                               # a zero-length registration is refused
        hip.host_register(ptr, n)
        try:
            dst = torch.zeros(n, dtype=torch.uint8, device=cuda)
            side = torch.cuda.Stream(device=cuda)
            side.wait_stream(torch.cuda.current_stream())
            off = 2 * 210 * 160 * 3                                 # one bank's slice, then the rest
            hip.memcpy_h2d_async(dst.data_ptr() + off, ptr + off, n - off, side.cuda_stream)
            hip.memcpy_h2d_async(dst.data_ptr(), ptr, off, side.cuda_stream)
            hip.memcpy_h2d_async(dst.data_ptr(), ptr, 0, side.cuda_stream)   # nothing to do
            side.synchronize()
            assert np.array_equal(dst.cpu().numpy(), src)
            with pytest.raises(ValueError):
                hip.memcpy_h2d_async(dst.data_ptr(), ptr, -1, side.cuda_stream)
        finally:
            hip.host_unregister(ptr)                                # succeeds (raises otherwise)
        del src
    finally:
        shm.close()
        shm.unlink()


# ---------------------------------------------------------------------------- engine
ENV = "SeaquestNoFrameskip-v4"
FACTORY = "tests.proc_vector_fixtures:short"


def _run_engine(vec, ingest, iters=40):
    from apex_amd.engine.host_env import HostEnvConfig, HostEnvEngine
    from apex_amd.engine.learner import LearnerConfig

    cfg = HostEnvConfig(replay_capacity=256, threshold_size=64, learner_steps_per_actor_step=1,
                        publish_param_interval=5, target_update_interval=20, seed=7, ingest=ingest,
                        learner=LearnerConfig(batch_size=32, forward="hip", seed=7))
    eng = HostEnvEngine(cfg, vec, "cuda:0")
    try:
        for _ in range(iters):
            eng.iteration()
        torch.cuda.synchronize()
        rp = eng.replay
        out = {"frames": rp.frames.clone(), "ep_log": eng.actor.ep_log.clone(),
               "step_counter": eng.actor.step_counter.clone(), "flat": eng.learner.flat.clone(),
               "leaves": rp.leaf_sum.clone()}
        out.update({k: getattr(rp, k).clone() for k in ("s_ids", "s2_ids", "action", "reward", "done")})
        return out, eng.learn_steps, eng.ingest
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _in_process_run():
    from apex_amd.envs.raw_vector import RawAtariVector

    vec = RawAtariVector([fx.short(ENV) for _ in range(4)])
    vec.seed(5)
    return _run_engine(vec, "auto")


@pytest.mark.parametrize("ingest", ["banked", "whole"])
def test_engine_over_workers_equals_engine_in_process(cuda, ingest):
    from apex_amd.envs.proc_vector import ProcRawAtariVector

    want, steps, resolved = _in_process_run()
    assert resolved == "whole" and steps == 3 + (40 - 16)           # learning from 64 rows = iteration 17
    assert float(want["ep_log"][:, 2].sum()) >= 4                   # episodes ended: ep_log is not trivial
    vec = ProcRawAtariVector(ENV, 4, workers=2, seed=5, factory=FACTORY)
    got, got_steps, resolved = _run_engine(vec, ingest)
    assert resolved == ingest and got_steps == steps
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert vec.processes and all(not p.is_alive() for p in vec.processes)
    with pytest.raises(FileNotFoundError):
        shared_memory.SharedMemory(name=vec.shm_name)


def test_engine_auto_is_banked_over_workers_and_banked_needs_banks(cuda):
    from apex_amd.engine.host_env import HostEnvConfig, HostEnvEngine
    from apex_amd.envs.proc_vector import ProcRawAtariVector
    from apex_amd.envs.raw_vector import RawAtariVector

    local = RawAtariVector([fx.short(ENV) for _ in range(2)])
    for bad in ("banked", "sometimes"):
        with pytest.raises(ValueError):
            HostEnvEngine(HostEnvConfig(replay_capacity=256, ingest=bad), local, "cuda:0")
    with ProcRawAtariVector(ENV, 2, workers=2, seed=1) as vec:
        eng = HostEnvEngine(HostEnvConfig(replay_capacity=256, learner_steps_per_actor_step=0), vec, "cuda:0")
        assert eng.ingest == "banked" and eng.actor.raw_np is vec.staging
        eng.iteration()
        eng.close()                                                 # closes the pool too
        assert all(not p.is_alive() for p in vec.processes)
        eng.close()                                                 # idempotent


# ---------------------------------------------------------------------------- CLI
def test_train_host_cli_with_workers_saves_resumes_and_equals_in_process(cuda, tmp_path, capsys):
    import multiprocessing

    from apex_amd import train_host
    from apex_amd.utils.checkpoint import sidecar_path

    def flags(ck):
        return ["--env", ENV, "--envs", "4", "--replay_buffer_size", "1024", "--threshold_size", "40",
                "--batch_size", "32", "--bps_interval", "5", "--save_interval", "10", "--learner-steps", "1",
                "--save-path", ck, "--no-tb"]

    ck_w, ck_0 = str(tmp_path / "workers.pth"), str(tmp_path / "local.pth")
    assert train_host.main(flags(ck_w) + ["--workers", "2", "--worker-timeout", "30", "--max-step", "12"]) == 0
    assert "4 host envs in 2 worker processes (banked ingest)" in capsys.readouterr().out
    assert train_host.main(flags(ck_0) + ["--workers", "0", "--max-step", "12"]) == 0
    a = torch.load(ck_w, map_location="cpu", weights_only=True)
    b = torch.load(ck_0, map_location="cpu", weights_only=True)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    n1 = torch.load(sidecar_path(ck_w), map_location="cpu", weights_only=True)["counters"]["learn_steps"]
    assert 12 <= n1 <= 14
    assert train_host.main(flags(ck_w) + ["--workers", "2", "--ingest", "whole", "--max-step", str(n1 + 6),
                                          "--resume", ck_w]) == 0
    out = capsys.readouterr().out
    assert f"training from step {n1}" in out and "(whole ingest)" in out
    n2 = torch.load(sidecar_path(ck_w), map_location="cpu", weights_only=True)["counters"]["learn_steps"]
    assert n1 + 6 <= n2 <= n1 + 8 and os.path.exists(ck_w)
    assert not [p for p in multiprocessing.active_children() if p.name.startswith("apex-env-worker")]
