"""Full-state checkpoints on the GPU: the ``state_digest`` kernel against its host definition,
exact resume of the GPU-env engine (a resumed run equals the uninterrupted run, bit for bit),
replay-preserving resume of the host-env engine with its frame-liveness invariant, and the
``--state-dir`` / ``--resume-state`` flags of both command lines."""
import os

import numpy as np
import pytest
import torch

from .host_env_util import twins

pytestmark = pytest.mark.gpu

DIGEST_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 3 * 7056 + 5, (1 << 20) + 5]


# ---------------------------------------------------------------------------- digest kernel
@pytest.fixture(scope="module")
def noise(cuda):
    """Random bytes, on the host and on the device (8 spare bytes for the offset views)."""
    host = np.random.default_rng(11).integers(0, 256, max(DIGEST_LENGTHS) + 8, dtype=np.uint8)
    return host, torch.from_numpy(host).to(cuda)


@pytest.mark.parametrize("n", DIGEST_LENGTHS)
def test_digest_kernel_equals_host_at_every_offset(noise, n):
    from apex_amd.utils.engine_state import digest_host, digest_tensor

    host, dev = noise
    for off in (0, 1, 3, 8):   # the allocation is 256-byte aligned: these bases are misaligned by off
        assert dev.data_ptr() % 16 == 0
        assert digest_tensor(dev[off:off + n]) == digest_host(host[off:off + n]), (n, off)


@pytest.mark.parametrize("dtype", [torch.int32, torch.float32, torch.float64, torch.int64])
def test_digest_kernel_on_typed_tensors(cuda, dtype):
    from apex_amd.utils.engine_state import digest_host, digest_tensor

    g = torch.Generator().manual_seed(5)
    t = torch.randint(-1 << 30, 1 << 30, (37, 13), generator=g).to(dtype)
    assert digest_tensor(t.to(cuda)) == digest_host(t.numpy().tobytes()) == digest_tensor(t)


def test_digest_kernel_sees_first_middle_and_last_byte(noise):
    from apex_amd.utils.engine_state import digest_tensor

    _, dev = noise
    buf = dev[:3 * 7056 + 5].clone()
    ref = digest_tensor(buf)
    for i in (0, buf.numel() // 2, buf.numel() - 1):
        buf[i] ^= 0x40
        assert digest_tensor(buf) != ref, i
        buf[i] ^= 0x40
    assert digest_tensor(buf) == ref


def test_digest_rejects_non_contiguous(cuda):
    from apex_amd.utils.engine_state import digest_tensor

    with pytest.raises(ValueError):
        digest_tensor(torch.zeros(8, 6, device=cuda).t())
    with pytest.raises(ValueError):
        digest_tensor(torch.zeros(64, dtype=torch.uint8, device=cuda)[::2])


# ---------------------------------------------------------------------------- GPU-env engine
def _engine(cuda, overlap: bool, graphs: bool, seed: int = 1122):
    """The configuration of ``test_training_left_bit_identical``: fill (32 actor steps) and, with
    graphs, capture (3 warm-up train steps)."""
    from apex_amd.engine.apex import ApexEngine, EngineConfig
    from apex_amd.engine.learner import LearnerConfig

    cfg = EngineConfig(n_envs=64, replay_capacity=4096, threshold_size=2048, overlap=overlap, use_graphs=graphs,
                       publish_param_interval=4, target_update_interval=6, seed=seed,
                       learner=LearnerConfig(batch_size=256, forward="hip"))
    eng = ApexEngine(cfg, cuda)
    eng.fill()
    if graphs:
        eng.capture()
    return eng


def _steps(eng, n: int) -> None:
    for _ in range(n):
        eng.train_step()
    torch.cuda.synchronize()


def _snapshot(eng) -> tuple[dict, dict]:
    torch.cuda.synchronize()   # (device-wide: the actor stream included)
    return {k: t.clone() for k, t in eng.state_tensors().items()}, eng.host_state()


def _assert_same_state(a, b, what: str) -> None:
    (ta, ha), (tb, hb) = a, b
    assert ta.keys() == tb.keys()
    for k in ta:
        assert torch.equal(ta[k], tb[k]), f"{what}: {k}"
    assert ha == hb, what


@pytest.mark.parametrize("overlap,graphs", [(True, True), (False, False)], ids=["overlap-graphs", "serial-eager"])
def test_resumed_run_equals_the_uninterrupted_run(cuda, tmp_path, overlap, graphs):
    """A: 80 steps (frame ring of 78 steps and slot ring of 64 steps both wrapped), save, 24 more.
    B: another seed, fill, capture, load, 24 steps.  C: like A without the save, 104 steps."""
    path = str(tmp_path / "state")
    eng_a = _engine(cuda, overlap, graphs)
    _steps(eng_a, 80)
    assert int(eng_a.actor.step_counter.item()) >= 78 and len(eng_a.replay) == 4096
    eng_a.save_state(path)
    _steps(eng_a, 24)
    a = _snapshot(eng_a)
    eng_c = _engine(cuda, overlap, graphs)
    _steps(eng_c, 104)
    _assert_same_state(_snapshot(eng_c), a, "uninterrupted control")   # (else B == A would prove nothing)
    del eng_c
    eng_b = _engine(cuda, overlap, graphs, seed=77)
    assert not torch.equal(eng_b.learner.flat, eng_a.learner.flat)
    eng_b.load_state(path)
    _steps(eng_b, 24)
    _assert_same_state(_snapshot(eng_b), a, "resumed")
    assert eng_b.learn_steps == eng_a.learn_steps == (3 if graphs else 0) + 104


@pytest.mark.parametrize("chunk", [64 << 20, (1 << 20) + 3], ids=["chunk-64M", "chunk-1M+3"])
def test_state_right_after_a_load(cuda, tmp_path, chunk):
    """Every listed tensor equals its clone taken at save time; saving the loaded engine again
    gives the same per-tensor digests; the rebuilt packed weights equal the saved engine's."""
    from apex_amd.utils.engine_state import read_manifest

    path, again = str(tmp_path / "state"), str(tmp_path / "again")
    eng_a = _engine(cuda, True, True)
    _steps(eng_a, 80)
    saved = _snapshot(eng_a)
    manifest = eng_a.save_state(path, chunk_bytes=chunk)
    _assert_same_state(_snapshot(eng_a), saved, "saving changes nothing")
    assert manifest["tensors"]["replay.frames"]["rows"] == eng_a.replay.frame_capacity
    eng_b = _engine(cuda, True, True, seed=77)
    host = eng_b.load_state(path, chunk_bytes=chunk)
    assert host == saved[1]
    _assert_same_state(_snapshot(eng_b), saved, "after load")
    assert torch.equal(eng_b.learner.net.arena, eng_a.learner.net.arena)   # (the optimizer maintains all of it)
    for x, y in ((eng_b.learner.tnet, eng_a.learner.tnet), (eng_b.policy.net, eng_a.policy.net)):
        assert torch.equal(x.arena[:x.fwd_numel], y.arena[:y.fwd_numel])   # (forward layouts: what they read)
    second = eng_b.save_state(again, chunk_bytes=chunk)
    assert {k: e["digest"] for k, e in second["tensors"].items()} == \
        {k: e["digest"] for k, e in read_manifest(path)["tensors"].items()}
    assert second["host"] == manifest["host"] and second["geometry"] == manifest["geometry"]


def test_barely_filled_replay_saves_live_rows_only(cuda, tmp_path):
    """Before the rings wrap only the rows written so far are saved, and a mismatching engine
    or an unsupported topology is refused."""
    from apex_amd.engine.apex import ApexEngine, EngineConfig
    from apex_amd.engine.learner import LearnerConfig
    from apex_amd.utils.engine_state import CheckpointError

    def engine(capacity=8192, batch=64, seed=3):
        cfg = EngineConfig(n_envs=64, replay_capacity=capacity, threshold_size=1024, seed=seed,
                           learner=LearnerConfig(batch_size=batch, forward="hip"))
        eng = ApexEngine(cfg, cuda)
        eng.fill()
        return eng

    eng = engine()
    _steps(eng, 4)
    path = str(tmp_path / "state")
    m = eng.save_state(path)
    steps = int(eng.actor.step_counter.item())
    assert steps == 16 + 4
    assert m["tensors"]["replay.frames"]["rows"] == (steps + 1) * 64
    assert m["tensors"]["replay.s_ids"]["rows"] == m["tensors"]["replay.leaf_sum"]["rows"] == steps * 64
    assert sum(e["nbytes"] for k, e in m["tensors"].items() if k.startswith("replay.")) < eng.replay.nbytes() // 4
    saved = _snapshot(eng)
    other = engine(seed=9)
    other.load_state(path)
    _assert_same_state(_snapshot(other), saved, "partial rows")
    with pytest.raises(CheckpointError, match="'capacity'"):
        engine(capacity=4096).load_state(path)
    with pytest.raises(CheckpointError, match="'batch'"):
        engine(batch=256).load_state(path)
    eng._allreduce = object()
    with pytest.raises(NotImplementedError):
        eng.save_state(path)


# ---------------------------------------------------------------------------- host-env engine
class _Liveness:
    """Write times of every frame position and every slot's row, kept from the step counter: a
    step with counter ``c`` writes frames ``((c + 1) * E + e) % F`` and, where it emitted, rows
    ``(c * E + e) % C``; a reset writes frames ``(c * E + e) % F``."""

    def __init__(self, E, C, F):
        self.E, self.C, self.F, self.tick = E, C, F, 0
        self.frame_time = np.full(F, -1, dtype=np.int64)
        self.row_time = np.full(C, -1, dtype=np.int64)

    def reset(self, counter: int) -> None:
        self.tick += 1
        self.frame_time[(counter * self.E + np.arange(self.E)) % self.F] = self.tick

    def step(self, counter: int, emitted: np.ndarray) -> None:
        self.tick += 1
        self.frame_time[((counter + 1) * self.E + np.arange(self.E)) % self.F] = self.tick
        slots = (counter * self.E + np.arange(self.E)) % self.C
        self.row_time[slots[emitted]] = self.tick

    def check(self, replay) -> None:
        live = (replay.leaf_sum > 0).cpu().numpy()
        if not live.any():   # (the first n - 1 steps of a run emit nothing)
            return
        ids = torch.cat([replay.s_ids, replay.s2_ids], 1).cpu().numpy()[live]
        newest = self.frame_time[ids].max(1)
        assert (self.row_time[live] >= 0).all()
        assert (newest <= self.row_time[live]).all(), "a sampleable row references a frame written after it"


def _host_engine(forward, batch, seed):
    from apex_amd.engine.host_env import HostEnvConfig, HostEnvEngine
    from apex_amd.engine.learner import LearnerConfig

    raw, _ = twins("Pong", 4, seed=seed)
    cfg = HostEnvConfig(replay_capacity=256, threshold_size=32, learner_steps_per_actor_step=1, seed=seed,
                        publish_param_interval=4, target_update_interval=10,
                        learner=LearnerConfig(batch_size=batch, forward=forward))
    return HostEnvEngine(cfg, raw, "cuda:0")


def _iterate(eng, live: _Liveness, n: int) -> None:
    for _ in range(n):
        c = int(eng.actor.step_counter.item())
        eng.iteration()
        torch.cuda.synchronize()
        assert int(eng.actor.step_counter.item()) == c + 1
        live.step(c, (eng.actor.prio > 0).cpu().numpy())
        live.check(eng.replay)
        rp = eng.replay
        assert float(rp.node_sum[-1][0]) == pytest.approx(float(rp.leaf_sum.double().sum()), rel=1e-9)
        if eng.learn_steps:
            assert np.isfinite(eng.learner.stats()["loss"])


@pytest.mark.parametrize("forward,batch", [("torch", 16), ("hip", 32)])
def test_host_env_resume_keeps_the_replay_alive(cuda, tmp_path, forward, batch):
    """100 iterations (slot ring of 64 steps and frame ring of 78 steps wrapped), then three
    save / fresh engine / load / 40 iterations cycles; the liveness invariant holds throughout."""
    path = str(tmp_path / "state")
    eng = _host_engine(forward, batch, seed=5)
    E, C, F = eng.E, eng.replay.capacity, eng.replay.frame_capacity
    assert (E, C, F) == (4, 256, 256 + 14 * 4)
    live = _Liveness(E, C, F)
    live.reset(0)
    _iterate(eng, live, 100)
    assert bool((eng.replay.leaf_sum > 0).any())
    for cycle in range(3):
        eng.save_state(path)
        saved = {k: t.clone() for k, t in eng.state_tensors().items()}
        s = int(saved["actor.step_counter"].item())
        learn_steps, actor_steps = eng.learn_steps, eng.actor_steps
        assert s == actor_steps
        eng.close()
        eng = _host_engine(forward, batch, seed=100 + cycle)
        eng.load_state(path)
        live.reset(s + 1)   # the dead step: its frames come from the reset, its slots are dead
        assert eng.learn_steps == learn_steps and eng.actor_steps == actor_steps + 1
        now = eng.state_tensors()
        dead = (s * E + torch.arange(E, device=cuda)) % C
        fresh = ((s + 1) * E + torch.arange(E, device=cuda)) % F
        keep_slot = torch.ones(C, dtype=torch.bool, device=cuda)
        keep_slot[dead] = False
        keep_frame = torch.ones(F, dtype=torch.bool, device=cuda)
        keep_frame[fresh] = False
        for k, t in saved.items():
            if k in ("replay.leaf_sum", "replay.leaf_min"):
                assert torch.equal(now[k][keep_slot], t[keep_slot]), k
            elif k == "replay.frames":
                assert torch.equal(now[k][keep_frame], t[keep_frame]), k
            elif k == "replay.filled":
                assert int(now[k].item()) == int(t.item()) + E
            elif k == "actor.step_counter":
                assert int(now[k].item()) == s + 1
            elif k.startswith("replay.node_"):
                continue   # ancestors of the dead slots: pinned by root == sum of leaves below
            else:
                assert torch.equal(now[k], t), k
        rp = eng.replay
        assert bool((rp.leaf_sum[dead] == 0).all()) and bool(torch.isinf(rp.leaf_min[dead]).all())
        assert float(rp.node_sum[-1][0]) == pytest.approx(float(rp.leaf_sum.double().sum()), rel=1e-9)
        assert torch.equal(eng.actor_flat, saved["policy.flat"])
        live.check(rp)
        _iterate(eng, live, 40)
        assert eng.learn_steps == learn_steps + 40 + 3   # (a fresh engine's 3 warm-up steps before its capture)
    eng.close()


# ---------------------------------------------------------------------------- command lines
def test_train_cli_resume_state_is_bit_exact(cuda, tmp_path, capsys):
    from apex_amd import train
    from apex_amd.utils.checkpoint import sidecar_path

    def flags(name):
        return ["--n-envs", "64", "--replay_buffer_size", "16384", "--threshold_size", "2048", "--bps_interval", "10",
                "--save_interval", "20", "--target_update_interval", "15", "--save-path", str(tmp_path / name),
                "--no-tb"]

    s1, s2 = str(tmp_path / "S1"), str(tmp_path / "S2")
    assert train.main(flags("a.pth") + ["--max-step", "30", "--state-dir", s1]) == 0
    assert train.main(flags("b.pth") + ["--max-step", "15", "--state-dir", s2]) == 0
    capsys.readouterr()
    assert train.main(flags("b.pth") + ["--resume-state", s2, "--max-step", "30"]) == 0
    assert f"resumed full state from {s2} at step 15" in capsys.readouterr().out
    a = torch.load(str(tmp_path / "a.pth"), map_location="cpu", weights_only=True)
    b = torch.load(str(tmp_path / "b.pth"), map_location="cpu", weights_only=True)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    sa = torch.load(sidecar_path(str(tmp_path / "a.pth")), map_location="cpu", weights_only=True)
    sb = torch.load(sidecar_path(str(tmp_path / "b.pth")), map_location="cpu", weights_only=True)
    for k in ("opt_s1", "opt_s2", "step_counter"):
        assert torch.equal(sa[k], sb[k]), k
    assert int(sa["step_counter"].item()) == 30
    assert os.path.isfile(os.path.join(s1, "manifest.pt")) and os.path.isfile(os.path.join(s2, "data.bin"))
    with pytest.raises(SystemExit) as e:
        train.main(flags("b.pth") + ["--resume-state", s2, "--resume", str(tmp_path / "b.pth"), "--max-step", "31"])
    assert e.value.code not in (0, None)


def test_train_host_cli_resume_state_keeps_the_replay(cuda, tmp_path, capsys):
    import re

    from apex_amd import train_host
    from apex_amd.utils.engine_state import read_manifest

    ck, sd = str(tmp_path / "model.pth"), str(tmp_path / "S")
    common = ["--env", "SeaquestNoFrameskip-v4", "--envs", "4", "--replay_buffer_size", "4096", "--threshold_size",
              "40", "--batch_size", "32", "--bps_interval", "5", "--save_interval", "10", "--learner-steps", "1",
              "--save-path", ck, "--no-tb"]
    assert train_host.main(common + ["--max-step", "20", "--state-dir", sd]) == 0
    host = read_manifest(sd)["host"]
    saved_size = host["actor_steps"] * 4
    assert 20 <= host["learn_steps"] <= 22 and saved_size >= 40 + 4 * 17
    capsys.readouterr()
    assert train_host.main(common + ["--max-step", str(host["learn_steps"] + 10), "--resume-state", sd]) == 0
    out = capsys.readouterr().out
    assert f"resumed full state from {sd} at step {host['learn_steps']}" in out
    first = re.search(r"^Step: (\d+) .*replay/size=([0-9.e+]+)", out, re.M)
    assert first is not None and int(first.group(1)) <= host["learn_steps"] + 6
    assert float(first.group(2)) >= saved_size   # (four significant digits: exact below 10,000)
    with pytest.raises(SystemExit) as e:
        train_host.main(common + ["--max-step", "40", "--resume-state", sd, "--resume", ck])
    assert e.value.code not in (0, None)
