#!/usr/bin/env python
"""One save and one load of an ``HBMReplay`` plus a ``DQNLearner`` through ``utils/engine_state.py``
at a given capacity, timed: wall time and GB/s of each, the save split into waiting for device
copies, file writes and digests, and the ``state_digest`` kernel's throughput on the frame ring
against a plain device read of the same bytes (``torch.sum`` over an ``int64`` view).  Prints one
JSON line.  ``--filled`` marks the whole replay live (random frame bytes, every row saved);
otherwise ``--rows`` transitions are live.  The run ends itself after ``--time-limit`` seconds.

    python scripts/diag/engine_state_timing.py --capacity 2000000 --filled --dir /tmp/state_timing
"""
import argparse
import json
import os
import shutil
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2048, help="live transitions when not --filled")
    ap.add_argument("--filled", action="store_true")
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--dir", default="/tmp/engine_state_timing")
    ap.add_argument("--digest-reps", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=300)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # (SIGALRM's default action ends the process)

    import torch

    from apex_amd.engine.hbm_replay import HBMReplay
    from apex_amd.engine.learner import DQNLearner, LearnerConfig
    from apex_amd.models.dqn import DuelingDQN
    from apex_amd.utils.engine_state import digest_tensor, load_engine_state, save_engine_state

    dev = torch.device("cuda", 0)
    rp = HBMReplay(a.capacity, a.envs, device=dev)
    learner = DQNLearner(DuelingDQN.from_shapes((4, 84, 84), 18), rp, LearnerConfig(batch_size=64, forward="hip"))
    rows = a.capacity if a.filled else min(a.rows, a.capacity)
    frame_rows = rp.frame_capacity if a.filled else min(rp.frame_capacity, rows + a.envs)
    g = torch.Generator(device=dev).manual_seed(1)
    step = 1 << 16
    for r0 in range(0, frame_rows, step):   # random bytes, a block of rows at a time
        n = min(step, frame_rows - r0)
        rp.frames[r0:r0 + n] = torch.randint(0, 256, (n, rp.frame_bytes), dtype=torch.uint8, device=dev, generator=g)
    rp.filled.fill_(rows)
    live = rp.live_rows(frame_rows)
    tensors = {f"replay.{k}": (t, live[k]) if k in live else t for k, t in rp.state_tensors().items()}
    tensors.update({f"learner.{k}": t for k, t in learner.state_tensors().items()})
    geometry = {"capacity": rp.capacity, "frame_capacity": rp.frame_capacity, "frame_bytes": rp.frame_bytes}
    path = os.path.join(a.dir, "state")
    shutil.rmtree(a.dir, ignore_errors=True)
    os.makedirs(a.dir)
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    m = save_engine_state(path, tensors, {"rows": rows}, geometry, chunk_bytes=a.chunk_mb << 20)
    t_save = time.perf_counter() - t0
    gb = m["total_bytes"] / 1e9
    for t in tensors.values():   # the load has to bring everything back
        (t[0][:t[1]] if isinstance(t, tuple) else t).zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    load_engine_state(path, tensors, geometry, chunk_bytes=a.chunk_mb << 20)
    t_load = time.perf_counter() - t0

    ring = rp.frames[:frame_rows]
    ring_gb = ring.numel() / 1e9
    words = ring.reshape(-1)[:ring.numel() // 8 * 8].view(torch.int64)
    digest_tensor(ring), words.sum()
    torch.cuda.synchronize()
    t_dig, t_sum = [], []
    for _ in range(a.digest_reps):
        t0 = time.perf_counter()
        digest_tensor(ring)   # (returns the value: synchronises)
        t_dig.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        words.sum()
        torch.cuda.synchronize()
        t_sum.append(time.perf_counter() - t0)
    out = {"capacity": a.capacity, "rows": rows, "frame_rows": frame_rows, "checkpoint_gb": round(gb, 3),
           "save_s": round(t_save, 3), "save_gb_s": round(gb / t_save, 2),
           "save_wait_copy_s": round(m["timing"]["copy"], 3), "save_write_s": round(m["timing"]["write"], 3),
           "save_digest_s": round(m["timing"]["digest"], 4),
           "load_s": round(t_load, 3), "load_gb_s": round(gb / t_load, 2),
           "ring_gb": round(ring_gb, 3), "digest_ms": round(1e3 * min(t_dig), 3),
           "digest_gb_s": round(ring_gb / min(t_dig), 1), "sum_int64_ms": round(1e3 * min(t_sum), 3),
           "sum_int64_gb_s": round(ring_gb / min(t_sum), 1)}
    print(json.dumps(out), flush=True)
    shutil.rmtree(a.dir, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
