"""hipGraph capture and the side-stream warm-up before it, shared by the DQN engines."""
from __future__ import annotations

import torch


def capture_graph(fn, pool=None) -> torch.cuda.CUDAGraph:
    """``fn()`` captured as one hipGraph on the current stream."""
    # thread_local capture: the process group's watchdog thread polls RCCL work events
    # while we capture; in the default (global) mode that call invalidates the capture
    # ("operation not permitted when stream is capturing", seen with --force-dp)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
        fn()
    return g


def warm_up(device, fn, iters: int) -> None:
    """``fn()`` ``iters`` times on a side stream that follows the current stream and that the
    current stream then follows (every kernel's first launch happens outside a capture).  No
    host synchronize: callers keep their own."""
    cur = torch.cuda.current_stream(device)
    s = torch.cuda.Stream(device=device)
    s.wait_stream(cur)
    with torch.cuda.stream(s):
        for _ in range(iters):
            fn()
    cur.wait_stream(s)
