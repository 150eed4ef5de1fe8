"""The host side of greedy evaluation that every engine shares.

* :class:`SideStreamEvaluation`: evaluation beside training.  A launch snapshots the weights on
  the current (training) stream and plays them on a side stream; the result lands in pinned host
  memory and is handed over exactly once.  Evaluations conflate: while one is in flight a
  further launch does nothing.  ``AtariEvaluator``, ``VectorEvaluator`` and ``AQLEvaluator`` are
  its subclasses; the latter two share :class:`RolloutEvaluation`.
* :class:`RolloutBuffers`: the device outputs of a one-launch rollout of ``n`` episodes
  (``vec_rollout`` / ``aql_rollout``) and their pinned host mirrors.
* :class:`GreedyRollouts`: ``_eval_seed`` / ``rollout_evaluate`` of the engines that own such
  buffers.
"""
from __future__ import annotations

import collections

import torch


class SideStreamEvaluation:
    """Greedy evaluation beside training.  A subclass's ``launch()`` hands :meth:`_launch` a
    snapshot of the source weights, taken on the current (training) stream, and a play -- the
    rollout and its copies to pinned host memory -- issued on the side stream; ``poll()`` /
    ``wait()`` hand each landed result (``{"tag": ..., **_result()}``) over exactly once.  While
    a launch is in flight a further one does nothing (the snapshot may still be read by the
    running kernel): evaluations conflate, as the reference's evaluator process does.  The
    training stream never waits on the side stream; all launches are eager, issued between
    graph replays, so no captured graph gains a node.

    ``stream`` / ``event`` / ``stream_ctx`` default to ``torch.cuda``'s (host tests pass fakes)."""

    def __init__(self, device, stream=None, event=None, stream_ctx=None):
        self.device = device
        self.stream = torch.cuda.Stream(device=device) if stream is None else stream
        self._ctx = torch.cuda.stream if stream_ctx is None else stream_ctx
        make = torch.cuda.Event if event is None else event
        self.snapshot_taken, self.results_landed = make(), make()
        self._pending = False   # a launch whose result is still on its way to the host
        self._tag = None
        self._done = collections.deque()   # landed results not yet handed over
        self.launches = 0

    def _launch(self, tag, snapshot, play) -> bool:
        """``snapshot()`` on the current stream, then ``play()`` on the side stream once the
        snapshot is taken.  ``False`` (and nothing called) while the previous launch has not
        landed."""
        if self._pending:
            if not self.results_landed.query():
                return False
            self._harvest()  # the pinned buffers are about to be reused
        snapshot()
        self.snapshot_taken.record()
        with self._ctx(self.stream):
            self.stream.wait_event(self.snapshot_taken)
            play()
            self.results_landed.record()
        self._pending, self._tag = True, tag
        self.launches += 1
        return True

    def _result(self) -> dict:
        """The landed pinned buffers as a result dict (without ``tag``)."""
        raise NotImplementedError

    def _harvest(self) -> None:
        self._pending = False
        self._done.append({"tag": self._tag, **self._result()})

    def poll(self) -> dict | None:
        """The oldest landed result not yet handed over (each exactly once), or ``None``."""
        if self._pending and self.results_landed.query():
            self._harvest()
        return self._done.popleft() if self._done else None

    def wait(self) -> dict | None:
        """As ``poll()``, but blocks until the launch in flight has landed: on the results event
        only, never on the device.  ``None`` if nothing was launched."""
        if self._done:
            return self._done.popleft()
        if not self._pending:
            return None
        self.results_landed.synchronize()
        self._harvest()
        return self._done.popleft()

    def latest(self, block: bool = False) -> dict | None:
        """The newest landed result, or ``None``; older ones not yet handed over are dropped
        (they are superseded).  ``block``: wait out the launch in flight first."""
        take, res = self.wait if block else self.poll, None
        while (r := take()) is not None:
            res = r
        return res


class RolloutBuffers:
    """Device outputs of a one-launch greedy rollout of ``n`` episodes: the return, the length
    and the ended flag of each.  Subclasses add the launch."""
    KEYS = ("returns", "lengths", "ended")

    def __init__(self, n: int, device):
        self.n = int(n)
        self.returns = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.lengths = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.ended = torch.zeros(self.n, dtype=torch.int32, device=device)

    def pinned(self) -> dict:
        """Pinned host mirrors of the outputs."""
        return {k: torch.zeros_like(getattr(self, k), device="cpu").pin_memory() for k in self.KEYS}

    def copy_to(self, host: dict) -> None:
        """Asynchronous copies of the outputs into ``host`` on the current stream."""
        for k, h in host.items():
            h.copy_(getattr(self, k), non_blocking=True)


class RolloutEvaluation(SideStreamEvaluation):
    """:class:`SideStreamEvaluation` of an engine with :class:`GreedyRollouts`: ``ro`` (rollout
    buffers over a network handle of the snapshot) plays ``ro.n`` episodes of at most ``limit``
    steps.  Subclasses build the snapshot network and supply ``_snapshot()``."""

    def __init__(self, engine, ro: RolloutBuffers, limit: int, **side):
        super().__init__(engine.device, **side)
        self.engine, self.ro, self.limit = engine, ro, int(limit)
        self.host = ro.pinned()

    def launch(self, seed: int | None = None, tag=None) -> bool:
        """Start one evaluation of the online weights as they are at this point of the current
        stream.  ``False`` (and nothing done) while the previous one has not landed."""
        sd = self.engine._eval_seed(seed)
        return self._launch(tag, self._snapshot, lambda: self._play(sd))

    def _snapshot(self) -> None:
        raise NotImplementedError

    def _play(self, seed: int) -> None:
        self.ro.launch(seed, self.limit)
        self.ro.copy_to(self.host)

    def _result(self) -> dict:
        return {k: h.tolist() for k, h in self.host.items()}


class GreedyRollouts:
    """``_eval_seed`` and ``rollout_evaluate`` of an engine.  The engine states ``_eval_steps``
    (the step counter that enters the default seed), ``_eval_limit`` (the default episode limit)
    and ``_make_rollout(n)`` (its :class:`RolloutBuffers` over the online weights), and keeps
    ``cfg.seed``."""
    _rollout = None

    def _eval_seed(self, seed: int | None) -> int:
        """The 48-bit env seed of an evaluation (default: ``cfg.seed``, a constant and the step
        counter)."""
        sd = (self.cfg.seed * 7919 + 0xE7A1 + self._eval_steps) if seed is None else int(seed)
        return sd & 0xFFFFFFFFFFFF

    def rollout_evaluate(self, episodes: int = 10, seed: int | None = None,
                         max_episode_steps: int | None = None) -> list[float]:
        """Greedy returns of ``episodes`` episodes, one env each, with the online weights: one
        rollout launch on the current stream plays them from reset to their first done, then one
        read-back.  Nothing is written to the replay.  The same seed and weights give the same
        floats, bit for bit those of the engine's stepwise ``evaluate()`` where it has one.  The
        weights are read in place (the caller's stream order protects them)."""
        n = int(episodes)
        limit = int(self._eval_limit if max_episode_steps is None else max_episode_steps)
        if self._rollout is None or self._rollout.n != n:
            self._rollout = self._make_rollout(n)
        self._rollout.launch(self._eval_seed(seed), limit)
        return self._rollout.returns.tolist()
