"""GPU actor shard: E vectorised envs + batched inference + on-device n-step batcher.

Replaces the reference's per-process actor loop (origin_repo/actor.py:52-115,
batchrecorder.py:42-78): one actor step of the whole shard is

  gather obs stacks (frame ids -> u8 [E,4,84,84])  ->  Q = policy(obs) [E,A]
  -> epsilon-greedy with the Ape-X ladder eps_i = 0.4^(1 + 7 i/(N-1)) on device
  -> vec env step (renders new frames straight into the HBM frame ring)
  -> n-step emit (transition + actor-computed priority written into replay slots)
  -> priority-tree leaf write + level recompute

Every op is a kernel on the caller's stream with static buffers, so the whole actor
step is captured into one hipGraph by :class:`apex_amd.engine.apex.ApexEngine`.
Actor ids are global (``actor_offset`` + local index) so the epsilon ladder spans
all shards of all ranks.
"""
from __future__ import annotations

import torch

from .hbm_replay import HBMReplay
from .shard import NStepShard

ENV_STATE_STRIDE = 32


class ActorShard(NStepShard):
    def __init__(self, replay: HBMReplay, n_envs: int, n_actions: int, n_step: int = 3, gamma: float = 0.99,
                 eps_base: float = 0.4, eps_alpha: float = 7.0, actor_offset: int = 0, total_actors: int | None = None,
                 seed: int = 0, mode: str = "reference", clip_rewards: bool = True, episode_life: bool = True,
                 max_episode_steps: int = 50000, action_repeat: int = 4, staged: int = 0):
        super().__init__(replay, n_envs, n_actions, n_step, gamma, eps_base, eps_alpha, actor_offset, total_actors,
                         seed, mode)
        E, A, dev = self.E, self.A, self.device
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.env_state = torch.zeros(E, ENV_STATE_STRIDE, **f32)
        self.obs = torch.zeros(E, 4, 84, 84, dtype=torch.uint8, device=dev)
        # staged mode (overlapped actor/learner streams): ``staged`` sets of [E] rows +
        # slots + priorities; the learner stream applies one half while the actor fills
        # the other
        self.staged = int(staged)
        if staged:
            self.stage = [{"s_ids": torch.zeros(E, 4, **i32), "s2_ids": torch.zeros(E, 4, **i32),
                           "action": torch.zeros(E, **i32), "reward": torch.zeros(E, **f32),
                           "done": torch.zeros(E, **f32)} for _ in range(self.staged)]
            self.stage_ptrs = [{k: v.data_ptr() for k, v in t.items()} for t in self.stage]
            self.stage_nstep = [self.make_nstep(gamma, mode, sp, stage=1) for sp in self.stage_ptrs]
            self.stage_slot = [torch.zeros(E, **i32) for _ in range(self.staged)]
            self.stage_prio = [torch.zeros(E, **f32) for _ in range(self.staged)]
        self.env_params = self.hip.VecEnvParams(E, A, replay.frame_bytes, replay.frame_capacity, action_repeat,
                                                int(clip_rewards), int(episode_life), int(max_episode_steps))
        self.reset()

    def reset(self) -> None:
        self.hip.vec_env_reset(self.env_state.data_ptr(), self.seed, self.replay.frames.data_ptr(), self.env_params,
                               self.step_counter.data_ptr(), self.new_frame.data_ptr(), self.st["hist"].data_ptr(),
                               self.ep_log.data_ptr(), self._stream())

    def state_tensors(self) -> dict[str, torch.Tensor]:
        """+ the env state and the staging sets (rows, slots, priorities) that ``apply_staged`` /
        ``staged_rows`` read on a later step.  ``obs`` is rewritten by every ``observe()``."""
        out = super().state_tensors()
        out["env_state"] = self.env_state
        for i in range(self.staged):
            out[f"stage_slot[{i}]"] = self.stage_slot[i]
            out[f"stage_prio[{i}]"] = self.stage_prio[i]
            for k, v in self.stage[i].items():
                out[f"stage[{i}].{k}"] = v
        return out

    def observe(self) -> torch.Tensor:
        """Current stacked observations u8 [E,4,84,84] (gathered from the frame ring)."""
        self.replay.gather_frames(self.st["hist"], self.obs)
        return self.obs

    def act_and_step(self, q: torch.Tensor | None = None, parity: int | None = None, selected: bool = False,
                     tree: bool = True) -> None:
        """Given Q for the current observations (in ``self.q`` or ``q``), act, step the
        envs and push the emitted transitions into the replay (staged mode: into staging
        set ``parity``; :meth:`apply_staged` moves them into the replay).  ``selected``:
        ``self.actions`` already holds this step's eps-greedy actions (picked by the forward
        given :meth:`act_args`).  ``tree=False``: rows only, no priority-tree write (a central
        actor rank's local mirror: the priorities travel in its packet to rank 0's tree)."""
        if q is not None and q.data_ptr() != self.q.data_ptr():
            self.q.copy_(q)
        if not selected:
            self.select()
        self.hip.vec_env_step(self.env_state.data_ptr(), self.actions.data_ptr(), self.seed,
                              self.step_counter.data_ptr(), self.replay.frames.data_ptr(), self.env_params,
                              self.reward.data_ptr(), self.done.data_ptr(), self.new_frame.data_ptr(),
                              self.ep_log.data_ptr(), self._stream())
        if parity is not None:
            assert 0 <= parity < self.staged, "staging set out of range"
            self._emit(self.stage_nstep[parity], self.stage_slot[parity], self.stage_prio[parity], True)
            return  # the kernel advanced step_counter
        self._emit(self.nstep, self.slot, self.prio, not tree)  # (no tree: the kernel bumps)
        if tree:
            self.replay.write_batch(pre=(self.slot, self.prio, self.replay.filled), bump=self.step_counter)

    def apply_staged(self, parity: int) -> None:
        """Scatter staging set ``parity`` into the replay tables and write its
        priorities into the tree (the learner stream's half of a staged actor step)."""
        self.apply_rows(parity)
        self.apply_prios(parity)

    def apply_rows(self, parity: int) -> None:
        self.hip.apply_staged_rows(self.stage_ptrs[parity], self.replay.trans_ptrs(),
                                   self.stage_slot[parity].data_ptr(), self.stage_prio[parity].data_ptr(), self.E,
                                   self._stream())

    def apply_prios(self, parity: int) -> None:
        self.replay.write_batch(pre=self.staged_prio_write(parity))

    def staged_rows(self, parity: int) -> tuple:
        """``HBMReplay.sample_indices(rows=...)`` of staging set ``parity``."""
        return self.stage_ptrs[parity], self.stage_slot[parity], self.stage_prio[parity]

    def staged_prio_write(self, parity: int) -> tuple:
        """``HBMReplay.write_batch`` pre-write of staging set ``parity``: (slots, raw
        priorities, ``replay.filled`` advanced by E)."""
        return self.stage_slot[parity], self.stage_prio[parity], self.replay.filled

    def step(self, policy) -> None:
        """One full actor step with ``policy(obs_u8) -> Q f32 [E, A]``."""
        obs = self.observe()
        q = policy(obs)
        self.act_and_step(q)
