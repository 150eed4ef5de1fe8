"""Host models of the actor-shard kernels (``ops/csrc/actor_kernels.hip``): Philox4x32-10,
the epsilon-greedy draw, one agent step of the device game with its renderer, and the n-step
batcher with the textbook drain queue's timing.  numpy and pure Python only -- no GPU code is
imported, so the models can be checked on any machine (``test_actor_oracle_host.py``) before
the kernels are compared with them (``test_gpu_actor.py``)."""
from __future__ import annotations

from collections import deque, namedtuple

import numpy as np

M32 = 0xFFFFFFFF
f32 = np.float32


# ------------------------------------------------------------------ Philox4x32-10 (common.h)
def philox4x32_10(counter4, key2):
    """Random123 Philox4x32 with 10 rounds: 4 counter words, 2 key words -> 4 output words."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter4)
    k0, k1 = (int(k) & M32 for k in key2)
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform4(seed, stream, counter):
    """Four float32 uniforms in [0,1): counter = (counter lo, counter hi, stream lo, stream hi),
    key = (seed lo, seed hi); each word's top 24 bits times 2^-24 (exact in float32)."""
    seed, stream, counter = int(seed), int(stream), int(counter)
    r = philox4x32_10((counter, counter >> 32, stream, stream >> 32), (seed, seed >> 32))
    return tuple(f32(w >> 8) * f32(2.0 ** -24) for w in r)


# ------------------------------------------------------------------ epsilon-greedy
def select_actions_ref(q, eps, seed, counter):
    """First argmax (ties to the lower index); explore iff not (u0 > eps[e]); the random action
    is min(int(u1 * A), A - 1) with the product rounded to float32."""
    q = np.asarray(q, dtype=np.float32)
    E, A = q.shape
    out = np.zeros(E, dtype=np.int32)
    for e in range(E):
        best, bv = 0, q[e, 0]
        for a in range(1, A):
            if q[e, a] > bv:
                bv, best = q[e, a], a
        u = uniform4(seed, e, counter)
        if not (u[0] > f32(eps[e])):
            best = min(int(u[1] * f32(A)), A - 1)
        out[e] = best
    return out


# ------------------------------------------------------------------ the device game
S_PX, S_PY, S_EX, S_EY, S_EVX, S_BX, S_BY, S_BACT, S_LIVES = 0, 1, 2, 8, 14, 20, 21, 22, 23
S_T, S_EPRET, S_EPLEN, S_POINTS, S_STRIDE = 24, 25, 26, 27, 32
S_DEFINED = 28  # fields 28..31 are padding
N_ENEMIES, N_LIVES, SCREEN = 6, 3, 84
GREYS = (20, 40, 90, 110, 150, 200, 255)  # background bands, enemies (even, odd), player, bullet

# ALE full action-meaning order (18) and the minimal NOOP FIRE RIGHT LEFT RIGHTFIRE LEFTFIRE
_DX18 = (0, 0, 0, 1, -1, 0, 1, -1, 1, -1, 0, 1, -1, 0, 1, -1, 1, -1)
_DY18 = (0, 0, -1, 0, 0, 1, -1, -1, 1, 1, -1, 0, 0, 1, -1, -1, 1, 1)
_FI18 = (0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1)
_DX6 = (0, 0, 1, -1, 1, -1)
_FI6 = (0, 1, 0, 0, 1, 1)

EnvStep = namedtuple("EnvStep", "state reward done frame ep_log reset_happened")


def _clamp(x, lo, hi):
    return min(max(x, f32(lo)), f32(hi))


class VecEnvOracle:
    """One env of the device game.  All arithmetic is float32 with one rounding per operation.
    The two Philox-derived expressions, 4 + 72 u and +-(0.4 + 0.8 u), are the only ones a
    compiler may contract to an fma; ``fused`` selects that rounding for both (float64 holds
    both expressions exactly, so one rounding of the float64 value is the fma's result)."""

    def __init__(self, E, n_actions, frame_capacity, action_repeat=4, clip_rewards=1, episode_life=1,
                 max_episode_steps=0, fused=True):
        self.E, self.A, self.F = int(E), int(n_actions), int(frame_capacity)
        self.repeat, self.clip, self.life = int(action_repeat), int(clip_rewards), int(episode_life)
        self.max_steps = int(max_episode_steps)
        self.fused = bool(fused)

    # ---- Philox-derived draws
    def _mad(self, a, u, b):
        """b + a * u in float32, fused or not."""
        if self.fused:
            return f32(float(f32(b)) + float(f32(a)) * float(u))
        return f32(b) + f32(a) * u

    def spawn_x(self, u):
        return self._mad(72.0, u, 4.0)

    def spawn_vx(self, u_sign, u_speed):
        s = self._mad(0.8, u_speed, 0.4)
        return -s if u_sign < f32(0.5) else s

    def decode(self, a):
        if self.A == 18:
            return _DX18[a], _DY18[a], _FI18[a]
        k = a if a < 6 else a % 6
        return _DX6[k], 0, _FI6[k]

    def frame_slot(self, step, e, reset=False):
        """Ring slot of the frame rendered by the step (or the reset) at counter ``step``."""
        return ((int(step) + (0 if reset else 1)) * self.E + e) % self.F

    # ---- reset
    def _reset_game(self, st, e, seed, ctr):
        st[S_PX], st[S_PY] = f32(40), f32(70)
        for k in range(N_ENEMIES):
            u = uniform4(seed, e * 64 + 32 + k, ctr)
            st[S_EX + k] = self.spawn_x(u[0])
            st[S_EY + k] = f32(8 + 6 * k)
            st[S_EVX + k] = self.spawn_vx(u[1], u[2])
        st[S_BX] = st[S_BY] = st[S_BACT] = f32(0)
        st[S_LIVES] = f32(N_LIVES)
        st[S_T] = f32(0)
        st[S_POINTS] = f32(0)

    def reset(self, e, seed, ctr, state=None):
        """State row after ``vec_env_reset`` (counter word ``ctr`` = step * 16 + 1)."""
        st = np.zeros(S_STRIDE, dtype=np.float32) if state is None else np.array(state, dtype=np.float32)
        self._reset_game(st, e, seed, ctr)
        st[S_EPRET] = st[S_EPLEN] = f32(0)
        return st

    # ---- one agent step
    def step(self, state, action, e, seed, step, ep_log):
        st = np.array(state, dtype=np.float32)
        log = np.array(ep_log, dtype=np.float32)
        dx, dy, fire = self.decode(int(action))
        step = int(step)
        r_raw = f32(0)
        life_lost = game_over = False
        for f in range(self.repeat):
            if game_over:
                break
            st[S_T] += f32(1)
            st[S_PX] = _clamp(st[S_PX] + f32(dx), 0, 80)
            st[S_PY] = _clamp(st[S_PY] + f32(dy), 42, 76)
            if fire and st[S_BACT] < f32(0.5):
                st[S_BACT] = f32(1)
                st[S_BX] = st[S_PX] + f32(1.5)
                st[S_BY] = st[S_PY] - f32(2)
            descend = int(st[S_T]) % 64 == 0
            crash = False
            for k in range(N_ENEMIES):
                ex = st[S_EX + k] + st[S_EVX + k]
                if ex < f32(0) or ex > f32(78):
                    st[S_EVX + k] = -st[S_EVX + k]
                    ex = _clamp(ex, 0, 78)
                st[S_EX + k] = ex
                if descend:
                    st[S_EY + k] += f32(2)
                if (abs(ex + f32(3) - st[S_PX] - f32(2)) < f32(4.5)
                        and abs(st[S_EY + k] + f32(1.5) - st[S_PY] - f32(2)) < f32(3.5)):
                    crash = True
                if st[S_EY + k] > f32(78):
                    crash = True
            if st[S_BACT] > f32(0.5):
                st[S_BY] -= f32(3)
                hit = -1
                for k in range(N_ENEMIES):
                    if (hit < 0 and abs(st[S_EX + k] + f32(3) - st[S_BX]) < f32(3.5)
                            and abs(st[S_EY + k] + f32(1.5) - st[S_BY]) < f32(2.5)):
                        hit = k
                if hit >= 0:
                    u = uniform4(seed, e * 64 + hit, step * 16 + 2 + f)
                    r_raw += f32(20 if self.A == 18 else 1)
                    st[S_EX + hit] = self.spawn_x(u[0])
                    st[S_EY + hit] = f32(8)
                    st[S_BACT] = f32(0)
                elif st[S_BY] < f32(0):
                    st[S_BACT] = f32(0)
            if crash:
                for k in range(N_ENEMIES):
                    st[S_EY + k] = f32(8 + 6 * k)
                if self.A == 18:
                    st[S_LIVES] -= f32(1)
                    life_lost = True
                    game_over = bool(st[S_LIVES] <= f32(0))
                else:  # Pong-like: the opponent scores, the game ends at 21
                    r_raw -= f32(1)
                    st[S_POINTS] += f32(1)
                    game_over = bool(st[S_POINTS] >= f32(21))
        r = f32(np.sign(r_raw)) if self.clip else r_raw
        st[S_EPRET] += r
        st[S_EPLEN] += f32(1)
        # the time limit counts agent steps since the last agent-level done (per life with episode_life)
        time_up = self.max_steps > 0 and bool(st[S_EPLEN] >= f32(self.max_steps))
        done = game_over or time_up or bool(self.life and life_lost)
        reset_happened = False
        if done:
            log[0], log[1] = st[S_EPRET], st[S_EPLEN]
            log[2] += f32(1)
            st[S_EPRET] = st[S_EPLEN] = f32(0)
            if game_over or time_up:
                self._reset_game(st, e, seed, step * 16 + 7)
                reset_happened = True
        return EnvStep(st, r, f32(1 if done else 0), self.render(st), log, reset_happened)

    # ---- renderer: later rectangles win (player, enemies 0-5, bullet)
    @staticmethod
    def render(st):
        img = np.full((SCREEN, SCREEN), 20, dtype=np.uint8)
        img[:5] = 40
        img[80:] = 90

        def rect(y0, y1, x0, x1, v):
            y0, y1, x0, x1 = (min(max(c, 0), SCREEN) for c in (y0, y1, x0, x1))
            if y1 > y0 and x1 > x0:
                img[y0:y1, x0:x1] = v

        py, px = int(st[S_PY]), int(st[S_PX])
        rect(py, py + 4, px, px + 4, 200)
        for k in range(N_ENEMIES):
            ey, ex = int(st[S_EY + k]), int(st[S_EX + k])
            rect(ey, ey + 3, ex, ex + 6, 150 if k & 1 else 110)
        if st[S_BACT] > f32(0.5):
            by, bx = int(st[S_BY]), int(st[S_BX])
            rect(by, by + 2, bx, bx + 1, 255)
        return img


# ------------------------------------------------------------------ n-step batcher
NStepRow = namedtuple("NStepRow", "s_ids s2_ids action reward done prio bound")


class NStepOracle:
    """One env of ``nstep_emit``.  ``apex_amd.replay.nstep.BatchStorage`` decides which
    transitions exist; returns and priorities are recomputed here in float64 from the float32
    inputs (gamma rounded to float32 as the kernel holds it).  Textbook mode adds the device's
    timing: BatchStorage emits a terminal flush all at once, the kernel writes at most one row
    per env per step, so rows wait in a FIFO that gives up its oldest entry each step.  The
    oracle also advances the observation stack (``hist``): shifted by the new frame, or the
    reset frame repeated four times after ``done``.

    ``bound`` of a row is the float32 error bound of its return and priority:
    (n + 6) 2^-23 (sum gamma^i |r_i| + gamma^n |max Q| + |Q(s0, a0)| + 1e-6) -- one rounding
    per float32 operation of the kernel plus a few ulp for powf."""

    def __init__(self, n, gamma, mode, hist):
        from apex_amd.replay.nstep import BatchStorage

        self.n, self.mode = int(n), mode
        self.gamma = float(f32(gamma))
        self.bs = BatchStorage(self.n, self.gamma, mode=mode)
        self.hist = tuple(int(h) for h in hist)
        self.pending = deque()
        self.rows = []          # every row BatchStorage produced, in its order
        self.stale_q = 0        # reference mode: emissions whose Q(s0) predates the episode (Q3)
        self.first_step_terminal = 0   # reference mode: done with an empty window (Q4)

    def _ret(self, rewards):
        R = absR = 0.0
        for i, r in enumerate(rewards):
            R += self.gamma ** i * float(r)
            absR += self.gamma ** i * abs(float(r))
        return R, absR

    def _row(self, k, rewards, q_next):
        bs, n = self.bs, self.n
        R, absR = self._ret(rewards)
        d = float(bs.dones[k])
        q0a = float(bs.q_values[k][bs.actions[k]])
        boot = self.gamma ** n * float(np.max(q_next)) * (1.0 - d)
        prio = abs(R + boot - q0a) + 1e-6
        bound = (n + 6) * 2.0 ** -23 * (absR + abs(boot) + abs(q0a) + 1e-6)
        return NStepRow(tuple(bs.states[k]), tuple(bs.next_states[k]), int(bs.actions[k]), R, d, prio, bound)

    def add(self, action, reward, done, q, new_frame):
        """Feed one agent step taken from the current ``hist``; returns the row the device
        writes this step, or None."""
        bs, n = self.bs, self.n
        q = np.array(q, dtype=np.float32)
        win_r = [float(r) for r in bs.reward_deque]
        k0 = len(bs)
        if self.mode == "reference":
            if done and not bs.state_deque:
                self.first_step_terminal += 1
            elif done and len(bs.q_values_deque) > len(bs.state_deque):
                self.stale_q += 1  # the Q window's head is still a row of the previous episode
        bs.add(self.hist, float(reward), int(action), bool(done), q)
        new = []
        if self.mode == "reference":
            if len(bs) > k0:
                new.append(self._row(k0, win_r + [float(reward)], q))
        else:
            k = k0
            if len(win_r) == n:  # the regular emission, bootstrapped from Q(s_t)
                new.append(self._row(k, win_r, q))
                win_r = win_r[1:]
                k += 1
            if done:
                rs = win_r + [float(reward)]
                for j in range(len(rs)):
                    new.append(self._row(k + j, rs[j:], np.zeros_like(q)))
        assert len(new) == len(bs) - k0
        self.rows.extend(new)
        self.pending.extend(new)
        out = None
        if self.mode == "reference":
            out = self.pending.popleft() if self.pending else None
            assert not self.pending
        elif self.pending:
            out = self.pending.popleft()
        f = int(new_frame)
        self.hist = (f, f, f, f) if done else self.hist[1:] + (f,)
        return out
