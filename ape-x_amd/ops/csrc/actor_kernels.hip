// Actor-shard kernels for gfx950: vectorised synthetic Atari env, on-device
// epsilon-greedy, and the n-step batcher with actor-computed priorities
// (reference memory.py:393-478, origin_repo/actor.py:52-115).
//
// The reference runs one env + one B=1 CPU forward per actor process and ships
// pickled 50-transition chunks over TCP.  Here an actor shard is E envs on one GPU:
// the env renders 84x84 u8 frames straight into the HBM frame ring, the Q-network
// runs once for all E envs, actions are drawn on device with a per-env epsilon, and
// the n-step kernel writes transitions + initial priorities directly into the replay
// (slot = (step*E + e) mod C, so a transition's lifetime is exactly C/E steps and the
// frame ring (F >= C + (2n+8)E) always outlives the transitions that reference it).
#include "atari_env_dev.h"
#include "common.h"
#include "kernels.h"

namespace apex {

// env state layout, decode_action, env_reset_state, render_frame, env_step_state: atari_env_dev.h

__global__ void vec_env_reset_k(float* state, uint64_t seed, uint8_t* frames, VecEnvParams p,
                                const int64_t* step_counter, int* new_frame, int* hist, float* ep_log) {
  const int e = blockIdx.x;
  float* st = state + (size_t)e * S_STRIDE;
  const int64_t step = step_counter ? step_counter[0] : 0;
  const int slot = (int)(((int64_t)step * p.E + e) % p.F);
  if (threadIdx.x == 0) {
    env_reset_state(st, seed, e, (uint64_t)step * 16 + 1);
    st[S_EPRET] = 0.f; st[S_EPLEN] = 0.f;
    new_frame[e] = slot;
    if (hist) for (int c = 0; c < 4; ++c) hist[e * 4 + c] = slot;
    if (ep_log) for (int c = 0; c < 4; ++c) ep_log[e * 4 + c] = 0.f;
  }
  __syncthreads();
  render_frame(st, frames + (size_t)slot * p.frame_bytes);
}

// One agent step = action_repeat emulator frames (MaxAndSkipEnv semantics: rewards
// summed, stop at game over).  episode_life: a lost life is an agent-level terminal
// but the game continues (EpisodicLifeEnv); game over / time limit reset the game.
__global__ void vec_env_step_k(float* state, const int* __restrict__ actions, uint64_t seed,
                               const int64_t* step_counter, uint8_t* frames, VecEnvParams p,
                               float* reward, float* done, int* new_frame, float* ep_log) {
  const int e = blockIdx.x;
  float* gst = state + (size_t)e * S_STRIDE;
  __shared__ float sst[S_STRIDE];
  const int64_t step = step_counter ? step_counter[0] : 0;
  const int slot = (int)(((int64_t)(step + 1) * p.E + e) % p.F);
  if (threadIdx.x == 0) {
    // the serial game logic runs on a register copy of the state (every index below is
    // a compile-time constant after unrolling): on the global copy each of its ~150
    // dependent accesses was an L2 round trip (17 us per step for 256 envs)
    float st[S_STRIDE];
#pragma unroll
    for (int i = 0; i < S_STRIDE; ++i) st[i] = gst[i];
    const EnvStepOut o = env_step_state(st, actions[e], seed, e, step, p);
    reward[e] = o.reward;
    done[e] = o.done ? 1.f : 0.f;
    if (o.done && ep_log) {
      ep_log[e * 4 + 0] = o.ep_ret;
      ep_log[e * 4 + 1] = o.ep_len;
      ep_log[e * 4 + 2] += 1.f;
    }
    new_frame[e] = slot;
#pragma unroll
    for (int i = 0; i < S_STRIDE; ++i) {
      gst[i] = st[i];
      sst[i] = st[i];
    }
  }
  __syncthreads();
  render_frame(sst, frames + (size_t)slot * p.frame_bytes);
}

// ------------------------------------------------------------------ epsilon-greedy
__global__ void select_actions_k(const float* __restrict__ q, int E, int A, const float* __restrict__ eps,
                                 uint64_t seed, const int64_t* counter, int* __restrict__ actions) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const float* row = q + (size_t)e * A;
  int best = 0;
  float bv = row[0];
  for (int a = 1; a < A; ++a)
    if (row[a] > bv) { bv = row[a]; best = a; }
  float u[4];
  uniform4(seed, (uint64_t)e, counter ? (uint64_t)counter[0] : 0ull, u);
  if (!(u[0] > eps[e])) {
    int r = (int)(u[1] * (float)A);
    best = r < A ? r : A - 1;
  }
  actions[e] = best;
}

// ------------------------------------------------------------------ n-step batcher
__device__ __forceinline__ void nstep_one(const NStepParams& p, const NStepState& st, const TransTable& tt,
                                          const float* __restrict__ q, const int* __restrict__ actions,
                                          const float* __restrict__ reward, const float* __restrict__ done,
                                          const int* __restrict__ new_frame, int64_t step, int e,
                                          int* __restrict__ slot_out, float* __restrict__ prio_out);

__global__ void nstep_emit_k(NStepParams p, NStepState st, TransTable tt, const float* __restrict__ q,
                             const int* __restrict__ actions, const float* __restrict__ reward,
                             const float* __restrict__ done, const int* __restrict__ new_frame,
                             int64_t* step_counter, int* __restrict__ slot_out,
                             float* __restrict__ prio_out, int bump) {
  const int64_t step = step_counter ? step_counter[0] : 0;
  if (bump) {
    // one workgroup strides over all envs, then advances the step counter once every
    // thread has read it (replaces a separate +1 launch on the actor stream)
    for (int e = threadIdx.x; e < p.E; e += blockDim.x) nstep_one(p, st, tt, q, actions, reward, done, new_frame,
                                                                  step, e, slot_out, prio_out);
    __syncthreads();
    if (threadIdx.x == 0) step_counter[0] = step + 1;
    return;
  }
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < p.E) nstep_one(p, st, tt, q, actions, reward, done, new_frame, step, e, slot_out, prio_out);
}

__device__ __forceinline__ void nstep_one(const NStepParams& p, const NStepState& st, const TransTable& tt,
                                          const float* __restrict__ q, const int* __restrict__ actions,
                                          const float* __restrict__ reward, const float* __restrict__ done,
                                          const int* __restrict__ new_frame, int64_t step, int e,
                                          int* __restrict__ slot_out, float* __restrict__ prio_out) {
  const int n = p.n, A = p.A;
  const int slot = (int)(((int64_t)step * p.E + e) % p.C);
  const int row = p.stage ? e : slot;  // staged: the learner scatters the row later
  int* meta = st.win_meta + e * 4;
  int start = meta[0], len = meta[1], qstart = meta[2], qlen = meta[3];
  int* hist = st.hist + e * 4;
  const float* qt = q + (size_t)e * A;
  const int at = actions[e];
  const float rt = reward[e];
  const bool dt = done[e] > 0.5f;
  const float gn = powf(p.gamma, (float)n);
  float qmax = qt[0];
  for (int a = 1; a < A; ++a) qmax = fmaxf(qmax, qt[a]);

  bool emitted = false;
  float prio = 0.f;
  auto write_trans = [&](const int* s0, int a0, float R, float d) {
    for (int c = 0; c < 4; ++c) {
      tt.s_ids[row * 4 + c] = s0[c];
      tt.s2_ids[row * 4 + c] = hist[c];
    }
    tt.action[row] = a0;
    tt.reward[row] = R;
    tt.done[row] = d;
  };

  if (p.mode == 0) {
    // ---- reference semantics (memory.py:415-440)
    if ((len == n || dt) && len > 0) {
      float R = 0.f, g = 1.f;
      for (int i = 0; i < len; ++i) { R += g * st.win_r[e * n + (start + i) % n]; g *= p.gamma; }
      R += g * rt;
      const int k0 = start;
      const int a0 = st.win_a[e * n + k0];
      const float q0a = st.win_q[((size_t)e * n + qstart) * A + a0];
      const float target = R + gn * qmax * (dt ? 0.f : 1.f);
      prio = fabsf(target - q0a) + 1e-6f;
      write_trans(st.win_ids + (e * n + k0) * 4, a0, R, dt ? 1.f : 0.f);
      emitted = true;
    }
    if (dt) {
      len = 0;  // state/action/reward deques cleared; the Q deque is not
    } else {
      int pos;
      if (len < n) { pos = (start + len) % n; ++len; } else { pos = start; start = (start + 1) % n; }
      for (int c = 0; c < 4; ++c) st.win_ids[(e * n + pos) * 4 + c] = hist[c];
      st.win_a[e * n + pos] = at;
      st.win_r[e * n + pos] = rt;
      int qpos;
      if (qlen < n) { qpos = (qstart + qlen) % n; ++qlen; } else { qpos = qstart; qstart = (qstart + 1) % n; }
      for (int a = 0; a < A; ++a) st.win_q[((size_t)e * n + qpos) * A + a] = qt[a];
    }
  } else {
    // ---- textbook n-step: R = sum_{i<n} gamma^i r, bootstrap gamma^n max Q(s_t)
    if (len == n) {
      float R = 0.f, g = 1.f;
      for (int i = 0; i < n; ++i) { R += g * st.win_r[e * n + (start + i) % n]; g *= p.gamma; }
      const int a0 = st.win_a[e * n + start];
      const float q0a = st.win_q[((size_t)e * n + start) * A + a0];
      prio = fabsf(R + gn * qmax - q0a) + 1e-6f;
      write_trans(st.win_ids + (e * n + start) * 4, a0, R, 0.f);
      emitted = true;
      start = (start + 1) % n;
      --len;
    }
    {  // push (s_t, a_t, r_t, Q(s_t))
      const int pos = (start + len) % n;
      ++len;
      for (int c = 0; c < 4; ++c) st.win_ids[(e * n + pos) * 4 + c] = hist[c];
      st.win_a[e * n + pos] = at;
      st.win_r[e * n + pos] = rt;
      for (int a = 0; a < A; ++a) st.win_q[((size_t)e * n + pos) * A + a] = qt[a];
    }
    // The drain queue is a ring of n rows (dmeta = head, count).  Every step adds one (s,a)
    // and emits at most one row, and emits nothing only while count == 0 and len < n, so
    // len + count <= n always holds: the n entries hold a flushed window behind the rows an
    // earlier episode still has pending (appended, not overwritten), and nothing is dropped.
    int* dmeta = st.drain_meta + e * 2;
    int dhead = dmeta[0], dcnt = dmeta[1];
    if (!emitted && dcnt > 0) {  // the oldest pending row goes first
      for (int c = 0; c < 4; ++c) {
        tt.s_ids[row * 4 + c] = st.drain_ids[(e * n + dhead) * 4 + c];
        tt.s2_ids[row * 4 + c] = st.drain_s2[e * 4 + c];
      }
      tt.action[row] = st.drain_a[e * n + dhead];
      tt.reward[row] = st.drain_r[e * n + dhead];
      tt.done[row] = 1.f;
      prio = st.drain_q[e * n + dhead];
      emitted = true;
      dhead = (dhead + 1) % n;
      --dcnt;
    }
    if (dt) {
      // flush the window as terminal transitions: one now (if the slot is free), the
      // rest appended to the drain queue, one emitted per following step.  drain_s2 stays
      // one row per env: every drained row has done = 1, so its next state is never
      // bootstrapped from and rows of an older episode may take the newer one's.
      for (int j = 0; j < len; ++j) {
        float R = 0.f, g = 1.f;
        for (int i = j; i < len; ++i) { R += g * st.win_r[e * n + (start + i) % n]; g *= p.gamma; }
        const int k = (start + j) % n;
        const int a0 = st.win_a[e * n + k];
        const float pr = fabsf(R - st.win_q[((size_t)e * n + k) * A + a0]) + 1e-6f;
        if (!emitted) {
          write_trans(st.win_ids + (e * n + k) * 4, a0, R, 1.f);
          prio = pr;
          emitted = true;
        } else if (dcnt < n) {  // always true (see above); keeps the ring in bounds regardless
          const int dl = (dhead + dcnt) % n;
          for (int c = 0; c < 4; ++c) st.drain_ids[(e * n + dl) * 4 + c] = st.win_ids[(e * n + k) * 4 + c];
          st.drain_a[e * n + dl] = a0;
          st.drain_r[e * n + dl] = R;
          st.drain_q[e * n + dl] = pr;
          ++dcnt;
        }
      }
      for (int c = 0; c < 4; ++c) st.drain_s2[e * 4 + c] = hist[c];
      len = 0;
      start = 0;
    }
    dmeta[0] = dhead;
    dmeta[1] = dcnt;
    qstart = start;
    qlen = len;
  }
  meta[0] = start; meta[1] = len; meta[2] = qstart; meta[3] = qlen;
  // advance the observation stack (FrameStack: the reset frame is repeated k times)
  const int f = new_frame[e];
  if (dt) {
    for (int c = 0; c < 4; ++c) hist[c] = f;
  } else {
    hist[0] = hist[1]; hist[1] = hist[2]; hist[2] = hist[3]; hist[3] = f;
  }
  slot_out[e] = slot;
  prio_out[e] = emitted ? prio : 0.f;
}

// staged rows -> replay tables (overlapped actor/learner: the learner stream applies the
// previous actor step's rows right before its tree write, so a row is never rewritten
// while the learner can still sample its slot)
__global__ void apply_staged_rows_k(TransTable st, TransTable dst, const int* __restrict__ slot,
                                    const float* __restrict__ prio, int E) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E || !(prio[e] > 0.f)) return;
  const int j = slot[e];
  reinterpret_cast<int4*>(dst.s_ids)[j] = reinterpret_cast<const int4*>(st.s_ids)[e];
  reinterpret_cast<int4*>(dst.s2_ids)[j] = reinterpret_cast<const int4*>(st.s2_ids)[e];
  dst.action[j] = st.action[e];
  dst.reward[j] = st.reward[e];
  dst.done[j] = st.done[e];
}

// evaluator envs (no n-step batcher): advance each env's observation stack and the step
// counter that seeds the env / action draws (lane 0 of block 0)
__global__ void frame_hist_step_k(int* __restrict__ hist, const int* __restrict__ new_frame,
                                  const float* __restrict__ done, int E, int64_t* counter) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e == 0 && counter) counter[0] += 1;
  if (e >= E) return;
  const int f = new_frame[e];
  int* h = hist + e * 4;
  if (done[e] > 0.f) {
    h[0] = h[1] = h[2] = h[3] = f;
  } else {
    h[0] = h[1]; h[1] = h[2]; h[2] = h[3]; h[3] = f;
  }
}

// ------------------------------------------------------------------ launchers
void frame_hist_step(int* hist, const int* new_frame, const float* done, int E, int64_t* counter, hipStream_t s) {
  if (E <= 0) return;
  frame_hist_step_k<<<(E + 255) / 256, 256, 0, s>>>(hist, new_frame, done, E, counter);
  LAUNCH_CHECK();
}

void vec_env_reset(float* state, uint64_t seed, uint8_t* frames, const VecEnvParams& p,
                   const int64_t* step_counter, int* new_frame, int* hist, float* ep_log, hipStream_t s) {
  if (p.frame_bytes != kScreen * kScreen) throw std::invalid_argument("vec env renders 84x84 frames");
  vec_env_reset_k<<<p.E, 256, 0, s>>>(state, seed, frames, p, step_counter, new_frame, hist, ep_log);
  LAUNCH_CHECK();
}

void vec_env_step(float* state, const int* actions, uint64_t seed, const int64_t* step_counter, uint8_t* frames,
                  const VecEnvParams& p, float* reward, float* done, int* new_frame, float* ep_log, hipStream_t s) {
  if (p.frame_bytes != kScreen * kScreen) throw std::invalid_argument("vec env renders 84x84 frames");
  if (p.n_actions != 18 && p.n_actions > 6) throw std::invalid_argument("vec env supports 18 or <=6 actions");
  vec_env_step_k<<<p.E, 256, 0, s>>>(state, actions, seed, step_counter, frames, p, reward, done, new_frame, ep_log);
  LAUNCH_CHECK();
}

void select_actions(const float* q, int E, int A, const float* eps, uint64_t seed, const int64_t* counter,
                    int* actions, hipStream_t s) {
  select_actions_k<<<(E + 255) / 256, 256, 0, s>>>(q, E, A, eps, seed, counter, actions);
  LAUNCH_CHECK();
}

void nstep_emit(const NStepParams& p, NStepState st, TransTable tt, const float* q, const int* actions,
                const float* reward, const float* done, const int* new_frame, int64_t* step_counter,
                int* slot_out, float* prio_out, hipStream_t s, bool bump) {
  if (p.n < 1 || p.n > 16) throw std::invalid_argument("n-step must be in [1, 16]");
  if (bump && !step_counter) throw std::invalid_argument("nstep_emit: bump needs a step counter");
  if (bump) {  // one workgroup (see nstep_emit_k)
    const int threads = std::min(1024, std::max(64, (p.E + 63) / 64 * 64));
    nstep_emit_k<<<1, threads, 0, s>>>(p, st, tt, q, actions, reward, done, new_frame, step_counter, slot_out,
                                       prio_out, 1);
  } else {
    nstep_emit_k<<<(p.E + 127) / 128, 128, 0, s>>>(p, st, tt, q, actions, reward, done, new_frame, step_counter,
                                                   slot_out, prio_out, 0);
  }
  LAUNCH_CHECK();
}

void apply_staged_rows(TransTable stage, TransTable dst, const int* slot, const float* prio, int E, hipStream_t s) {
  if (E <= 0) return;
  apply_staged_rows_k<<<(E + 255) / 256, 256, 0, s>>>(stage, dst, slot, prio, E);
  LAUNCH_CHECK();
}

}  // namespace apex
