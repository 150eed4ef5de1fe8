// Device bodies of the synthetic vector Atari env, shared by the stepwise kernels
// (actor_kernels.hip: vec_env_reset_k / vec_env_step_k) and the one-launch greedy rollout
// (atari_rollout_kernels.hip), so both step bit for bit alike -- the way aql_dev.h and
// classic_dynamics are shared by their stepwise and rollout kernels.
#pragma once
#include "common.h"
#include "kernels.h"

namespace apex {

// ------------------------------------------------------------------ env state layout
enum : int {
  S_PX = 0, S_PY = 1, S_EX = 2, S_EY = 8, S_EVX = 14, S_BX = 20, S_BY = 21, S_BACT = 22, S_LIVES = 23,
  S_T = 24, S_EPRET = 25, S_EPLEN = 26, S_POINTS = 27, S_STRIDE = 32
};
constexpr int kEnemies = 6;
constexpr int kLives = 3;
constexpr int kScreen = 84;

// action -> (dx, dy, fire) using the ALE full action-meaning order
// NOOP FIRE UP RIGHT LEFT DOWN UPRIGHT UPLEFT DOWNRIGHT DOWNLEFT UPFIRE RIGHTFIRE LEFTFIRE
// DOWNFIRE UPRIGHTFIRE UPLEFTFIRE DOWNRIGHTFIRE DOWNLEFTFIRE; minimal sets (Pong: 6) map
// onto NOOP FIRE RIGHT LEFT RIGHTFIRE LEFTFIRE.
__device__ __forceinline__ void decode_action(int a, int n_actions, int& dx, int& dy, int& fire) {
  if (n_actions == 18) {
    const signed char DX[18] = {0, 0, 0, 1, -1, 0, 1, -1, 1, -1, 0, 1, -1, 0, 1, -1, 1, -1};
    const signed char DY[18] = {0, 0, -1, 0, 0, 1, -1, -1, 1, 1, -1, 0, 0, 1, -1, -1, 1, 1};
    const signed char FI[18] = {0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1};
    dx = DX[a]; dy = DY[a]; fire = FI[a];
  } else {
    const signed char DX[6] = {0, 0, 1, -1, 1, -1};
    const signed char FI[6] = {0, 1, 0, 0, 1, 1};
    const int k = a < 6 ? a : a % 6;
    dx = DX[k]; dy = 0; fire = FI[k];
  }
}

__device__ __forceinline__ void env_reset_state(float* st, uint64_t seed, int e, uint64_t ctr) {
  float u[4];
  st[S_PX] = 40.f;
  st[S_PY] = 70.f;
#pragma unroll
  for (int k = 0; k < kEnemies; ++k) {
    uniform4(seed, (uint64_t)e * 64 + 32 + k, ctr, u);
    st[S_EX + k] = 4.f + 72.f * u[0];
    st[S_EY + k] = 8.f + 6.f * k;
    st[S_EVX + k] = (u[1] < 0.5f ? -1.f : 1.f) * (0.4f + 0.8f * u[2]);
  }
  st[S_BX] = 0.f; st[S_BY] = 0.f; st[S_BACT] = 0.f;
  st[S_LIVES] = (float)kLives;
  st[S_T] = 0.f;
  st[S_POINTS] = 0.f;
}

// One workgroup renders one env's 84x84 frame (thread 0 has already updated the state) into
// `dst` and, when given, into a second image `dst2` (the rollout's LDS copy of the frame).
__device__ __forceinline__ void render_frame(const float* st, uint8_t* dst, uint32_t* dst2 = nullptr) {
  __shared__ int rect[(kEnemies + 2) * 4];
  __shared__ int val[kEnemies + 2];
  if (threadIdx.x == 0) {
    rect[0] = (int)st[S_PY]; rect[1] = (int)st[S_PY] + 4; rect[2] = (int)st[S_PX]; rect[3] = (int)st[S_PX] + 4;
    val[0] = 200;
    for (int k = 0; k < kEnemies; ++k) {
      rect[4 + 4 * k] = (int)st[S_EY + k]; rect[5 + 4 * k] = (int)st[S_EY + k] + 3;
      rect[6 + 4 * k] = (int)st[S_EX + k]; rect[7 + 4 * k] = (int)st[S_EX + k] + 6;
      val[1 + k] = (k & 1) ? 150 : 110;
    }
    const int ba = st[S_BACT] > 0.5f;
    rect[4 + 4 * kEnemies] = ba ? (int)st[S_BY] : -10; rect[5 + 4 * kEnemies] = ba ? (int)st[S_BY] + 2 : -10;
    rect[6 + 4 * kEnemies] = (int)st[S_BX]; rect[7 + 4 * kEnemies] = (int)st[S_BX] + 1;
    val[1 + kEnemies] = 255;
  }
  __syncthreads();
  uint32_t* out = reinterpret_cast<uint32_t*>(dst);
  for (int w = threadIdx.x; w < kScreen * kScreen / 4; w += blockDim.x) {
    const int y = (w * 4) / kScreen, x0 = (w * 4) % kScreen;
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j;
      int v = y < 5 ? 40 : (y >= 80 ? 90 : 20);
#pragma unroll
      for (int r = 0; r < kEnemies + 2; ++r)
        if (y >= rect[4 * r] && y < rect[4 * r + 1] && x >= rect[4 * r + 2] && x < rect[4 * r + 3]) v = val[r];
      packed |= (uint32_t)v << (8 * j);
    }
    out[w] = packed;
    if (dst2) dst2[w] = packed;
  }
}

// What one agent step leaves besides the new state.
struct EnvStepOut {
  float reward;
  bool done;       // agent-level terminal
  float ep_ret, ep_len;  // the finished episode's return / length (valid when done)
};

// One agent step of env `e` on a register copy `st` of its state row (every index is a
// compile-time constant after unrolling) = action_repeat emulator frames (MaxAndSkipEnv
// semantics: rewards summed, stop at game over).  episode_life: a lost life is an agent-level
// terminal but the game continues (EpisodicLifeEnv); game over / time limit reset the game.
// Philox words: (step * 16 + 2 + f) for the respawn of emulator frame f, step * 16 + 7 for the reset.
__device__ __forceinline__ EnvStepOut env_step_state(float (&st)[S_STRIDE], int action, uint64_t seed, int e,
                                                     int64_t step, const VecEnvParams& p) {
  int dx, dy, fire;
  decode_action(action, p.n_actions, dx, dy, fire);
  float r_raw = 0.f;
  bool life_lost = false, game_over = false;
  for (int f = 0; f < p.action_repeat && !game_over; ++f) {
    st[S_T] += 1.f;
    st[S_PX] = fminf(fmaxf(st[S_PX] + dx, 0.f), 80.f);
    st[S_PY] = fminf(fmaxf(st[S_PY] + dy, 42.f), 76.f);
    if (fire && st[S_BACT] < 0.5f) { st[S_BACT] = 1.f; st[S_BX] = st[S_PX] + 1.5f; st[S_BY] = st[S_PY] - 2.f; }
    const bool descend = ((int)st[S_T] % 64) == 0;
    bool crash = false;
#pragma unroll
    for (int k = 0; k < kEnemies; ++k) {
      float ex = st[S_EX + k] + st[S_EVX + k];
      if (ex < 0.f || ex > 78.f) { st[S_EVX + k] = -st[S_EVX + k]; ex = fminf(fmaxf(ex, 0.f), 78.f); }
      st[S_EX + k] = ex;
      if (descend) st[S_EY + k] += 2.f;
      if (fabsf(ex + 3.f - st[S_PX] - 2.f) < 4.5f && fabsf(st[S_EY + k] + 1.5f - st[S_PY] - 2.f) < 3.5f) crash = true;
      if (st[S_EY + k] > 78.f) crash = true;
    }
    if (st[S_BACT] > 0.5f) {
      st[S_BY] -= 3.f;
      int hit = -1;
#pragma unroll
      for (int k = 0; k < kEnemies; ++k)
        if (hit < 0 && fabsf(st[S_EX + k] + 3.f - st[S_BX]) < 3.5f && fabsf(st[S_EY + k] + 1.5f - st[S_BY]) < 2.5f)
          hit = k;
      if (hit >= 0) {
        float u[4];
        uniform4(seed, (uint64_t)e * 64 + hit, (uint64_t)step * 16 + 2 + f, u);
        r_raw += (p.n_actions == 18) ? 20.f : 1.f;
#pragma unroll
        for (int k = 0; k < kEnemies; ++k)
          if (k == hit) {  // register-resident: no dynamic index
            st[S_EX + k] = 4.f + 72.f * u[0];
            st[S_EY + k] = 8.f;
          }
        st[S_BACT] = 0.f;
      } else if (st[S_BY] < 0.f) {
        st[S_BACT] = 0.f;
      }
    }
    if (crash) {
#pragma unroll
      for (int k = 0; k < kEnemies; ++k) st[S_EY + k] = 8.f + 6.f * k;
      if (p.n_actions == 18) {
        st[S_LIVES] -= 1.f;
        life_lost = true;
        game_over = st[S_LIVES] <= 0.f;
      } else {  // Pong-like: opponent scores, game ends at 21
        r_raw -= 1.f;
        st[S_POINTS] += 1.f;
        game_over = st[S_POINTS] >= 21.f;
      }
    }
  }
  const float r = p.clip_rewards ? (r_raw > 0.f ? 1.f : (r_raw < 0.f ? -1.f : 0.f)) : r_raw;
  st[S_EPRET] += r;
  st[S_EPLEN] += 1.f;
  // S_EPLEN counts agent steps since the last agent-level done: with episode_life, per life
  const bool time_up = p.max_episode_steps > 0 && st[S_EPLEN] >= (float)p.max_episode_steps;
  EnvStepOut o;
  o.reward = r;
  o.done = game_over || time_up || (p.episode_life && life_lost);
  o.ep_ret = st[S_EPRET];
  o.ep_len = st[S_EPLEN];
  if (o.done) {
    st[S_EPRET] = 0.f;
    st[S_EPLEN] = 0.f;
    if (game_over || time_up) env_reset_state(st, seed, e, (uint64_t)step * 16 + 7);
  }
  return o;
}

}  // namespace apex
