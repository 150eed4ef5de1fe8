// Vector-observation Ape-X kernels for gfx950: classic-control envs that write their
// observations into the HBM frame ring, the acting forward of the MLP dueling net with the
// epsilon-greedy draw, and the learner's fused forward x3 / loss / backward (reference
// ApeX.py, DQN.py with model.py's MLP DuelingDQN: features.0 = Linear(obs, 128), two
// 128-hidden heads).
//
// A vector observation is a "frame" of 4 * obs bytes in the replay's frame ring, so the n-step
// batcher, the PER tree, the priority mix, the grad norm and the optimizer are the existing
// kernels, unchanged.  Everything is fp32 FMA: the net is ~34k MAC per sample, the work is
// latency-bound, and the design goal is few launches and no host sync.
//
//   vec_classic_reset / vec_classic_step  one thread per env (CartPole, MountainCar dynamics of
//                                         envs/classic.py in fp32)
//   vec_act      one workgroup per 8 envs: both heads' 128x128 weights staged (transposed) in LDS,
//                Q[E, A], then select_actions_k's draw in the same launch
//   vec_host_eval_act  vec_act for the host-env evaluator: the observations straight from the staging
//                block's reset_obs rows, the step by value, epsilon 0 (engine/vector_host_eval.py)
//   dqn_frame    one workgroup, <= 8 envs: the actor side of one DQN.py frame (eps(t) / beta(t), vec_act's
//                forward and draw on the online net, the env step, the FrameStack advance, the replay
//                insert at the running max priority and its tree walk) in one launch (engine/dqn.py)
//   vec_rollout  one workgroup per 8 greedy episodes, reset to first done in one launch: heads staged
//                once, then forward / first argmax / env dynamics per step, no ring and no host
//   vec_learn    one workgroup per 4 sampled rows: target net on (s, s'), online net on (s, s'),
//                double-DQN n-step Huber loss, backward to per-sample vectors (aql_learn_bwd's
//                shape); block 0 also writes the next step's PER beta
//   vec_grad     batch contraction of the per-sample vectors into the flat gradient, one element
//                per thread, summed in batch order (no atomics: deterministic) + one fp64
//                sum-of-squares partial per workgroup in grad_sumsq's format
#include "common.h"
#include "kernels.h"
#include "tree_dev.h"

namespace apex {

namespace {

constexpr int kH = kVecHidden;         // 128
constexpr int kRows = 8;                // rows per forward pass of a workgroup
constexpr int kWPitch = kH + 1;         // transposed weight image [k][j], padded: conflict-free both ways
constexpr int kWHead = kH * kWPitch;    // floats per head image
constexpr int kThreads = 256;

// ------------------------------------------------------------------ envs
// the reset observation of env e at Philox counter ctr (CartPole: 4 floats; MountainCar: 2 + zeros)
__device__ __forceinline__ void classic_reset_obs(int kind, uint64_t seed, int e, uint64_t ctr, float* st) {
  float u[4];
  uniform4(seed, (uint64_t)e, ctr, u);
  if (kind == 0) {  // CartPole: U(-0.05, 0.05)^4
#pragma unroll
    for (int k = 0; k < 4; ++k) st[k] = -0.05f + 0.1f * u[k];
  } else {          // MountainCar: position U(-0.6, -0.4), velocity 0
    st[0] = -0.6f + 0.2f * u[0];
    st[1] = 0.f;
    st[2] = 0.f;
    st[3] = 0.f;
  }
}

// one step of env `kind` from state s with action a: next state nv[4] (MountainCar: 2 + zeros),
// reward, terminal.  Shared by vec_classic_step_k and vec_rollout_k, so both step bit for bit alike.
__device__ __forceinline__ void classic_dynamics(int kind, const float* s, int a, float* nv, float& r, bool& term) {
  if (kind == 0) {  // CartPole (Barto et al. 1983; envs/classic.py CartPoleEnv, as aql_env_step)
    const float x = s[0], xd = s[1], th = s[2], thd = s[3];
    const float force = (a == 1) ? 10.f : -10.f;
    const float ct = cosf(th), sn = sinf(th);
    const float tmp = (force + 0.05f * thd * thd * sn) / 1.1f;
    const float tha = (9.8f * sn - ct * tmp) / (0.5f * (4.f / 3.f - 0.1f * ct * ct / 1.1f));
    const float xa = tmp - 0.05f * tha * ct / 1.1f;
    nv[0] = x + 0.02f * xd;
    nv[1] = xd + 0.02f * xa;
    nv[2] = th + 0.02f * thd;
    nv[3] = thd + 0.02f * tha;
    r = 1.f;
    term = nv[0] < -2.4f || nv[0] > 2.4f || nv[2] < -0.20943951f || nv[2] > 0.20943951f;
  } else {          // MountainCar (Moore 1990; envs/classic.py MountainCarEnv)
    float pos = s[0], v = s[1];
    v += (float)(a - 1) * 0.001f + cosf(3.f * pos) * (-0.0025f);
    v = fminf(fmaxf(v, -0.07f), 0.07f);
    pos += v;
    pos = fminf(fmaxf(pos, -1.2f), 0.6f);
    if (pos == -1.2f && v < 0.f) v = 0.f;  // inelastic left wall
    nv[0] = pos;
    nv[1] = v;
    nv[2] = 0.f;
    nv[3] = 0.f;
    r = -1.f;
    term = pos >= 0.5f;
  }
}

__global__ void vec_classic_reset_k(VecEnv V, const int64_t* step_counter, int* new_frame, int* hist,
                                    float* ep_log) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= V.E) return;
  const int64_t step = step_counter ? step_counter[0] : 0;
  const int slot = (int)(((int64_t)step * V.E + e) % V.F);
  float* gst = V.state + (size_t)e * vecs::STRIDE;
  float st[4];
  classic_reset_obs(V.kind, V.seed, e, (uint64_t)step * 16 + 1, st);
  for (int k = 0; k < vecs::STRIDE; ++k) gst[k] = k < 4 ? st[k] : 0.f;
  for (int k = 0; k < V.obs; ++k) V.ring[(size_t)slot * V.obs + k] = st[k];
  new_frame[e] = slot;
  if (hist) for (int c = 0; c < 4; ++c) hist[e * 4 + c] = slot;
  if (ep_log) for (int c = 0; c < 4; ++c) ep_log[e * 4 + c] = 0.f;
}

// Env e's step at counter `step` with action a: dynamics, TimeLimit, episode log, the reset draw
// on done, the new observation into its ring row.  Shared by vec_classic_step_k and dqn_frame_k,
// so both step bit for bit alike.
__device__ __forceinline__ void classic_env_step(const VecEnv& V, int e, int64_t step, int a, float* reward,
                                                 float* done, int* new_frame, float* ep_log) {
  const int slot = (int)(((int64_t)(step + 1) * V.E + e) % V.F);
  float* gst = V.state + (size_t)e * vecs::STRIDE;
  float nv[4];
  float r;
  bool term;
  classic_dynamics(V.kind, gst, a, nv, r, term);
  const float ep_ret = gst[vecs::EPRET] + r;
  const float ep_len = gst[vecs::EPLEN] + 1.f;
  const bool time_up = V.max_steps > 0 && ep_len >= (float)V.max_steps;  // TimeLimit ends with done = 1
  const bool d = term || time_up;
  reward[e] = r;
  done[e] = d ? 1.f : 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) gst[vecs::LAST + k] = nv[k];  // the step's own s' (before a reset)
  if (d) {
    if (ep_log) {
      ep_log[e * 4 + 0] = ep_ret;
      ep_log[e * 4 + 1] = ep_len;
      ep_log[e * 4 + 2] += 1.f;
    }
    classic_reset_obs(V.kind, V.seed, e, (uint64_t)step * 16 + 7, nv);
    gst[vecs::EPRET] = 0.f;
    gst[vecs::EPLEN] = 0.f;
  } else {
    gst[vecs::EPRET] = ep_ret;
    gst[vecs::EPLEN] = ep_len;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) gst[k] = nv[k];
  for (int k = 0; k < V.obs; ++k) V.ring[(size_t)slot * V.obs + k] = nv[k];
  new_frame[e] = slot;
}

__global__ void vec_classic_step_k(VecEnv V, const int* __restrict__ actions, const int64_t* step_counter,
                                   float* reward, float* done, int* new_frame, float* ep_log) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= V.E) return;
  classic_env_step(V, e, step_counter ? step_counter[0] : 0, actions[e], reward, done, new_frame, ep_log);
}

// ------------------------------------------------------------------ MLP dueling forward
// LDS of a forward workgroup: both heads' first layers, transposed ([k][j], pitch 129), and the
// activations of kRows rows.
struct alignas(16) FwdLds {
  float W[2 * kWHead];          // advantage.0 | value.0
  float x[kRows * kVecMaxObs];
  float f[kRows * kH];          // relu(features.0)
  float h[kRows * 2 * kH];      // relu(advantage.0) | relu(value.0)
  float q[kRows * 8];
};

// 128 elements per thread in rounds of 32 loads issued before their LDS stores: the copy pays the
// global latency 4 times, not once per element (8 loads in flight: 16 rounds, 2/3 of the kernel)
__device__ __forceinline__ void stage_heads(const VecNet& n, float* W) {
  constexpr int kPer = 2 * kH * kH / kThreads, kInFlight = 32;
  static_assert(kPer % kInFlight == 0 && (kH * kH) % (kThreads * kInFlight) == 0, "a round stays within one head");
#pragma unroll
  for (int c0 = 0; c0 < kPer; c0 += kInFlight) {
    const int head = (c0 * kThreads) >> 14;  // compile-time per round
    const float* src = head ? n.wv1 : n.wa1;
    float v[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) v[u] = src[((c0 + u) * kThreads + threadIdx.x) & (kH * kH - 1)];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int li = ((c0 + u) * kThreads + threadIdx.x) & (kH * kH - 1);
      W[head * kWHead + (li & (kH - 1)) * kWPitch + (li >> 7)] = v[u];
    }
  }
}

// This thread's operands of the first two layers: its features.0 row and bias (unit j), its
// advantage.0 / value.0 bias (head, unit j).  They do not depend on the rows.
struct FwdOperands {
  float w[kVecMaxObs], b0, b1;
};

__device__ __forceinline__ FwdOperands load_fwd_operands(const VecNet& n) {
  const int t = threadIdx.x, j = t & (kH - 1), head = t >> 7;
  FwdOperands o;
#pragma unroll
  for (int k = 0; k < kVecMaxObs; ++k) o.w[k] = k < n.obs ? n.w0[j * n.obs + k] : 0.f;
  o.b0 = n.b0[j];
  o.b1 = (head ? n.bv1 : n.ba1)[j];
  return o;
}

// features.0: thread = (unit j, 4 rows).  L.x -> L.f
__device__ __forceinline__ void fwd_features(const FwdOperands& o, FwdLds& L) {
  const int t = threadIdx.x, j = t & (kH - 1), r0 = (t >> 7) * 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float acc = o.b0;
#pragma unroll
    for (int k = 0; k < kVecMaxObs; ++k) acc = fmaf(o.w[k], L.x[(r0 + r) * kVecMaxObs + k], acc);
    L.f[(r0 + r) * kH + j] = fmaxf(acc, 0.f);
  }
}

// advantage.0 / value.0: thread = (head, unit j), all rows.  L.f -> L.h
__device__ __forceinline__ void fwd_hidden(const FwdOperands& o, FwdLds& L) {
  const int t = threadIdx.x, j = t & (kH - 1), head = t >> 7;
  float acc[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) acc[r] = o.b1;
  const float* Wh = L.W + head * kWHead + j;
  for (int k = 0; k < kH; k += 4) {
    const float w0 = Wh[(k + 0) * kWPitch], w1 = Wh[(k + 1) * kWPitch], w2 = Wh[(k + 2) * kWPitch],
                w3 = Wh[(k + 3) * kWPitch];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const float4 fv = *reinterpret_cast<const float4*>(&L.f[r * kH + k]);
      acc[r] = fmaf(w0, fv.x, acc[r]);
      acc[r] = fmaf(w1, fv.y, acc[r]);
      acc[r] = fmaf(w2, fv.z, acc[r]);
      acc[r] = fmaf(w3, fv.w, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r) L.h[r * 2 * kH + t] = fmaxf(acc[r], 0.f);
}

// Q of the kRows rows in L.x (weights of `n` already staged in L.W) -> L.f, L.h, L.q.
// Begins and ends with a workgroup barrier.
__device__ void vec_forward(const VecNet& n, FwdLds& L) {
  const int t = threadIdx.x;
  __syncthreads();
  const FwdOperands op = load_fwd_operands(n);
  fwd_features(op, L);
  __syncthreads();
  fwd_hidden(op, L);
  __syncthreads();
  {  // advantage.2 / value.2 and the dueling combine: a wave per row pair
    const int lane = t & 63, wave = t >> 6;
    for (int r = wave; r < kRows; r += 4) {
      const float* hr = L.h + r * 2 * kH;
      float advsum = 0.f, val = 0.f;
      for (int o = 0; o <= n.A; ++o) {
        const float* wo = o < n.A ? n.wa2 + o * kH : n.wv2;
        const float* hb = o < n.A ? hr : hr + kH;
        float p = fmaf(wo[lane], hb[lane], wo[lane + 64] * hb[lane + 64]);
        p = wave_sum(p);
        if (o < n.A) {
          p += n.ba2[o];
          advsum += p;
          if (lane == 0) L.q[r * 8 + o] = p;
        } else {
          val = p + n.bv2[0];
        }
      }
      if (lane == 0) {
        const float mean = advsum / (float)n.A;
        for (int o = 0; o < n.A; ++o) L.q[r * 8 + o] = val + L.q[r * 8 + o] - mean;
      }
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------ acting
__global__ __launch_bounds__(kThreads) void vec_act_k(VecAct a) {
  __shared__ FwdLds L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows;
  if (t < kRows * kVecMaxObs) {
    const int r = t / kVecMaxObs, k = t % kVecMaxObs;
    const int e = min(e0 + r, a.E - 1);  // rows past E repeat the last env (never written)
    L.x[t] = k < a.net.obs ? a.ring[(size_t)a.hist[e * 4 + 3] * a.net.obs + k] : 0.f;
  }
  stage_heads(a.net, L.W);
  vec_forward(a.net, L);
  const int e = e0 + t;
  if (t < kRows && e < a.E) {
    const int A = a.net.A;
    const float* row = L.q + t * 8;
    // select_actions_k's draw: first argmax; explore iff !(u0 > eps); min(int(u1 A), A - 1)
    int best = 0;
    float bv = row[0];
    for (int k = 1; k < A; ++k)
      if (row[k] > bv) { bv = row[k]; best = k; }
    for (int k = 0; k < A; ++k) a.q[(size_t)e * A + k] = row[k];
    float u[4];
    uniform4(a.seed, (uint64_t)e, a.counter ? (uint64_t)a.counter[0] : 0ull, u);
    if (!(u[0] > a.eps[e])) {
      const int r = (int)(u[1] * (float)A);
      best = r < A ? r : A - 1;
    }
    a.actions[e] = best;
  }
}

// ------------------------------------------------------------------ greedy act over host envs
// The act half of one evaluator step over HOST envs (engine/vector_host_eval.py): vec_act_k with
// the observation read straight from the staging block's reset_obs rows and the step k by value --
// no ring, no hist, no counter in memory.  The observation load is issued before stage_heads and
// lands in L.x behind it: it is in flight under the head staging.  Same forward, same draw at
// epsilon 0 (explore iff !(u0 > 0)): Q and the actions are vec_act_k's bit for bit.
__global__ __launch_bounds__(kThreads) void vec_host_eval_act_k(VecHostEvalAct a) {
  __shared__ FwdLds L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows;
  float x = 0.f;
  if (t < kRows * kVecMaxObs) {
    const int r = t / kVecMaxObs, k = t % kVecMaxObs;
    const int e = min(e0 + r, a.N - 1);  // rows past N repeat the last env (never written)
    if (k < a.net.obs) x = a.stage[(size_t)(a.N + e) * a.net.obs + k];
  }
  stage_heads(a.net, L.W);
  if (t < kRows * kVecMaxObs) L.x[t] = x;
  vec_forward(a.net, L);
  const int e = e0 + t;
  if (t < kRows && e < a.N) {
    const int A = a.net.A;
    const float* row = L.q + t * 8;
    // vec_act_k's draw at eps = 0: first argmax; explore iff !(u0 > 0); min(int(u1 A), A - 1)
    int best = 0;
    float bv = row[0];
    for (int k = 1; k < A; ++k)
      if (row[k] > bv) { bv = row[k]; best = k; }
    for (int k = 0; k < A; ++k) a.q[(size_t)e * A + k] = row[k];
    float u[4];
    uniform4(a.seed, (uint64_t)e, (uint64_t)a.k, u);
    if (!(u[0] > 0.f)) {
      const int r = (int)(u[1] * (float)A);
      best = r < A ? r : A - 1;
    }
    a.actions[e] = best;
  }
}

// ------------------------------------------------------------------ one DQN.py frame
// The actor side of one frame of the single-process prioritized DQN in one workgroup: schedules,
// vec_act_k's forward and draw, the env step, the FrameStack advance, the replay insert at the
// running max priority and the tree walk.  Threads 0..E-1 each own one env after the forward.
// The tree walk (update_levels_block) needs no LDS beyond the E slots: the head image stays.
__global__ __launch_bounds__(kThreads) void dqn_frame_k(DqnFrame f) {
  __shared__ FwdLds L;
  __shared__ int sids[kRows];
  const int t = threadIdx.x;
  const int E = f.env.E;
  // both counters are read by every thread here and advanced by thread 0 behind the last barrier
  const int64_t step = f.t[0];
  const int64_t filled = f.filled[0];
  if (t < kRows * kVecMaxObs) {
    const int r = t / kVecMaxObs, k = t % kVecMaxObs;
    const int e = min(r, E - 1);  // rows past E repeat the last env (never written), as vec_act_k
    L.x[t] = k < f.net.obs ? f.env.ring[(size_t)f.hist[e * 4 + 3] * f.net.obs + k] : 0.f;
  }
  // eps(t), beta(t) in fp64, rounded to fp32 once (algo/schedules.py)
  const double st = (double)step;
  const float eps = (float)(f.eps_final + (f.eps_start - f.eps_final) * exp(-st / f.eps_decay));
  if (t == 0) {
    f.eps_out[0] = eps;
    f.beta_out[0] = (float)fmin(1.0, f.beta0 + st * (1.0 - f.beta0) / f.beta_horizon);
  }
  stage_heads(f.net, L.W);
  vec_forward(f.net, L);
  if (t < E) {
    const int e = t, A = f.net.A;
    const float* row = L.q + t * 8;
    // vec_act_k's draw: first argmax; explore iff !(u0 > eps); min(int(u1 A), A - 1)
    int best = 0;
    float bv = row[0];
    for (int k = 1; k < A; ++k)
      if (row[k] > bv) { bv = row[k]; best = k; }
    for (int k = 0; k < A; ++k) f.q[(size_t)e * A + k] = row[k];
    float u[4];
    uniform4(f.act_seed, (uint64_t)e, (uint64_t)step, u);
    if (!(u[0] > eps)) {
      const int r = (int)(u[1] * (float)A);
      best = r < A ? r : A - 1;
    }
    f.actions[e] = best;
    classic_env_step(f.env, e, step, best, f.reward, f.done, f.new_frame, f.ep_log);
    // FrameStack advance (frame_hist_step_k) and the transition (hist before, a, r, hist after, done)
    int4* hp = reinterpret_cast<int4*>(f.hist) + e;
    const int4 h0 = *hp;
    const int nf = f.new_frame[e];
    const float d = f.done[e];
    const int4 h1 = d > 0.f ? make_int4(nf, nf, nf, nf) : make_int4(h0.y, h0.z, h0.w, nf);
    *hp = h1;
    if (d > 0.f && f.ep_log) f.ep_log[e * 4 + 3] += f.ep_log[e * 4 + 0];  // sum of finished returns
    const int j = (int)((filled + e) % f.C);
    reinterpret_cast<int4*>(f.tt.s_ids)[j] = h0;
    reinterpret_cast<int4*>(f.tt.s2_ids)[j] = h1;
    f.tt.action[j] = best;
    f.tt.reward[j] = f.reward[e];
    f.tt.done[j] = d;
    // insert at the running max priority (write_leaf's "no priority given"); max_prio stays
    write_leaf(f.tree, j, f.max_prio[0], f.alpha);
    sids[e] = j;
    f.slot[e] = j;
  }
  update_levels_block(f.tree, sids, E, 1, f.tree.levels);  // (each level begins with a barrier)
  if (t == 0) {
    f.filled[0] = filled + E;
    f.t[0] = step + 1;
  }
}

// ------------------------------------------------------------------ greedy rollouts
// This lane's operands of the output layers, held across env steps: output o < A is
// advantage.2 row o, output A is value.2 (lanes `lane` and `lane + 64` of each row).
struct OutOperands {
  float lo[kVecMaxA + 1], hi[kVecMaxA + 1], b[kVecMaxA + 1];
};

__device__ __forceinline__ OutOperands load_out_operands(const VecNet& n) {
  const int lane = threadIdx.x & 63;
  OutOperands w;
#pragma unroll
  for (int o = 0; o <= kVecMaxA; ++o) {
    const float* wo = o < n.A ? n.wa2 + o * kH : n.wv2;
    w.lo[o] = o <= n.A ? wo[lane] : 0.f;
    w.hi[o] = o <= n.A ? wo[lane + 64] : 0.f;
    w.b[o] = o < n.A ? n.ba2[o] : o == n.A ? n.bv2[0] : 0.f;
  }
  return w;
}

// vec_forward with every step-invariant load taken by the caller: the same fma chains, sums
// and reductions in the same order, so Q is bit-equal to vec_forward's.
__device__ __forceinline__ void vec_forward_held(int A, const FwdOperands& op, const OutOperands& w, FwdLds& L) {
  const int t = threadIdx.x;
  __syncthreads();
  fwd_features(op, L);
  __syncthreads();
  fwd_hidden(op, L);
  __syncthreads();
  {  // advantage.2 / value.2 and the dueling combine: a wave per row pair
    const int lane = t & 63, wave = t >> 6;
    for (int r = wave; r < kRows; r += 4) {
      const float* hr = L.h + r * 2 * kH;
      float advsum = 0.f, val = 0.f;
#pragma unroll
      for (int o = 0; o <= kVecMaxA; ++o) {
        if (o > A) continue;  // (uniform)
        const float* hb = o < A ? hr : hr + kH;
        float p = fmaf(w.lo[o], hb[lane], w.hi[o] * hb[lane + 64]);
        p = wave_sum(p);
        if (o < A) {
          p += w.b[o];
          advsum += p;
          if (lane == 0) L.q[r * 8 + o] = p;
        } else {
          val = p + w.b[o];
        }
      }
      if (lane == 0) {
        const float mean = advsum / (float)A;
        for (int o = 0; o < A; ++o) L.q[r * 8 + o] = val + L.q[r * 8 + o] - mean;
      }
    }
  }
  __syncthreads();
}

// One workgroup plays kRows greedy episodes from reset to their first done.  Threads 0..7 each
// own one episode (state, return and length in registers); all 256 threads run the forward.
// A row that has ended, or lies past N, stays in L.x as it was and is never written again.
__global__ __launch_bounds__(kThreads) void vec_rollout_k(VecRollout p) {
  __shared__ FwdLds L;
  __shared__ int any_live;
  const int t = threadIdx.x;
  const int e = blockIdx.x * kRows + t;
  const int obs = p.obs, A = p.net.A;
  const bool tracing = p.trace_obs != nullptr;
  bool live = t < kRows && e < p.N;
  float st[4] = {0.f, 0.f, 0.f, 0.f};
  float ret = 0.f;
  int len = 0;
  if (t < kRows) {
    // vec_classic_reset's draw at step counter 0 (rows past N repeat the last episode's)
    classic_reset_obs(p.kind, p.seed, min(e, p.N - 1), 1, st);
#pragma unroll
    for (int k = 0; k < kVecMaxObs; ++k) L.x[t * kVecMaxObs + k] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < obs) L.x[t * kVecMaxObs + k] = st[k];
  }
  stage_heads(p.net, L.W);
  const FwdOperands op = load_fwd_operands(p.net);
  const OutOperands wout = load_out_operands(p.net);
  for (int step = 0; step < p.max_steps; ++step) {
    vec_forward_held(A, op, wout, L);
    if (t < 64) {  // (the owners' wave)
      if (live) {
        const float* row = L.q + t * 8;
        int best = 0;  // vec_act_k's first argmax
        float bv = row[0];
        for (int k = 1; k < A; ++k)
          if (row[k] > bv) { bv = row[k]; best = k; }
        if (tracing && step < p.trace_T) {
          const size_t at = (size_t)e * p.trace_T + step;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < obs) p.trace_obs[at * obs + k] = st[k];
          for (int k = 0; k < A; ++k) p.trace_q[at * A + k] = row[k];
          p.trace_act[at] = best;
        }
        float nv[4], r;
        bool term;
        classic_dynamics(p.kind, st, best, nv, r, term);
        ret += r;
        len += 1;
        if (term || len >= p.max_steps) {
          p.returns[e] = ret;
          p.lengths[e] = len;
          p.ended[e] = term ? 1 : 2;
          live = false;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            st[k] = nv[k];
            if (k < obs) L.x[t * kVecMaxObs + k] = nv[k];
          }
        }
      }
      const bool any = __ballot(live) != 0ull;
      if (t == 0) any_live = any;
    }
    __syncthreads();
    if (!any_live) break;  // (uniform; the next write of any_live lies behind the forward's barriers)
  }
}

// ------------------------------------------------------------------ learner
constexpr int kSamples = kRows / 2;  // sampled rows per workgroup: rows 0..3 = s, 4..7 = s'

__global__ __launch_bounds__(kThreads) void vec_learn_k(VecLearn p) {
  __shared__ FwdLds L;
  __shared__ float qt[kRows * 8];
  __shared__ __align__(16) float dh[kSamples * 2 * kH];
  __shared__ float dfp[2 * kSamples * kH];
  __shared__ float sg[kSamples];
  __shared__ int sa[kSamples];
  const int t = threadIdx.x, j = t & (kH - 1), head = t >> 7;
  const int b0 = blockIdx.x * kSamples;
  const int obs = p.on.obs, A = p.on.A;
  if (blockIdx.x == 0 && t == 0 && p.beta_out) {
    // PER beta of the NEXT step (this step's draw has run): beta_by_frame(step + 1)
    const double st = (double)(p.step ? p.step[0] : 0) + 1.0;
    p.beta_out[0] = (float)fmin(1.0, p.beta0 + st * (1.0 - p.beta0) / p.beta_horizon);
  }
  if (t < kRows * kVecMaxObs) {
    const int r = t / kVecMaxObs, k = t % kVecMaxObs;
    const int b = min(b0 + (r & (kSamples - 1)), p.B - 1);
    const int row = p.idx[b];
    const int id = (r < kSamples ? p.s_ids : p.s2_ids)[row * 4 + 3];
    L.x[t] = k < obs ? p.ring[(size_t)id * obs + k] : 0.f;
  }
  // target net first, so the online heads stay in LDS for the backward
  stage_heads(p.tg, L.W);
  vec_forward(p.tg, L);
  if (t < kRows * 8) qt[t] = L.q[t];
  __syncthreads();
  stage_heads(p.on, L.W);
  vec_forward(p.on, L);
  if (t < kSamples) {
    const int b = b0 + t;
    float g = 0.f;
    int a = 0;
    if (b < p.B) {
      const int row = p.idx[b];
      a = min(max(p.act[row], 0), A - 1);
      const float* q2 = L.q + (kSamples + t) * 8;
      int astar = 0;
      float best = q2[0];
      for (int k = 1; k < A; ++k)
        if (q2[k] > best) { best = q2[k]; astar = k; }
      // the arithmetic of dqn_loss_k
      const float y = p.rew[row] + p.gamma_n * qt[(kSamples + t) * 8 + astar] * (1.f - p.done[row]);
      const float qa = L.q[t * 8 + a];
      const float delta = fabsf(y - qa);
      const float hub = delta < 1.f ? 0.5f * delta * delta : delta - 0.5f;
      p.delta[b] = delta;
      p.lw[b] = p.w[b] * hub;
      g = p.w[b] / (float)p.B * fminf(fmaxf(qa - y, -1.f), 1.f);
      for (int k = 0; k < A; ++k) {
        p.q_s[(size_t)b * A + k] = L.q[t * 8 + k];
        p.q_s2[(size_t)b * A + k] = q2[k];
        p.qt_s2[(size_t)b * A + k] = qt[(kSamples + t) * 8 + k];
      }
      // Q = V + A_a - mean(A): dV = g, dA_k = g (1[k == a] - 1/A)
      float* v = p.vec + (size_t)b * vecv::STRIDE;
      for (int k = 0; k < 8; ++k) v[vecv::DA + k] = k < A ? g * ((k == a ? 1.f : 0.f) - 1.f / (float)A) : 0.f;
      v[vecv::DA + 7] = g;
    }
    sg[t] = g;
    sa[t] = a;
  }
  __syncthreads();
  {  // d(hidden pre-activation): thread = (head, unit j)
    float wa[kVecMaxA];
#pragma unroll
    for (int k = 0; k < kVecMaxA; ++k) wa[k] = (head == 0 && k < A) ? p.on.wa2[k * kH + j] : 0.f;
    const float wv = p.on.wv2[j];
    const float invA = 1.f / (float)A;
#pragma unroll
    for (int r = 0; r < kSamples; ++r) {
      const float g = sg[r];
      float s;
      if (head == 0) {
        s = 0.f;
#pragma unroll
        for (int k = 0; k < kVecMaxA; ++k) s = fmaf(g * ((k == sa[r] ? 1.f : 0.f) - invA), wa[k], s);
      } else {
        s = g * wv;
      }
      const float hv = L.h[r * 2 * kH + t];
      s = hv > 0.f ? s : 0.f;
      dh[r * 2 * kH + t] = s;
      if (b0 + r < p.B) {
        float* v = p.vec + (size_t)(b0 + r) * vecv::STRIDE;
        v[vecv::H + t] = hv;
        v[vecv::DH + t] = s;
      }
    }
  }
  __syncthreads();
  {  // d(features) = W_adv1^T dh_adv + W_val1^T dh_val: thread = (head, input k), partial per head
    float acc[kSamples] = {0.f, 0.f, 0.f, 0.f};
    const float* Wk = L.W + head * kWHead + j * kWPitch;  // row k = j of the transposed image
    for (int u = 0; u < kH; u += 4) {
      const float w0 = Wk[u], w1 = Wk[u + 1], w2 = Wk[u + 2], w3 = Wk[u + 3];
#pragma unroll
      for (int r = 0; r < kSamples; ++r) {
        const float4 d = *reinterpret_cast<const float4*>(&dh[r * 2 * kH + head * kH + u]);
        acc[r] = fmaf(w0, d.x, acc[r]);
        acc[r] = fmaf(w1, d.y, acc[r]);
        acc[r] = fmaf(w2, d.z, acc[r]);
        acc[r] = fmaf(w3, d.w, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kSamples; ++r) dfp[(head * kSamples + r) * kH + j] = acc[r];
  }
  __syncthreads();
  for (int i = t; i < kSamples * kH; i += kThreads) {
    const int r = i >> 7, k = i & (kH - 1);
    if (b0 + r >= p.B) continue;
    const float fv = L.f[r * kH + k];
    float* v = p.vec + (size_t)(b0 + r) * vecv::STRIDE;
    v[vecv::F + k] = fv;
    v[vecv::DF + k] = fv > 0.f ? dfp[r * kH + k] + dfp[(kSamples + r) * kH + k] : 0.f;
    if (k < kVecMaxObs) v[vecv::X + k] = L.x[r * kVecMaxObs + k];
  }
}

// ------------------------------------------------------------------ batch contraction
// grad[i] = sum_b G[b][row] * X[b][col] for the tensor that owns flat element i (the ten
// tensors of DuelingDQN.parameters() in order), b ascending; + one fp64 sum-of-squares
// partial per workgroup.
__global__ __launch_bounds__(kThreads) void vec_grad_k(VecGrad g) {
  __shared__ double red[kThreads / 64];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int obs = g.obs, A = g.A;
  float v = 0.f;
  if (i < g.n) {
    // (offset, columns, output-gradient vector, input vector) of the owning tensor
    int64_t off = 0;
    int cols, goff, xoff;
    const int64_t o1 = (int64_t)kH * obs, o2 = o1 + kH, o3 = o2 + kH * kH, o4 = o3 + kH, o5 = o4 + (int64_t)A * kH,
                  o6 = o5 + A, o7 = o6 + kH * kH, o8 = o7 + kH, o9 = o8 + kH;
    if (i < o1)      { off = 0;  cols = obs; goff = vecv::DF;      xoff = vecv::X; }
    else if (i < o2) { off = o1; cols = 1;   goff = vecv::DF;      xoff = -1; }
    else if (i < o3) { off = o2; cols = kH;  goff = vecv::DH;      xoff = vecv::F; }
    else if (i < o4) { off = o3; cols = 1;   goff = vecv::DH;      xoff = -1; }
    else if (i < o5) { off = o4; cols = kH;  goff = vecv::DA;      xoff = vecv::H; }
    else if (i < o6) { off = o5; cols = 1;   goff = vecv::DA;      xoff = -1; }
    else if (i < o7) { off = o6; cols = kH;  goff = vecv::DH + kH; xoff = vecv::F; }
    else if (i < o8) { off = o7; cols = 1;   goff = vecv::DH + kH; xoff = -1; }
    else if (i < o9) { off = o8; cols = kH;  goff = vecv::DA + 7;  xoff = vecv::H + kH; }
    else             { off = o9; cols = 1;   goff = vecv::DA + 7;  xoff = -1; }
    const int local = (int)(i - off);
    const int row = local / cols, col = local - row * cols;
    // 8 samples' loads in flight per round, summed in batch order (x = 1 for a bias)
    const float* pg = g.vec + goff + row;
    const float* px = xoff >= 0 ? g.vec + xoff + col : nullptr;
    int b = 0;
    for (; b + 8 <= g.B; b += 8) {
      float gv[8], xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        gv[u] = pg[(size_t)(b + u) * vecv::STRIDE];
        xv[u] = px ? px[(size_t)(b + u) * vecv::STRIDE] : 1.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) v = fmaf(gv[u], xv[u], v);
    }
    for (; b < g.B; ++b) v = fmaf(pg[(size_t)b * vecv::STRIDE], px ? px[(size_t)b * vecv::STRIDE] : 1.f, v);
    g.grad[i] = v;
  }
  double sq = wave_sum((double)v * (double)v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) g.part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

void check_net(const VecNet& n, const char* who) {
  if (n.obs < 1 || n.obs > kVecMaxObs || n.A < 1 || n.A > kVecMaxA)
    throw std::invalid_argument(std::string(who) + ": obs in [1, 8] and actions in [1, 7]");
  if (!n.w0 || !n.b0 || !n.wa1 || !n.ba1 || !n.wa2 || !n.ba2 || !n.wv1 || !n.bv1 || !n.wv2 || !n.bv2)
    throw std::invalid_argument(std::string(who) + ": missing parameter tensor");
}

void check_env_kind(int kind, int obs) {
  if (kind < 0 || kind > 1) throw std::invalid_argument("vec classic env: kind 0 (CartPole) / 1 (MountainCar)");
  if (obs != (kind == 0 ? 4 : 2)) throw std::invalid_argument("vec classic env: obs must be 4 (CartPole) / 2");
}

void check_env(const VecEnv& V) {
  check_env_kind(V.kind, V.obs);
  if (V.E < 1 || V.F < 2 * V.E) throw std::invalid_argument("vec classic env: ring must hold >= 2 E rows");
  if (!V.state || !V.ring) throw std::invalid_argument("vec classic env: state / ring missing");
}

}  // namespace

// ------------------------------------------------------------------ launchers
void vec_classic_reset(const VecEnv& V, const int64_t* step_counter, int* new_frame, int* hist, float* ep_log,
                       hipStream_t s) {
  check_env(V);
  vec_classic_reset_k<<<(V.E + 63) / 64, 64, 0, s>>>(V, step_counter, new_frame, hist, ep_log);
  LAUNCH_CHECK();
}

void vec_classic_step(const VecEnv& V, const int* actions, const int64_t* step_counter, float* reward, float* done,
                      int* new_frame, float* ep_log, hipStream_t s) {
  check_env(V);
  vec_classic_step_k<<<(V.E + 63) / 64, 64, 0, s>>>(V, actions, step_counter, reward, done, new_frame, ep_log);
  LAUNCH_CHECK();
}

void vec_act(const VecAct& a, hipStream_t s) {
  check_net(a.net, "vec_act");
  if (a.E < 1 || !a.ring || !a.hist || !a.eps || !a.q || !a.actions)
    throw std::invalid_argument("vec_act: E >= 1 with ring, hist, eps, q and actions");
  vec_act_k<<<(a.E + kRows - 1) / kRows, kThreads, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vec_host_eval_act(const VecHostEvalAct& a, hipStream_t s) {
  check_net(a.net, "vec_host_eval_act");
  if (a.N < 1 || a.N > 64) throw std::invalid_argument("vec_host_eval_act: 1 <= N <= 64 evaluator envs");
  if (a.k < 0) throw std::invalid_argument("vec_host_eval_act: step k >= 0");
  if (!a.stage) throw std::invalid_argument("vec_host_eval_act: the staging block's device copy");
  if (!a.q || !a.actions) throw std::invalid_argument("vec_host_eval_act: q and actions");
  vec_host_eval_act_k<<<(a.N + kRows - 1) / kRows, kThreads, 0, s>>>(a);
  LAUNCH_CHECK();
}

void dqn_frame(const DqnFrame& f, hipStream_t s) {
  check_net(f.net, "dqn_frame");
  check_env(f.env);
  if (f.net.obs != f.env.obs) throw std::invalid_argument("dqn_frame: the net's obs differs from the env's");
  if (f.env.E > kRows) throw std::invalid_argument("dqn_frame: at most 8 envs (one forward pass of a workgroup)");
  if (f.C < f.env.E || f.tree.size[0] != f.C || f.tree.levels < 1 || !f.tree.leaf_sum || !f.tree.leaf_min)
    throw std::invalid_argument("dqn_frame: the tree must have one leaf per replay slot, capacity >= E");
  if (!f.hist || !f.t || !f.eps_out || !f.beta_out || !f.q || !f.actions || !f.reward || !f.done || !f.new_frame ||
      !f.filled || !f.slot || !f.max_prio || !f.tt.s_ids || !f.tt.s2_ids || !f.tt.action || !f.tt.reward ||
      !f.tt.done)
    throw std::invalid_argument("dqn_frame: missing buffer");
  if (!(f.eps_decay > 0.0) || !(f.beta_horizon > 0.0))
    throw std::invalid_argument("dqn_frame: epsilon decay and beta horizon must be > 0");
  dqn_frame_k<<<1, kThreads, 0, s>>>(f);
  LAUNCH_CHECK();
}

void vec_rollout(const VecRollout& r, hipStream_t s) {
  check_net(r.net, "vec_rollout");
  check_env_kind(r.kind, r.obs);
  if (r.net.obs != r.obs) throw std::invalid_argument("vec_rollout: the net's obs differs from the env's");
  if (r.N < 1 || r.N > 1024) throw std::invalid_argument("vec_rollout: N must be in [1, 1024]");
  if (r.max_steps < 1 || r.max_steps > 10000)
    throw std::invalid_argument("vec_rollout: max_steps must be in [1, 10000]");
  if (!r.returns || !r.lengths || !r.ended) throw std::invalid_argument("vec_rollout: returns, lengths and ended");
  const int given = (r.trace_obs != nullptr) + (r.trace_q != nullptr) + (r.trace_act != nullptr);
  if (given != 0 && given != 3) throw std::invalid_argument("vec_rollout: the trace is all three buffers or none");
  if (given == 3 && r.trace_T < 1) throw std::invalid_argument("vec_rollout: trace_T >= 1 with a trace");
  vec_rollout_k<<<(r.N + kRows - 1) / kRows, kThreads, 0, s>>>(r);
  LAUNCH_CHECK();
}

void vec_learn(const VecLearn& p, hipStream_t s) {
  check_net(p.on, "vec_learn (online)");
  check_net(p.tg, "vec_learn (target)");
  if (p.on.obs != p.tg.obs || p.on.A != p.tg.A) throw std::invalid_argument("vec_learn: nets differ in shape");
  if (p.B < 1 || p.B > 1024) throw std::invalid_argument("vec_learn: batch must be in [1, 1024]");
  if (!p.ring || !p.s_ids || !p.s2_ids || !p.act || !p.rew || !p.done || !p.idx || !p.w || !p.q_s || !p.q_s2 ||
      !p.qt_s2 || !p.vec || !p.delta || !p.lw)
    throw std::invalid_argument("vec_learn: missing buffer");
  if (p.beta_out && !(p.beta_horizon > 0.0)) throw std::invalid_argument("vec_learn: beta horizon must be > 0");
  vec_learn_k<<<(p.B + kSamples - 1) / kSamples, kThreads, 0, s>>>(p);
  LAUNCH_CHECK();
}

int64_t vec_param_count(int obs, int A) {
  return (int64_t)kH * obs + kH + 2 * ((int64_t)kH * kH + kH) + (int64_t)A * kH + A + kH + 1;
}

int vec_grad_blocks(int64_t n) { return (int)((n + kThreads - 1) / kThreads); }

void vec_grad(const VecGrad& g, hipStream_t s) {
  if (g.obs < 1 || g.obs > kVecMaxObs || g.A < 1 || g.A > kVecMaxA || g.n != vec_param_count(g.obs, g.A))
    throw std::invalid_argument("vec_grad: n must be the MLP dueling net's parameter count");
  if (g.B < 1 || !g.vec || !g.grad || !g.part) throw std::invalid_argument("vec_grad: missing buffer");
  vec_grad_k<<<vec_grad_blocks(g.n), kThreads, 0, s>>>(g);
  LAUNCH_CHECK();
}

}  // namespace apex
