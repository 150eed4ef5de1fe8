// Device bodies shared by the stepwise AQL acting kernels (aql_kernels.hip: aql_propose_k,
// aql_candidate_q_k; aql_engine_kernels.hip: the vector envs), the one-launch greedy rollout
// (aql_rollout_kernels.hip) and the one-launch acting frame (aql_frame_kernels.hip).  Each
// function is the per-state / per-candidate / per-env body of one kernel with its operands
// passed as pointers: the callers choose where a matrix lives (LDS or global) and how the work
// is spread over threads, the arithmetic order is fixed here -- so the rollout and the frame
// reproduce the stepwise kernels bit for bit.  Every multiply-add of the network
// bodies is an explicit fmaf: left to -ffp-contract=fast, the compiler fused a dot product in
// one caller and (after vectorising two chains into packed mul + add) not in another.
#pragma once
#include "common.h"
#include "kernels.h"

namespace apex {
namespace aqld {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kH = 64;        // hidden units of q_feature / action_out / advantage1
constexpr int kCat = 128;     // concat width, proposal hidden width
constexpr int kPitch = 129;   // LDS row pitch (floats) of the critic's 128-wide rows
constexpr int kQf2Pitch = 65; // LDS row pitch of q_feature.2
constexpr int kBwObs = 24, kBwAct = 4;

// element i of the critic's effective NoisyLinear workspace (W1 [64][128] | b1 [64] | w2 [64] |
// b2 [1]): mu + sigma * eps in train mode, mu in eval mode
__device__ __forceinline__ float noisy_eff_val(const AQLNet& net, int i) {
  const int n1 = kH * kCat;
  auto eff = [&](const float* mu, const float* sg, const float* ep, int k) {
    return net.noisy ? fmaf(sg[k], ep[k], mu[k]) : mu[k];
  };
  if (i < n1) return eff(net.a1_wmu, net.a1_wsig, net.a1_weps, i);
  if (i < n1 + kH) return eff(net.a1_bmu, net.a1_bsig, net.a1_beps, i - n1);
  if (i < n1 + 2 * kH) return eff(net.a2_wmu, net.a2_wsig, net.a2_weps, i - n1 - kH);
  return eff(net.a2_bmu, net.a2_bsig, net.a2_beps, 0);
}

// ------------------------------------------------------------------ critic (one wave)
// The state half of one state `s`: q_feature (obs -> 64 -> 64, ReLU both) and advantage1's bias
// plus its state columns.  qf1: q_feature.0 rows at pitch p1; qf2s / w1s: LDS images at
// kQf2Pitch / kPitch; hb, qf: 64-float scratch of this wave.  Returns lane's unit.
__device__ __forceinline__ float q_state(const float* qf1, int p1, const float* qf_b1, const float* qf_b2,
                                         const float* s, int obs, const float* qf2s, const float* w1s,
                                         const float* b1eff, float* hb, float* qf, int lane) {
  float acc = qf_b1[lane];
  for (int i = 0; i < obs; ++i) acc = fmaf(qf1[lane * p1 + i], s[i], acc);
  hb[lane] = fmaxf(acc, 0.f);
  __builtin_amdgcn_wave_barrier();
  acc = qf_b2[lane];
#pragma unroll 8
  for (int j = 0; j < kH; ++j) acc = fmaf(qf2s[lane * kQf2Pitch + j], hb[j], acc);
  qf[lane] = fmaxf(acc, 0.f);
  __builtin_amdgcn_wave_barrier();
  float sadv = b1eff[lane];  // advantage1 bias + its state half
#pragma unroll 8
  for (int j = 0; j < kH; ++j) sadv = fmaf(w1s[lane * kPitch + kH + j], qf[j], sadv);
  return sadv;
}

// Q of one candidate `a` (adim floats; the discrete envs' action index as one float) on top of
// the state half `sadv`.  ao1: action_out.0 rows at pitch pa; hb: 128, xb: 64 floats of scratch.
__device__ __forceinline__ float q_cand(const AQLNet& net, const float* ao1, int pa, const float* a, const float* w1s,
                                        const float* ao2s, const float* w2eff, float b2eff, float sadv, float* hb,
                                        float* xb, int lane) {
  float acc;
  if (net.cont) {
    float h0 = net.ao_b1[lane], h1 = net.ao_b1[lane + 64];
    for (int d = 0; d < net.adim; ++d) {
      const float ad = a[d];
      h0 = fmaf(ao1[lane * pa + d], ad, h0);
      h1 = fmaf(ao1[(lane + 64) * pa + d], ad, h1);
    }
    __builtin_amdgcn_wave_barrier();
    hb[lane] = fmaxf(h0, 0.f);
    hb[lane + 64] = fmaxf(h1, 0.f);
    __builtin_amdgcn_wave_barrier();
    acc = net.ao_b2[lane];
#pragma unroll 8
    for (int j = 0; j < kCat; ++j) acc = fmaf(ao2s[lane * kPitch + j], hb[j], acc);
    xb[lane] = fmaxf(acc, 0.f);
  } else {
    xb[lane] = fmaxf(fmaf(ao1[lane * pa], a[0], net.ao_b1[lane]), 0.f);
  }
  __builtin_amdgcn_wave_barrier();
  // advantage1 (NoisyLinear 128 -> 64): the action half on top of the state half; advantage2 (64 -> 1)
  acc = sadv;
#pragma unroll 8
  for (int j = 0; j < kH; ++j) acc = fmaf(w1s[lane * kPitch + j], xb[j], acc);
  const float qv = wave_sum(w2eff[lane] * fmaxf(acc, 0.f)) + b2eff;
  __builtin_amdgcn_wave_barrier();
  return qv;
}

// q_cand for four candidates at once (a[c]: candidate c's action): every weight read from LDS
// serves four candidates, whose activations sit interleaved ([unit][4]: one 16-byte broadcast
// read per unit) -- 6 LDS cycles per unit and four candidates instead of 16.  Each candidate's
// fma chain is q_cand's, in q_cand's order: the same bits.  hb: 512, xb: 256 floats of this
// wave's scratch, 16-byte aligned.
__device__ __forceinline__ void q_cand4(const AQLNet& net, const float* ao1, int pa, const float* const (&a)[4],
                                        const float* w1s, const float* ao2s, const float* w2eff, float b2eff,
                                        float sadv, float* hb, float* xb, int lane, float (&qv)[4]) {
  float acc[4];
  if (net.cont) {
    f32x4 h0, h1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      h0[c] = net.ao_b1[lane];
      h1[c] = net.ao_b1[lane + 64];
    }
    for (int d = 0; d < net.adim; ++d) {
      const float w0 = ao1[lane * pa + d], w1 = ao1[(lane + 64) * pa + d];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float ad = a[c][d];
        h0[c] = fmaf(w0, ad, h0[c]);
        h1[c] = fmaf(w1, ad, h1[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      h0[c] = fmaxf(h0[c], 0.f);
      h1[c] = fmaxf(h1[c], 0.f);
    }
    __builtin_amdgcn_wave_barrier();
    *reinterpret_cast<f32x4*>(hb + 4 * lane) = h0;
    *reinterpret_cast<f32x4*>(hb + 4 * (lane + 64)) = h1;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = net.ao_b2[lane];
#pragma unroll 8
    for (int j = 0; j < kCat; ++j) {
      const float w = ao2s[lane * kPitch + j];
      const f32x4 x = *reinterpret_cast<const f32x4*>(hb + 4 * j);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = fmaf(w, x[c], acc[c]);
    }
    f32x4 xo;
#pragma unroll
    for (int c = 0; c < 4; ++c) xo[c] = fmaxf(acc[c], 0.f);
    *reinterpret_cast<f32x4*>(xb + 4 * lane) = xo;
  } else {
    f32x4 xo;
#pragma unroll
    for (int c = 0; c < 4; ++c) xo[c] = fmaxf(fmaf(ao1[lane * pa], a[c][0], net.ao_b1[lane]), 0.f);
    *reinterpret_cast<f32x4*>(xb + 4 * lane) = xo;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = sadv;
#pragma unroll 8
  for (int j = 0; j < kH; ++j) {
    const float w = w1s[lane * kPitch + j];
    const f32x4 x = *reinterpret_cast<const f32x4*>(xb + 4 * j);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = fmaf(w, x[c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) qv[c] = wave_sum(w2eff[lane] * fmaxf(acc[c], 0.f)) + b2eff;
  __builtin_amdgcn_wave_barrier();
}

// first argmax of q[0..T) by one wave (lowest index on ties), then aql_select_k's epsilon draw:
// stream `b` of `seed` at `ctr`; a 24-bit uniform <= eps takes a random candidate instead
__device__ __forceinline__ int select_cand(const float* q, int T, float eps, uint64_t seed, int b, uint64_t ctr,
                                           int lane) {
  float best = -INFINITY;
  int arg = 0x7fffffff;
  for (int t = lane; t < T; t += 64) {
    const float v = q[t];
    if (v > best || (v == best && t < arg)) { best = v; arg = t; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
  }
  float u[4];
  uniform4(seed, (uint64_t)b, ctr, u);
  if (u[0] <= eps) arg = min((int)(u[1] * (float)T), T - 1);  // random candidate (model.py:331-333)
  return arg;
}

// ------------------------------------------------------------------ proposal
// state embedding unit: features = Linear(obs -> 128) + ReLU (model.py:289-291); frow: the
// unit's row of q.features
__device__ __forceinline__ float prop_embed(const float* frow, const float* s, int obs, float bias) {
  float acc = bias;
  for (int i = 0; i < obs; ++i) acc = fmaf(frow[i], s[i], acc);
  return fmaxf(acc, 0.f);
}

// dist_feature.0 unit (128 -> 128, ReLU) for NS states at once: wr = the unit's row, e[k] = the
// k-th state's embedding (both 16-byte aligned)
template <int NS>
__device__ __forceinline__ void prop_hidden(const float* wr, const float* const (&e)[NS], float bj, float (&out)[NS]) {
  float a[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) a[k] = bj;
#pragma unroll 8
  for (int i = 0; i < kCat; i += 4) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(wr + i);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(e[k] + i);
      a[k] = fmaf(w[0], x[0], a[k]);
      a[k] = fmaf(w[1], x[1], a[k]);
      a[k] = fmaf(w[2], x[2], a[k]);
      a[k] = fmaf(w[3], x[3], a[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) out[k] = fmaxf(a[k], 0.f);
}

// dist_feature.2 unit (128 -> na): the mean (continuous) / logit (discrete) of one output
__device__ __forceinline__ float prop_out(const float* w2row, const float* hid, float bias) {
  float acc = bias;
#pragma unroll 16
  for (int i = 0; i < kCat; ++i) acc = fmaf(w2row[i], hid[i], acc);
  return acc;
}

// element e = (candidate tt, dim d) of row b's continuous candidate set: U(low, high) for the
// first U candidates, then MVN(mu, diag(var)) samples (Box-Muller); Philox stream b * 4096 + e
__device__ __forceinline__ float prop_sample_cont(int e, int A, int U, int b, uint64_t seed, uint64_t ctr,
                                                  const float* low, const float* high, const float* var,
                                                  const float* mu) {
  const int tt = e / A, d = e % A;
  float u[4];
  uniform4(seed, (uint64_t)b * 4096 + e, ctr, u);
  return tt < U ? fmaf(high[d] - low[d], u[0], low[d]) : fmaf(sqrtf(var[d]), std_normal(u[1], u[2]), mu[d]);
}

// uniform without replacement for a discrete space: partial Fisher-Yates over 0..A-1 (one
// thread); streams b * 4096 + 4000 + i
__device__ __forceinline__ void prop_perm(int* perm, int A, int U, int b, uint64_t seed, uint64_t ctr) {
  float u[4];
  for (int i = 0; i < A; ++i) perm[i] = i;
  for (int i = 0; i < U; ++i) {
    uniform4(seed, (uint64_t)b * 4096 + 4000 + i, ctr, u);
    const int jj = i + min((int)(u[0] * (float)(A - i)), A - i - 1);
    const int tmp = perm[i];
    perm[i] = perm[jj];
    perm[jj] = tmp;
  }
}

// softmax normalisers of the logits (every thread computes its own copy)
__device__ __forceinline__ void prop_softmax_norm(const float* mu, int A, float& mx, float& z) {
  mx = -INFINITY;
  for (int i = 0; i < A; ++i) mx = fmaxf(mx, mu[i]);
  z = 0.f;
  for (int i = 0; i < A; ++i) z += expf(mu[i] - mx);
}

// candidate tt of row b's discrete candidate set: the permutation prefix, then inverse-CDF
// categorical samples of softmax(logits); stream b * 4096 + tt
__device__ __forceinline__ float prop_sample_disc(int tt, int A, int U, int b, uint64_t seed, uint64_t ctr,
                                                  const int* perm, const float* mu, float mx, float z) {
  if (tt < U) return (float)perm[tt];
  float u[4];
  uniform4(seed, (uint64_t)b * 4096 + tt, ctr, u);
  const float target = u[0] * z;
  float c = 0.f;
  int k = A - 1;
  for (int i = 0; i < A; ++i) {
    c += expf(mu[i] - mx);
    if (c > target) { k = i; break; }
  }
  return (float)k;
}

// ------------------------------------------------------------------ vector envs (one wave per env)
// (The CartPole / Pendulum expressions are left to the compiler's contraction, as they always
// were: spelling them out would change what the stepwise envs compute.  That both callers get
// the same contraction is pinned by the rollout == stepwise tests on all three env kinds.)
__device__ __forceinline__ float env_normal(uint64_t seed, int e, int i, int kind, uint64_t ctr) {
  float u[4];
  uniform4(seed, ((uint64_t)kind << 48) | ((uint64_t)(uint32_t)e << 8) | (uint32_t)i, ctr, u);
  return std_normal(u[0], u[1]);
}
__device__ __forceinline__ float env_uniform(uint64_t seed, int e, int i, int kind, uint64_t ctr) {
  float u[4];
  uniform4(seed, ((uint64_t)kind << 48) | ((uint64_t)(uint32_t)e << 8) | (uint32_t)i, ctr, u);
  return u[2];
}

// reset draw of env e: new observation into o[0..obs) and the internal state into ph[0..4)
__device__ __forceinline__ void env_reset_state(int kind, uint64_t seed, int e, int lane, uint64_t ctr, float* o,
                                                float* ph) {
  if (kind == 0) {  // s ~ N(0, 0.1)
    if (lane < kBwObs) o[lane] = 0.1f * env_normal(seed, e, lane, 1, ctr);
  } else if (kind == 1) {  // CartPole: U(-0.05, 0.05)^4
    if (lane < 4) {
      const float v = -0.05f + 0.1f * env_uniform(seed, e, lane, 1, ctr);
      o[lane] = v;
      ph[lane] = v;
    }
  } else {  // Pendulum: th ~ U(-pi, pi), thdot ~ U(-1, 1)
    const float th = -3.14159265f + 6.2831853f * env_uniform(seed, e, 0, 1, ctr);
    const float thd = -1.f + 2.f * env_uniform(seed, e, 1, 1, ctr);
    if (lane == 0) {
      ph[0] = th;
      ph[1] = thd;
      o[0] = cosf(th);
      o[1] = sinf(th);
      o[2] = thd;
    }
  }
}

// dynamics of env e from observation s / internal state ph under action a_in (adim floats; the
// discrete envs' action index as a float): lane's component of s' in s2, the reward and the
// terminal flag (wave-uniform); ph is advanced in place
__device__ __forceinline__ void env_dynamics(const AqlEnv& V, int e, int lane, const float* s, float* ph,
                                             const float* a_in, uint64_t ctr, float& s2, float& r, bool& term) {
  s2 = 0.f;
  r = 0.f;
  term = false;
  if (V.kind == 0) {  // BipedalWalker-shaped (envs/classic.py BipedalWalkerShapedEnv.step)
    float a[kBwAct], pen = 0.f;
#pragma unroll
    for (int d = 0; d < kBwAct; ++d) {
      a[d] = fminf(fmaxf(a_in[d], -1.f), 1.f);
      pen += fabsf(a[d]);
    }
    if (lane < kBwObs) {
      float z = 0.01f * env_normal(V.seed, e, lane, 0, ctr);
      for (int k = 0; k < kBwObs; ++k) z = fmaf(V.dynA[lane * kBwObs + k], s[k], z);
#pragma unroll
      for (int d = 0; d < kBwAct; ++d) z = fmaf(V.dynB[lane * kBwAct + d], a[d], z);
      s2 = tanhf(z);
    }
    const float progress = 0.05f * wave_sum(lane < kBwObs ? V.dynw[lane] * s2 : 0.f);
    r = progress - 0.00035f * 80.f * pen;
    const float s0 = __shfl(s2, 0, 64);
    if (fabsf(s0) > 0.995f) {  // "hull touches ground"
      r = -100.f;
      term = true;
    }
  } else if (V.kind == 1) {  // CartPole (Barto et al. 1983; envs/classic.py CartPoleEnv)
    const float x = ph[0], xd = ph[1], th = ph[2], thd = ph[3];
    const float force = ((int)a_in[0] == 1) ? 10.f : -10.f;
    const float ct = cosf(th), sn = sinf(th);
    const float tmp = (force + 0.05f * thd * thd * sn) / 1.1f;
    const float tha = (9.8f * sn - ct * tmp) / (0.5f * (4.f / 3.f - 0.1f * ct * ct / 1.1f));
    const float xa = tmp - 0.05f * tha * ct / 1.1f;
    const float nv[4] = {x + 0.02f * xd, xd + 0.02f * xa, th + 0.02f * thd, thd + 0.02f * tha};
    if (lane < 4) s2 = nv[lane];
    r = 1.f;
    term = nv[0] < -2.4f || nv[0] > 2.4f || nv[2] < -0.20943951f || nv[2] > 0.20943951f;
    __builtin_amdgcn_wave_barrier();
    if (lane < 4) ph[lane] = nv[lane];
  } else {  // Pendulum (envs/classic.py PendulumEnv)
    const float th = ph[0], thd = ph[1];
    const float u = fminf(fmaxf(a_in[0], -2.f), 2.f);
    const float an = remainderf(th, 6.2831853f);  // normalised angle in [-pi, pi]
    const float cost = an * an + 0.1f * thd * thd + 0.001f * u * u;
    float nthd = thd + (-3.f * 10.f / 2.f * sinf(th + 3.14159265f) + 3.f * u) * 0.05f;
    const float nth = th + nthd * 0.05f;
    nthd = fminf(fmaxf(nthd, -8.f), 8.f);
    const float nv[3] = {cosf(nth), sinf(nth), nthd};
    if (lane < 3) s2 = nv[lane];
    r = -cost;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      ph[0] = nth;
      ph[1] = nthd;
    }
  }
}

// reset env e (one wave): new observation into obs_buf / phys
__device__ __forceinline__ void env_reset_one(const AqlEnv& V, int e, int lane, uint64_t ctr) {
  env_reset_state(V.kind, V.seed, e, lane, ctr, V.obs_buf + (size_t)e * V.obs, V.phys + (size_t)e * 4);
  if (lane == 0) {
    V.ep_len[e] = 0;
    V.ep_ret[e] = 0.f;
  }
}

// One env's step by one wave: dynamics, reward, the raw transition into replay slot `slot`,
// episode bookkeeping / reset.  `a`: this env's action vector (adim floats; the discrete envs'
// action index as a float), `aidx`: its candidate index.
__device__ __forceinline__ void env_step_wave(const AqlEnv& V, int e, int lane, const float* a_in, int aidx,
                                              const float* __restrict__ amu, const AqlInsert& I, int64_t slot,
                                              uint64_t ctr) {
  const int obs = V.obs;
  const float* s = V.obs_buf + (size_t)e * obs;
  float s2, r;
  bool term;
  env_dynamics(V, e, lane, s, V.phys + (size_t)e * 4, a_in, ctr, s2, r, term);
  const int len = V.ep_len[e] + 1;
  const bool done = term || len >= V.max_steps;  // TimeLimit sets done (stored as terminal)
  // raw transition into the replay ring
  if (lane < obs) {
    I.st[slot * obs + lane] = s[lane];
    I.st2[slot * obs + lane] = s2;
  }
  const int TA = V.T * V.adim;
  for (int k = lane; k < TA; k += 64) I.amu[slot * TA + k] = amu[(size_t)e * TA + k];
  if (lane == 0) {
    I.act[slot] = aidx;
    I.rew[slot] = r;
    I.done[slot] = done ? 1.f : 0.f;
    I.slots[e] = (int)slot;
  }
  __builtin_amdgcn_wave_barrier();
  if (done) {
    if (lane == 0) {
      const int k = atomicAdd(V.ep_count, 1);
      float* lg = V.ep_log + (size_t)(k % V.log_cap) * 2;
      lg[0] = V.ep_ret[e] + r;
      lg[1] = (float)len;
    }
    __builtin_amdgcn_wave_barrier();
    env_reset_one(V, e, lane, ctr);
  } else {
    if (lane < obs) V.obs_buf[(size_t)e * obs + lane] = s2;
    if (lane == 0) {
      V.ep_len[e] = len;
      V.ep_ret[e] += r;
    }
  }
}

}  // namespace aqld
}  // namespace apex
