// aql_frame: one env's whole acting frame of the single-process AQL trainer (reference
// AQL.py:113-125) in ONE launch (gfx950).
//
// The stepwise sequence costs five launches per frame for one env: aql_propose -> aql_noisy_eff +
// aql_candidate_q -> aql_select -> aql_env_step -> per_write_leaves, plus the host's epsilon and
// beta writes.  Here one 512-thread workgroup -- one loop body of aql_rollout_k -- reads the frame
// counter t on the device and does, in order:
//
//   1. stage what the critic reads once per candidate into LDS.  The online weights change every
//      frame (one SGD step per frame), so the staging is per launch; the effective NoisyLinear
//      weights are mu + sigma * eps of the ONLINE net (train mode: AQL.py acts with the net it
//      trains, noise applied).
//   2. proposal MLP on the current observation -> the candidate set with aql_propose's Philox
//      keys (env 0: stream e, discrete permutation 4000 + i, counter t) -> the critic over the T
//      candidates (8 waves, candidate c on wave c mod 8).
//   3. this frame's epsilon, then aql_select's draw and first argmax (stream 0 of sel_seed at t).
//   4. the env step with env_step_wave (aql_dev.h): the raw transition and its candidate set into
//      slot `filled mod C`, episode bookkeeping / reset (TimeLimit stored as done), episode log.
//   5. that slot's leaf at max_prio^alpha and every level of its path (sum and min); filled += 1.
//   6. the learner's beta(t) = min(1, beta0 + t (1 - beta0) / max_step) in fp64; t += 1.
//
// The epsilon stream.  AQL.py:116 draws `0.5 if random.random() > 0.1 else 0.05` per frame.  Here
// frame t draws u = uniform4(eps_seed, stream 0, counter t)[0] -- a Philox key of its own
// (eps_seed), so the draw is independent of the selection's (sel_seed) and the proposal's
// (prop_seed) -- and epsilon = u > eps_p ? eps_hi : eps_lo with (eps_hi, eps_lo, eps_p) =
// (0.5, 0.05, 0.1).  u is a 24-bit uniform in [0, 1) and eps_p is compared as fp32.
// aql_frame_eps is the same draw as a launch of its own (the launch-by-launch yardstick).
//
// Where the data lives: the split of aql_rollout_kernels.hip.  The critic's three matrices are
// read once per CANDIDATE with a lane-per-row pattern (odd pitches 129 / 65: conflict-free) and
// are LDS-resident; the small first layers (q.features, q_feature.0, action_out.0) are staged
// because a runtime-length loop of dependent global loads pays an L2 round trip per input; the
// proposal's dist_feature.0 / .2 are read once per frame and go through L2 (thread j reads its
// row as independent 16-byte loads).  The candidate set and its Q row stay in LDS (T <= 1024,
// T * (adim + 1) <= 4608 floats).  ~150 KB of LDS: one workgroup per CU, and there is only one.
// The critic pass is bound by LDS reads (a lane-per-row dot product reads one weight and one
// activation per fma), so a wave scores four candidates per pass on every weight it reads
// (q_cand4, aql_dev.h): the same fma chains, a third of the LDS cycles.
// Every barrier is workgroup-uniform (no data-dependent exit).  Global writes: the replay row,
// the tree path, the env state / episode log, the counters, beta, and the five small outputs
// (selected index, action, epsilon, reward, done) -- plus the Q row when q_out is given (tests).
#include <stdexcept>

#include "aql_dev.h"
#include "common.h"
#include "kernels.h"
#include "tree_dev.h"

namespace apex {
namespace {

using namespace aqld;
constexpr int kFrThreads = 512, kFrWaves = kFrThreads / 64;
constexpr int kFrMaxT = 1024;        // candidates
constexpr int kFrCandFloats = 4608;  // LDS floats for a_mu [T][adim] + Q [T]
constexpr int kFrMaxAdim = 8;
constexpr int kGroup = 4;            // candidates per critic pass of a wave (q_cand4)
constexpr int kScr = kGroup * 192;   // per-wave critic scratch: hb [128][4] | xb [64][4]
constexpr int kFrMaxObs = 24;        // the device envs' widest observation (BipedalWalker-shaped)
constexpr int kFrObsPitch = kFrMaxObs | 1;

__device__ __forceinline__ float frame_eps(uint64_t seed, uint64_t t, float hi, float lo, float p) {
  float u[4];
  uniform4(seed, 0ull, t, u);
  return u[0] > p ? hi : lo;
}

__global__ __launch_bounds__(kFrThreads) void aql_frame_k(AqlFrame F) {
  __shared__ float w1s[kH * kPitch];    // advantage1 effective weight [64][128]
  __shared__ float ao2s[kH * kPitch];   // action_out.2 [64][128] (continuous)
  __shared__ float qf2s[kH * kQf2Pitch];
  __shared__ float fq[(kCat + kH) * kFrObsPitch];  // q.features [128][obs] | q_feature.0 [64][obs] at pitch obs | 1
  __shared__ float ao1[kCat * kFrMaxAdim];  // action_out.0 [128 | 64][adim]
  __shared__ float cq[kFrCandFloats];       // a_mu [T][adim] | Q [T]
  // proposal phase: emb [128] | hid [128] | mu [64] | perm [64]; critic phase: kScr floats per wave
  __shared__ __attribute__((aligned(16))) float scr[kFrWaves * kScr];
  __shared__ float s_b1[kH], s_w2[kH], s_sadv[kH], s_obs[64];
  __shared__ int sids[1];
  const AQLNet& net = F.net;
  const AqlEnv& V = F.V;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int obs = net.obs, adim = net.adim, T = net.T, A = net.na, U = net.uniform, cont = net.cont;
  const int p = obs | 1;
  // both counters are read by every thread here and advanced by thread 0 behind the last barrier
  const int64_t step = F.t[0];
  const int64_t filled = F.filled[0];
  const uint64_t ctr = (uint64_t)step;
  const int64_t slot = filled % F.I.C;
  float* fw = fq;
  float* qf1 = fq + kCat * p;
  float* cand = cq;
  float* qs = cq + T * adim;
  float* emb = scr;
  float* hid = scr + kCat;
  float* mu = scr + 2 * kCat;
  int* perm = reinterpret_cast<int*>(scr + 2 * kCat + 64);
  // ---- stage (per launch: the weights moved since the last frame).  Every load is issued
  // before the first LDS store: loop-by-loop staging waited out one global round trip per
  // iteration (16 for the two 64x128 matrices).  Unconditional loads from clamped indices.
  {
    constexpr int K1 = kH * kCat / kFrThreads, K2 = kH * kH / kFrThreads;  // 16, 8
    constexpr int KF = (kCat * kFrMaxObs + kFrThreads - 1) / kFrThreads;   // 6
    constexpr int KQ = (kH * kFrMaxObs + kFrThreads - 1) / kFrThreads;     // 3
    const int nf = kCat * obs, nq = kH * obs, na1 = (cont ? kCat : kH) * adim;  // na1 <= 512
    float m[K1], sg[K1], ep[K1], av[K1], q2[K2], f1[KF], f2[KQ];
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      const int e = tid + kFrThreads * k;
      m[k] = net.a1_wmu[e];
      sg[k] = net.a1_wsig[e];
      ep[k] = net.a1_weps[e];
      av[k] = cont ? net.ao_w2[e] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < K2; ++k) q2[k] = net.qf_w2[tid + kFrThreads * k];
#pragma unroll
    for (int k = 0; k < KF; ++k) f1[k] = net.f_w[min(tid + kFrThreads * k, nf - 1)];
#pragma unroll
    for (int k = 0; k < KQ; ++k) f2[k] = net.qf_w1[min(tid + kFrThreads * k, nq - 1)];
    const float a1v = net.ao_w1[min(tid, na1 - 1)];
    const float ob = V.obs_buf[min(tid, obs - 1)];
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      const int e = tid + kFrThreads * k, r = e >> 7, c = e & 127;
      w1s[r * kPitch + c] = fmaf(sg[k], ep[k], m[k]);  // (noisy_eff_val, train mode)
      if (cont) ao2s[r * kPitch + c] = av[k];
    }
#pragma unroll
    for (int k = 0; k < K2; ++k) {
      const int e = tid + kFrThreads * k;
      qf2s[(e >> 6) * kQf2Pitch + (e & 63)] = q2[k];
    }
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      const int e = tid + kFrThreads * k;
      if (e < nf) fw[(e / obs) * p + e % obs] = f1[k];
    }
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
      const int e = tid + kFrThreads * k;
      if (e < nq) qf1[(e / obs) * p + e % obs] = f2[k];
    }
    if (tid < na1) ao1[tid] = a1v;
    if (tid < obs) s_obs[tid] = ob;
  }
  if (tid < kH) {
    s_b1[tid] = noisy_eff_val(net, kH * kCat + tid);
    s_w2[tid] = noisy_eff_val(net, kH * kCat + kH + tid);
  }
  const float b2eff = noisy_eff_val(net, kH * kCat + 2 * kH);
  __syncthreads();
  // ---- state embedding (threads 0..127) beside the critic's state half (wave 2)
  if (tid < kCat) {
    emb[tid] = prop_embed(fw + tid * p, s_obs, obs, net.f_b[tid]);
  } else if (wave == 2) {
    float* sb = scr + 2 * kScr;
    s_sadv[lane] = q_state(qf1, p, net.qf_b1, net.qf_b2, s_obs, obs, qf2s, w1s, s_b1, sb, sb + kH, lane);
  }
  __syncthreads();
  if (tid < kCat) {
    const float* const e1[1] = {emb};
    float h1[1];
    prop_hidden<1>(net.df_w1 + (size_t)tid * kCat, e1, net.df_b1[tid], h1);
    hid[tid] = h1[0];
  }
  __syncthreads();
  if (tid < A) mu[tid] = prop_out(net.df_w2 + (size_t)tid * kCat, hid, net.df_b2[tid]);
  __syncthreads();
  // ---- the candidate set (env index 0, counter t)
  if (cont) {
    for (int e = tid; e < T * A; e += kFrThreads)
      cand[e] = prop_sample_cont(e, A, U, 0, F.prop_seed, ctr, F.low, F.high, F.var, mu);
  } else {
    if (tid == 0) prop_perm(perm, A, U, 0, F.prop_seed, ctr);
    __syncthreads();
    float mx, z;
    prop_softmax_norm(mu, A, mx, z);
    for (int tt = tid; tt < T; tt += kFrThreads)
      cand[tt] = prop_sample_disc(tt, A, U, 0, F.prop_seed, ctr, perm, mu, mx, z);
  }
  __syncthreads();  // (the proposal scratch is free from here: the critic's waves reuse it)
  // ---- the critic over the T candidates: wave w takes candidates w, w + 8, ... four at a time
  // (q_cand4; past T a pass recomputes candidate T - 1 and drops it)
  {
    float* hb = scr + wave * kScr;
    const float sadv = s_sadv[lane];
    for (int c0 = wave; c0 < T; c0 += kGroup * kFrWaves) {
      const float* ac[kGroup];
#pragma unroll
      for (int g = 0; g < kGroup; ++g) ac[g] = cand + min(c0 + g * kFrWaves, T - 1) * adim;
      float qv[kGroup];
      q_cand4(net, ao1, adim, ac, w1s, ao2s, s_w2, b2eff, sadv, hb, hb + kGroup * kCat, lane, qv);
#pragma unroll
      for (int g = 0; g < kGroup; ++g)
        if (lane == 0 && c0 + g * kFrWaves < T) qs[c0 + g * kFrWaves] = qv[g];
    }
  }
  __syncthreads();
  if (F.q_out)
    for (int c = tid; c < T; c += kFrThreads) F.q_out[c] = qs[c];
  // ---- this frame's epsilon, the selection, the env step and the insert (wave 0)
  if (wave == 0) {
    const float eps = frame_eps(F.eps_seed, ctr, F.eps_hi, F.eps_lo, F.eps_p);
    const int arg = select_cand(qs, T, eps, F.sel_seed, 0, ctr, lane);
    if (lane < adim) F.env_act[lane] = cand[arg * adim + lane];
    env_step_wave(V, 0, lane, cand + arg * adim, arg, cand, F.I, slot, ctr);
    if (lane == 0) {
      F.act_idx[0] = arg;
      F.eps_out[0] = eps;
      F.reward[0] = F.I.rew[slot];
      F.done[0] = F.I.done[slot];
      // insert at the running max priority (write_leaf's "no priority given"); max_prio stays
      write_leaf(F.tree, (int)slot, F.max_prio[0], F.alpha);
      sids[0] = (int)slot;
    }
  }
  update_levels_block(F.tree, sids, 1, 1, F.tree.levels);  // (each level begins with a barrier)
  if (tid == 0) {
#pragma clang fp contract(off)
    const double st = (double)step;  // AQL.py beta_by_frame in the host's double arithmetic, then to fp32
    const double b = F.beta0 + st * (1.0 - F.beta0) / F.beta_max_step;
    F.beta_out[0] = (float)(b < 1.0 ? b : 1.0);
    F.filled[0] = filled + 1;
    F.t[0] = step + 1;
  }
}

__global__ void aql_frame_eps_k(uint64_t seed, const int64_t* __restrict__ t, float hi, float lo, float p,
                                float* __restrict__ eps_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) eps_out[0] = frame_eps(seed, (uint64_t)t[0], hi, lo, p);
}

}  // namespace

// Limits: obs / actions as aql_propose (1..64), action dim <= 8, and the candidate set must fit
// the kernel's LDS layout: T <= 1024 and T * (adim + 1) <= 4608 floats (as aql_rollout).
void aql_frame(const AqlFrame& F, hipStream_t s) {
  static const int obs_of[3] = {kBwObs, 4, 3}, adim_of[3] = {kBwAct, 1, 1}, cont_of[3] = {1, 0, 1};
  const AQLNet& n = F.net;
  const AqlEnv& V = F.V;
  if (V.kind < 0 || V.kind > 2) throw std::invalid_argument("aql_frame: kind 0 (bipedal) / 1 (cartpole) / 2 (pendulum)");
  if (V.E != 1) throw std::invalid_argument("aql_frame: one env");
  if (n.obs < 1 || n.obs > 64) throw std::invalid_argument("aql_frame: 1 <= obs <= 64");
  if (n.na < 1 || n.na > 64) throw std::invalid_argument("aql_frame: 1 <= actions <= 64");
  if (n.adim < 1 || n.adim > kFrMaxAdim) throw std::invalid_argument("aql_frame: 1 <= action dim <= 8");
  if (!n.cont && n.uniform > n.na) throw std::invalid_argument("aql_frame: uniform > actions (discrete)");
  if (n.uniform < 0 || n.uniform > n.T) throw std::invalid_argument("aql_frame: 0 <= uniform <= T");
  if (n.T < 1 || n.T > kFrMaxT || n.T * (n.adim + 1) > kFrCandFloats)
    throw std::invalid_argument("aql_frame: the candidate set must fit LDS: T <= 1024 and T * (adim + 1) <= 4608");
  static_assert(kBwObs <= kFrMaxObs && kBwAct * kCat <= kFrThreads, "the staging covers the device envs' shapes");
  if (n.obs != obs_of[V.kind] || n.adim != adim_of[V.kind] || (n.cont != 0) != (cont_of[V.kind] != 0) ||
      (n.cont && n.na != n.adim) || V.obs != n.obs || V.adim != n.adim || V.T != n.T)
    throw std::invalid_argument("aql_frame: the net's / env's obs / action dims do not match the env kind");
  if (!n.noisy) throw std::invalid_argument("aql_frame: acting is the train-mode net (noisy = 1)");
  if (!n.qf_w1 || !n.qf_b1 || !n.qf_w2 || !n.qf_b2 || !n.ao_w1 || !n.ao_b1 || !n.a1_wmu || !n.a1_bmu || !n.a2_wmu ||
      !n.a2_bmu || !n.f_w || !n.f_b || !n.df_w1 || !n.df_b1 || !n.df_w2 || !n.df_b2 ||
      (n.cont && (!n.ao_w2 || !n.ao_b2)) || !n.a1_wsig || !n.a1_weps || !n.a1_bsig || !n.a1_beps || !n.a2_wsig ||
      !n.a2_weps || !n.a2_bsig || !n.a2_beps)
    throw std::invalid_argument("aql_frame: missing weights");
  if (reinterpret_cast<uintptr_t>(n.df_w1) & 15)
    throw std::invalid_argument("aql_frame: dist_feature.0 must be 16-byte aligned (flatten with align=4)");
  if (n.cont && (!F.low || !F.high || !F.var)) throw std::invalid_argument("aql_frame: action bounds / variance");
  if (V.kind == 0 && (!V.dynA || !V.dynB || !V.dynw)) throw std::invalid_argument("aql_frame: dynamics matrices");
  if (V.max_steps < 1 || V.log_cap < 1 || !V.obs_buf || !V.phys || !V.ep_len || !V.ep_ret || !V.ep_count || !V.ep_log)
    throw std::invalid_argument("aql_frame: env buffers");
  const AqlInsert& I = F.I;
  if (!I.st || !I.st2 || !I.rew || !I.done || !I.amu || !I.act || !I.slots || I.C < 1)
    throw std::invalid_argument("aql_frame: replay tables");
  if (I.C > ((int64_t)1 << 31) - 1 || F.tree.size[0] < I.C || F.tree.levels < 1)
    throw std::invalid_argument("aql_frame: the tree must cover the ring");
  if (!F.t || !F.filled || (const void*)F.filled != (const void*)I.filled || (const void*)F.t != (const void*)V.counter)
    throw std::invalid_argument("aql_frame: t / filled must be the env's counter and the ring's fill count");
  if (!F.max_prio || !F.beta_out || !F.act_idx || !F.env_act || !F.eps_out || !F.reward || !F.done)
    throw std::invalid_argument("aql_frame: missing buffers");
  if (!(F.beta_max_step > 0.0)) throw std::invalid_argument("aql_frame: the beta horizon must be > 0");
  aql_frame_k<<<1, kFrThreads, 0, s>>>(F);
  LAUNCH_CHECK();
}

void aql_frame_eps(uint64_t eps_seed, const int64_t* t, float eps_hi, float eps_lo, float eps_p, float* eps_out,
                   hipStream_t s) {
  if (!t || !eps_out) throw std::invalid_argument("aql_frame_eps: counter / output");
  aql_frame_eps_k<<<1, 64, 0, s>>>(eps_seed, t, eps_hi, eps_lo, eps_p, eps_out);
  LAUNCH_CHECK();
}

}  // namespace apex
