// aql_host_eval_act: the act half of one greedy AQL evaluator step over HOST envs in ONE launch
// (gfx950).
//
// The stepwise form is aql_propose -> aql_candidate_q -> aql_select (eps 0) plus the counter add:
// four enqueues per evaluator step.  Here one 512-thread workgroup per evaluator env -- the loop
// body of aql_rollout_k without the env -- reads env b's observation from the `reset_obs` rows of
// the device copy of the vector env's staging block and does, in order: proposal MLP -> candidate
// set -> critic over the T candidates with the NoisyNet means (net.noisy = 0; mu + sigma * eps
// when the handle says so) -> first argmax (aql_select at eps 0).  It writes env_act[b] =
// cand[arg] and act_idx[b]; with the trace pointers (both or none) also the candidate set and its
// Q row.  Every per-state / per-candidate body is the __device__ function the stepwise kernels
// call (aql_dev.h) with the stepwise Philox keys -- proposal stream b * 4096 + e (discrete
// permutation b * 4096 + 4000 + i), selection stream b, counter = the evaluator step k -- so the
// outputs equal the stepwise ones bit for bit.
//
// `k` is passed by value (the evaluator launches eagerly and knows its step); thread 0 of
// workgroup 0 stores counter[0] = k + 1, the value the stepwise form's counter add leaves.  No
// thread of this kernel reads the counter, so the store cannot race.
//
// Where the data lives: aql_rollout_kernels.hip's split.  The critic's three matrices (odd pitches
// 129 / 65, read once per candidate with a lane-per-row pattern) and the small input layers
// (q.features, q_feature.0 at pitch obs | 1, action_out.0) are staged in LDS; dist_feature.0 / .2
// are read once per step through L2 as 16-byte loads; the candidate set and its Q row live in LDS
// (T <= 1024, T * (adim + 1) <= 4608 floats).  Two instances share the body.  Observations up to
// 24 wide (every env the project ships) leave room for four critic scratch rows per wave, and a
// wave scores four candidates per pass on every weight it reads (q_cand4, aql_frame_k's loop: the
// same fma chains, a third of the LDS cycles): 150,016 B.  Wider ones (up to 64) take the 49,920 B
// input-layer image of aql_rollout_k and its one-candidate loop (q_cand): 162,304 B.  Either way one
// workgroup per CU of the CU's 160 KiB, hence N <= 64.
//
// The weights may have moved since the last step (a refresh), and a launch keeps nothing, so the
// staging is per launch: about 130 KB per workgroup.  Every global load of the staging is issued
// before the first LDS store (aql_frame_k's finding: loop-by-loop staging waits out one global
// round trip per iteration), from clamped indices where the length is a runtime value.  Every
// barrier is workgroup-uniform (no data-dependent exit).  No workgroup writes a word another
// workgroup of the launch reads.
#include <stdexcept>

#include "aql_dev.h"
#include "common.h"
#include "kernels.h"

namespace apex {
namespace {

using namespace aqld;
constexpr int kEvThreads = 512, kEvWaves = kEvThreads / 64;
constexpr int kEvMaxT = 1024;        // candidates per step
constexpr int kEvCandFloats = 4608;  // LDS floats for a_mu [T][adim] + Q [T]
constexpr int kEvMaxAdim = 8;
constexpr int kEvMaxObs = 64;
constexpr int kEvWideObs = 24;       // up to here the small input layers leave room for the grouped critic
constexpr int kEvMaxN = 64;          // evaluator envs: one workgroup per env and CU

// kMaxObs: the widest observation the staged input layers hold; kGroup: candidates per critic pass
// of a wave -- 1 (q_cand, aql_rollout_k's loop) or 4 (q_cand4, aql_frame_k's loop: the same fma
// chains on every weight a wave reads, a third of the LDS cycles; 4x the per-wave scratch).
template <int kMaxObs, int kGroup>
__global__ __launch_bounds__(kEvThreads) void aql_host_eval_act_k(AqlHostEvalAct R) {
  constexpr int kScr = kGroup * 192;    // per-wave critic scratch: hb [128][kGroup] | xb [64][kGroup]
  __shared__ float w1s[kH * kPitch];    // advantage1 effective weight [64][128]
  __shared__ float ao2s[kH * kPitch];   // action_out.2 [64][128] (continuous)
  __shared__ float qf2s[kH * kQf2Pitch];
  __shared__ float fq[(kCat + kH) * (kMaxObs | 1)];  // q.features [128][obs] | q_feature.0 [64][obs] at pitch obs | 1
  __shared__ float ao1[kCat * kEvMaxAdim];  // action_out.0 [128 | 64][adim]
  __shared__ float cq[kEvCandFloats];       // a_mu [T][adim] | Q [T]
  // proposal phase: emb [128] | hid [128] | mu [64] | perm [64]; critic phase: kScr floats per wave
  __shared__ __attribute__((aligned(16))) float scr[kEvWaves * kScr];
  __shared__ float s_b1[kH], s_w2[kH], s_sadv[kH], s_obs[kMaxObs];
  const AQLNet& net = R.net;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int obs = net.obs, adim = net.adim, T = net.T, A = net.na, U = net.uniform, cont = net.cont;
  const int p = obs | 1;
  const uint64_t ctr = (uint64_t)R.k;
  float* fw = fq;
  float* qf1 = fq + kCat * p;
  float* cand = cq;
  float* qs = cq + T * adim;
  float* emb = scr;
  float* hid = scr + kCat;
  float* mu = scr + 2 * kCat;
  int* perm = reinterpret_cast<int*>(scr + 2 * kCat + 64);
  if (b == 0 && tid == 0) R.counter[0] = R.k + 1;
  // ---- stage (per launch): every load first, then the LDS stores
  {
    constexpr int K1 = kH * kCat / kEvThreads, K2 = kH * kH / kEvThreads;  // 16, 8
    constexpr int KF = (kCat * kMaxObs + kEvThreads - 1) / kEvThreads;      // 16 | 6
    constexpr int KQ = (kH * kMaxObs + kEvThreads - 1) / kEvThreads;        // 8 | 3
    constexpr int KA = kCat * kEvMaxAdim / kEvThreads;                      // 2
    const int nf = kCat * obs, nq = kH * obs, na1 = (cont ? kCat : kH) * adim;
    float m[K1], av[K1], q2[K2], f1[KF], f2[KQ], a1v[KA];
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      const int e = tid + kEvThreads * k;
      m[k] = noisy_eff_val(net, e);
      av[k] = cont ? net.ao_w2[e] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < K2; ++k) q2[k] = net.qf_w2[tid + kEvThreads * k];
#pragma unroll
    for (int k = 0; k < KF; ++k) f1[k] = net.f_w[min(tid + kEvThreads * k, nf - 1)];
#pragma unroll
    for (int k = 0; k < KQ; ++k) f2[k] = net.qf_w1[min(tid + kEvThreads * k, nq - 1)];
#pragma unroll
    for (int k = 0; k < KA; ++k) a1v[k] = net.ao_w1[min(tid + kEvThreads * k, na1 - 1)];
    const float ob = R.stage[(size_t)(R.N + b) * obs + min(tid, obs - 1)];  // reset_obs row b
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      const int e = tid + kEvThreads * k, r = e >> 7, c = e & 127;
      w1s[r * kPitch + c] = m[k];
      if (cont) ao2s[r * kPitch + c] = av[k];
    }
#pragma unroll
    for (int k = 0; k < K2; ++k) {
      const int e = tid + kEvThreads * k;
      qf2s[(e >> 6) * kQf2Pitch + (e & 63)] = q2[k];
    }
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      const int e = tid + kEvThreads * k;
      if (e < nf) fw[(e / obs) * p + e % obs] = f1[k];
    }
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
      const int e = tid + kEvThreads * k;
      if (e < nq) qf1[(e / obs) * p + e % obs] = f2[k];
    }
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      const int e = tid + kEvThreads * k;
      if (e < na1) ao1[e] = a1v[k];
    }
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
  // ---- the candidate set
  if (cont) {
    for (int e = tid; e < T * A; e += kEvThreads)
      cand[e] = prop_sample_cont(e, A, U, b, R.prop_seed, ctr, R.low, R.high, R.var, mu);
  } else {
    if (tid == 0) prop_perm(perm, A, U, b, R.prop_seed, ctr);
    __syncthreads();
    float mx, z;
    prop_softmax_norm(mu, A, mx, z);
    for (int tt = tid; tt < T; tt += kEvThreads)
      cand[tt] = prop_sample_disc(tt, A, U, b, R.prop_seed, ctr, perm, mu, mx, z);
  }
  __syncthreads();  // (the proposal scratch is free from here: the critic's waves reuse it)
  if (R.amu)
    for (int e = tid; e < T * adim; e += kEvThreads) R.amu[(size_t)b * T * adim + e] = cand[e];
  // ---- the critic over the T candidates (wave w: candidates w, w + 8, ...; grouped: four at a
  // time, and past T a pass recomputes candidate T - 1 and drops it)
  {
    float* hb = scr + wave * kScr;
    const float sadv = s_sadv[lane];
    if constexpr (kGroup == 1) {
      for (int c = wave; c < T; c += kEvWaves) {
        const float qv = q_cand(net, ao1, adim, cand + c * adim, w1s, ao2s, s_w2, b2eff, sadv, hb, hb + kCat, lane);
        if (lane == 0) qs[c] = qv;
      }
    } else {
      for (int c0 = wave; c0 < T; c0 += kGroup * kEvWaves) {
        const float* ac[kGroup];
#pragma unroll
        for (int g = 0; g < kGroup; ++g) ac[g] = cand + min(c0 + g * kEvWaves, T - 1) * adim;
        float qv[kGroup];
        q_cand4(net, ao1, adim, ac, w1s, ao2s, s_w2, b2eff, sadv, hb, hb + kGroup * kCat, lane, qv);
#pragma unroll
        for (int g = 0; g < kGroup; ++g)
          if (lane == 0 && c0 + g * kEvWaves < T) qs[c0 + g * kEvWaves] = qv[g];
      }
    }
  }
  __syncthreads();
  if (R.q)
    for (int c = tid; c < T; c += kEvThreads) R.q[(size_t)b * T + c] = qs[c];
  // ---- greedy selection (aql_select at eps 0)
  if (wave == 0) {
    const int arg = select_cand(qs, T, 0.f, R.sel_seed, b, ctr, lane);
    if (lane < adim) R.env_act[b * adim + lane] = cand[arg * adim + lane];
    if (lane == 0) R.act_idx[b] = arg;
  }
}

}  // namespace

// Limits: 1 <= N <= 64 evaluator envs, obs / actions 1..64, action dim 1..8, and the candidate
// set must fit the kernel's LDS layout: T <= 1024 and T * (adim + 1) <= 4608 floats.  There is no
// env kind: any observation / action shape within the limits is taken.
void aql_host_eval_act(const AqlHostEvalAct& R, hipStream_t s) {
  const AQLNet& n = R.net;
  if (R.N < 1 || R.N > kEvMaxN) throw std::invalid_argument("aql_host_eval_act: 1 <= N <= 64 (one workgroup per env and CU)");
  if (R.k < 0) throw std::invalid_argument("aql_host_eval_act: step k >= 0");
  if (n.obs < 1 || n.obs > kEvMaxObs) throw std::invalid_argument("aql_host_eval_act: 1 <= obs <= 64");
  if (n.na < 1 || n.na > 64) throw std::invalid_argument("aql_host_eval_act: 1 <= actions <= 64");
  if (n.adim < 1 || n.adim > kEvMaxAdim) throw std::invalid_argument("aql_host_eval_act: 1 <= action dim <= 8");
  if (n.cont ? n.na != n.adim : n.adim != 1)
    throw std::invalid_argument("aql_host_eval_act: action dim = actions (continuous) / 1 (discrete)");
  if (!n.cont && n.uniform > n.na) throw std::invalid_argument("aql_host_eval_act: uniform > actions (discrete)");
  if (n.uniform < 0 || n.uniform > n.T) throw std::invalid_argument("aql_host_eval_act: 0 <= uniform <= T");
  if (n.T < 1 || n.T > kEvMaxT || n.T * (n.adim + 1) > kEvCandFloats)
    throw std::invalid_argument("aql_host_eval_act: the candidate set must fit LDS: T <= 1024 and T * (adim + 1) <= 4608");
  if (!R.stage) throw std::invalid_argument("aql_host_eval_act: the staging block's device copy");
  if (!R.env_act || !R.act_idx || !R.counter) throw std::invalid_argument("aql_host_eval_act: null outputs");
  if ((R.amu != nullptr) != (R.q != nullptr)) throw std::invalid_argument("aql_host_eval_act: both trace pointers or none");
  if (!n.qf_w1 || !n.qf_b1 || !n.qf_w2 || !n.qf_b2 || !n.ao_w1 || !n.ao_b1 || !n.a1_wmu || !n.a1_bmu || !n.a2_wmu ||
      !n.a2_bmu || !n.f_w || !n.f_b || !n.df_w1 || !n.df_b1 || !n.df_w2 || !n.df_b2 ||
      (n.cont && (!n.ao_w2 || !n.ao_b2)) ||
      (n.noisy && (!n.a1_wsig || !n.a1_weps || !n.a1_bsig || !n.a1_beps || !n.a2_wsig || !n.a2_weps || !n.a2_bsig ||
                   !n.a2_beps)))
    throw std::invalid_argument("aql_host_eval_act: missing weights");
  if (reinterpret_cast<uintptr_t>(n.df_w1) & 15)
    throw std::invalid_argument("aql_host_eval_act: dist_feature.0 must be 16-byte aligned (flatten with align=4)");
  if (n.cont && (!R.low || !R.high || !R.var)) throw std::invalid_argument("aql_host_eval_act: action bounds / variance");
  if (n.obs <= kEvWideObs)
    aql_host_eval_act_k<kEvWideObs, 4><<<R.N, kEvThreads, 0, s>>>(R);
  else
    aql_host_eval_act_k<kEvMaxObs, 1><<<R.N, kEvThreads, 0, s>>>(R);
  LAUNCH_CHECK();
}

}  // namespace apex
