// aql_rollout: N greedy AQL episodes from reset to their first done in ONE launch (gfx950).
//
// The stepwise evaluator (AQLEngine.evaluate) pays five launches per env step: aql_propose ->
// aql_noisy_eff + aql_candidate_q -> aql_select (eps 0) -> aql_env_step, plus the torch ops that
// accumulate the returns.  Here one 512-thread workgroup plays one episode: it stages the
// weights once, then loops  proposal MLP -> candidate sampling (Philox) -> critic over the T
// candidates -> first argmax -> env step  until the episode's first done or max_steps.  Every
// per-state / per-candidate / per-env body is the __device__ function the stepwise kernels
// call (aql_dev.h) with the stepwise Philox keys -- proposal stream b * 4096 + e (discrete
// permutation b * 4096 + 4000 + i) and selection stream b at counter t = 0, 1, ...; env noise /
// reset streams of env_normal / env_uniform, the first reset at counter 0xFFFFFFFF -- so the
// returns equal the stepwise evaluator's bit for bit.
//
// Where the data lives.  LDS is 160 KiB per CU and a workgroup may take all of it.  The critic's
// three matrices (advantage1 effective weight and action_out.2 at pitch 129, q_feature.2 at
// pitch 65: 82,688 B) are read once per CANDIDATE, T times per step, with a lane-per-row
// pattern that only an odd LDS pitch serves without conflicts: they are LDS-resident.  The
// proposal's matrices are read once per STEP.  Its big one, dist_feature.0 [128][128] (67,584 B
// at its staged pitch), does not fit beside the critic and the candidate set, so thread j reads
// its row j through L2 as 32 independent 16-byte loads (the 64 KB stay in the XCD's L2 between
// steps); dist_feature.2 [na][128] likewise (na lanes, 16 loads in flight).  What a
// runtime-length loop of dependent global loads would read -- q.features [128][obs],
// q_feature.0 [64][obs] and action_out.0 [128][adim]; one L2 round trip per input otherwise --
// is small (<= 49,920 + 4,096 B) and is staged.  The candidate set and its Q row live in LDS
// too (18,432 B: T * (adim + 1) <= 4608 floats), so nothing but the trace and the three results
// is ever written to global memory.  Total 162,336 B: one workgroup per CU.
//
// One episode per workgroup: every barrier is workgroup-uniform by construction (the loop exit
// is a flag in LDS read after a barrier), episodes of different lengths never wait for each
// other, and N <= 1024 workgroups of 8 waves fill the chip for the larger N.  Eight waves
// share the T candidates of a step (wave w: candidates w, w + 8, ...); the proposal MLP runs on
// 128 threads (its dot products are sequential chains, as in aql_propose_k) beside the state half
// of the critic on wave 2.
#include <stdexcept>

#include "aql_dev.h"
#include "common.h"
#include "kernels.h"

namespace apex {
namespace {

using namespace aqld;
constexpr int kRollThreads = 512, kRollWaves = kRollThreads / 64;
constexpr int kRollMaxT = 1024;        // candidates per step
constexpr int kRollCandFloats = 4608;  // LDS floats for a_mu [T][adim] + Q [T]
constexpr int kRollMaxAdim = 8;
constexpr int kScr = 192;              // per-wave critic scratch: hb [128] | xb [64]

__global__ __launch_bounds__(kRollThreads) void aql_rollout_k(AqlRollout R) {
  __shared__ float w1s[kH * kPitch];    // advantage1 effective weight [64][128]
  __shared__ float ao2s[kH * kPitch];   // action_out.2 [64][128] (continuous)
  __shared__ float qf2s[kH * kQf2Pitch];
  __shared__ float fq[(kCat + kH) * 65];  // q.features [128][obs] | q_feature.0 [64][obs] at pitch obs | 1
  __shared__ float ao1[kCat * kRollMaxAdim];  // action_out.0 [128 | 64][adim]
  __shared__ float cq[kRollCandFloats];       // a_mu [T][adim] | Q [T]
  // proposal phase: emb [128] | hid [128] | mu [64] | perm [64]; critic phase: kScr floats per wave
  __shared__ __attribute__((aligned(16))) float scr[kRollWaves * kScr];
  __shared__ float s_b1[kH], s_w2[kH], s_sadv[kH], s_obs[64], s_phys[4];
  __shared__ int s_done;
  const AQLNet& net = R.net;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int obs = net.obs, adim = net.adim, T = net.T, A = net.na, U = net.uniform, cont = net.cont;
  const int p = obs | 1;
  float* fw = fq;
  float* qf1 = fq + kCat * p;
  float* cand = cq;
  float* qs = cq + T * adim;
  float* emb = scr;
  float* hid = scr + kCat;
  float* mu = scr + 2 * kCat;
  int* perm = reinterpret_cast<int*>(scr + 2 * kCat + 64);
  // ---- stage once per workgroup
  for (int e = tid; e < kH * kCat; e += kRollThreads) {
    const int r = e >> 7, c = e & 127;
    w1s[r * kPitch + c] = noisy_eff_val(net, e);
    if (cont) ao2s[r * kPitch + c] = net.ao_w2[e];
  }
  for (int e = tid; e < kH * kH; e += kRollThreads) qf2s[(e >> 6) * kQf2Pitch + (e & 63)] = net.qf_w2[e];
  for (int e = tid; e < kCat * obs; e += kRollThreads) fw[(e / obs) * p + e % obs] = net.f_w[e];
  for (int e = tid; e < kH * obs; e += kRollThreads) qf1[(e / obs) * p + e % obs] = net.qf_w1[e];
  for (int e = tid; e < (cont ? kCat : kH) * adim; e += kRollThreads) ao1[e] = net.ao_w1[e];
  if (tid < kH) {
    s_b1[tid] = noisy_eff_val(net, kH * kCat + tid);
    s_w2[tid] = noisy_eff_val(net, kH * kCat + kH + tid);
  }
  const float b2eff = noisy_eff_val(net, kH * kCat + 2 * kH);
  if (wave == 0) env_reset_state(R.kind, R.env_seed, b, lane, 0xFFFFFFFFull, s_obs, s_phys);
  AqlEnv V{};
  V.kind = R.kind;
  V.seed = R.env_seed;
  V.dynA = R.dynA;
  V.dynB = R.dynB;
  V.dynw = R.dynw;
  float ret = 0.f;
  int len = 0;
  __syncthreads();
  for (int t = 0; t < R.max_steps; ++t) {
    const uint64_t ctr = (uint64_t)t;
    const bool tr = R.trace_obs != nullptr && t < R.trace_T;  // workgroup-uniform
    const size_t trow = (size_t)b * R.trace_T + t;
    // ---- state embedding (threads 0..127) beside the critic's state half (wave 2)
    if (tid < kCat) {
      emb[tid] = prop_embed(fw + tid * p, s_obs, obs, net.f_b[tid]);
    } else if (wave == 2) {
      float* sb = scr + 2 * kScr;
      s_sadv[lane] = q_state(qf1, p, net.qf_b1, net.qf_b2, s_obs, obs, qf2s, w1s, s_b1, sb, sb + kH, lane);
    } else if (tr && tid - 192 < obs) {
      R.trace_obs[trow * obs + (tid - 192)] = s_obs[tid - 192];
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
      for (int e = tid; e < T * A; e += kRollThreads)
        cand[e] = prop_sample_cont(e, A, U, b, R.prop_seed, ctr, R.low, R.high, R.var, mu);
    } else {
      if (tid == 0) prop_perm(perm, A, U, b, R.prop_seed, ctr);
      __syncthreads();
      float mx, z;
      prop_softmax_norm(mu, A, mx, z);
      for (int tt = tid; tt < T; tt += kRollThreads)
        cand[tt] = prop_sample_disc(tt, A, U, b, R.prop_seed, ctr, perm, mu, mx, z);
    }
    __syncthreads();  // (the proposal scratch is free from here: the critic's waves reuse it)
    if (tr)
      for (int e = tid; e < T * adim; e += kRollThreads) R.trace_amu[trow * T * adim + e] = cand[e];
    // ---- the critic over the T candidates
    {
      float* hb = scr + wave * kScr;
      const float sadv = s_sadv[lane];
      for (int c = wave; c < T; c += kRollWaves) {
        const float qv = q_cand(net, ao1, adim, cand + c * adim, w1s, ao2s, s_w2, b2eff, sadv, hb, hb + kCat, lane);
        if (lane == 0) qs[c] = qv;
      }
    }
    __syncthreads();
    if (tr)
      for (int c = tid; c < T; c += kRollThreads) R.trace_q[trow * T + c] = qs[c];
    // ---- greedy selection (aql_select at eps 0) and the env step
    if (wave == 0) {
      const int arg = select_cand(qs, T, 0.f, R.sel_seed, b, ctr, lane);
      float s2, r;
      bool term;
      env_dynamics(V, b, lane, s_obs, s_phys, cand + arg * adim, ctr, s2, r, term);
      len += 1;
      ret += r;
      const bool done = term || len >= R.max_steps;
      __builtin_amdgcn_wave_barrier();
      if (!done && lane < obs) s_obs[lane] = s2;
      if (lane == 0) {
        if (tr) {
          R.trace_act[trow] = arg;
          R.trace_rew[trow] = r;
        }
        s_done = done ? 1 : 0;
        if (done) {
          R.returns[b] = ret;
          R.lengths[b] = len;
          R.ended[b] = term ? 1 : 2;
        }
      }
    }
    __syncthreads();
    if (s_done) break;  // workgroup-uniform
  }
}

}  // namespace

// Limits: 1 <= N <= 1024 episodes, 1 <= max_steps <= 10000, obs / actions as aql_propose
// (1..64), action dim <= 8, and the candidate set must fit the kernel's LDS layout:
// T <= 1024 and T * (adim + 1) <= 4608 floats -- the AQL constructor's default of 500
// candidates fits for every action dim <= 8.
void aql_rollout(const AqlRollout& R, hipStream_t s) {
  static const int obs_of[3] = {kBwObs, 4, 3}, adim_of[3] = {kBwAct, 1, 1}, cont_of[3] = {1, 0, 1};
  const AQLNet& n = R.net;
  if (R.N < 1 || R.N > 1024) throw std::invalid_argument("aql_rollout: 1 <= N <= 1024");
  if (R.max_steps < 1 || R.max_steps > 10000) throw std::invalid_argument("aql_rollout: 1 <= max_steps <= 10000");
  if (R.kind < 0 || R.kind > 2) throw std::invalid_argument("aql_rollout: kind 0 (bipedal) / 1 (cartpole) / 2 (pendulum)");
  if (n.obs < 1 || n.obs > 64) throw std::invalid_argument("aql_rollout: 1 <= obs <= 64");
  if (n.na < 1 || n.na > 64) throw std::invalid_argument("aql_rollout: 1 <= actions <= 64");
  if (n.adim < 1 || n.adim > kRollMaxAdim) throw std::invalid_argument("aql_rollout: 1 <= action dim <= 8");
  if (!n.cont && n.uniform > n.na) throw std::invalid_argument("aql_rollout: uniform > actions (discrete)");
  if (n.uniform < 0 || n.uniform > n.T) throw std::invalid_argument("aql_rollout: 0 <= uniform <= T");
  if (n.T < 1 || n.T > kRollMaxT || n.T * (n.adim + 1) > kRollCandFloats)
    throw std::invalid_argument("aql_rollout: the candidate set must fit LDS: T <= 1024 and T * (adim + 1) <= 4608");
  if (n.obs != obs_of[R.kind] || n.adim != adim_of[R.kind] || (n.cont != 0) != (cont_of[R.kind] != 0) ||
      (n.cont && n.na != n.adim))
    throw std::invalid_argument("aql_rollout: the net's obs / action dims do not match the env kind");
  if (!R.returns || !R.lengths || !R.ended) throw std::invalid_argument("aql_rollout: null outputs");
  const int ntr = (R.trace_obs != nullptr) + (R.trace_amu != nullptr) + (R.trace_q != nullptr) +
                  (R.trace_act != nullptr) + (R.trace_rew != nullptr);
  if (ntr != 0 && ntr != 5) throw std::invalid_argument("aql_rollout: all five trace pointers or none");
  if (ntr == 5 && R.trace_T < 1) throw std::invalid_argument("aql_rollout: trace_T >= 1");
  if (!n.qf_w1 || !n.qf_b1 || !n.qf_w2 || !n.qf_b2 || !n.ao_w1 || !n.ao_b1 || !n.a1_wmu || !n.a1_bmu || !n.a2_wmu ||
      !n.a2_bmu || !n.f_w || !n.f_b || !n.df_w1 || !n.df_b1 || !n.df_w2 || !n.df_b2 ||
      (n.cont && (!n.ao_w2 || !n.ao_b2)) ||
      (n.noisy && (!n.a1_wsig || !n.a1_weps || !n.a1_bsig || !n.a1_beps || !n.a2_wsig || !n.a2_weps || !n.a2_bsig ||
                   !n.a2_beps)))
    throw std::invalid_argument("aql_rollout: missing weights");
  if (reinterpret_cast<uintptr_t>(n.df_w1) & 15)
    throw std::invalid_argument("aql_rollout: dist_feature.0 must be 16-byte aligned (flatten with align=4)");
  if (n.cont && (!R.low || !R.high || !R.var)) throw std::invalid_argument("aql_rollout: action bounds / variance");
  if (R.kind == 0 && (!R.dynA || !R.dynB || !R.dynw)) throw std::invalid_argument("aql_rollout: dynamics matrices");
  aql_rollout_k<<<R.N, kRollThreads, 0, s>>>(R);
  LAUNCH_CHECK();
}

}  // namespace apex
