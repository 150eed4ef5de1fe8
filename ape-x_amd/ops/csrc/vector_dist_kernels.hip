// Categorical (C51) distributional heads for the wide MLP dueling DQN of the vector-observation Ape-X
// engine on gfx950: obs <= 128, A <= 8, 2 <= atoms N <= 64, hidden 128, batches to 1024, fp32.
// advantage.2 is [A N][128] (unit a N + z), value.2 [N][128]; the logits of action a are
// l[a][z] = V[z] + Adv[a][z] - mean_a' Adv[a'][z], the return distribution is softmax_z(l[a]) over the
// support z_i = v_min + i dz, dz = (v_max - v_min) / (N - 1), and Q[a] is its mean.
//
// The trunk (features.0, advantage.0 | value.0) is vector_wide_kernels.hip's: native fp32 MFMA
// (v_mfma_f32_32x32x2_f32) through the operand scheme of vector_wide_common.h, 256 threads, a workgroup
// per 32 rows, activations in LDS.  Everything is summed in an order fixed by the code, with no
// atomics: reruns are bit-identical.
//
//   vecd_forward  (device) after the trunk each action's atoms are padded to 64 columns of the LDS
//                 logits image lg [32][A 64 + 4], so an action is two 32x32 tiles that share their
//                 activation (tile_nt<2>; one tile when N <= 32) and value.2 is one more such pair:
//                 A + 1 pairs = 2A + 2 tiles dealt over the four waves.  Units >= N of a block are
//                 zero operands, never read from the weights, and stored as zeros.  value.2's rows
//                 are not 16-byte aligned in the flat parameter vector when A N % 4 != 0: ldw4's
//                 dword form.  V [32][65] and the action mean [32][65] take the place of the
//                 observation tile, which is dead once features.0 is done.  Then the mean over
//                 actions per (row, z) in index order, lanes along z; then one thread per (row, a):
//                 l = V + Adv - mean, the max, lg <- l - max, s = sum_z exp(l - max), and
//                 Q[a] = sum_z (exp(l - max) / s) fmaf(z, dz, v_min), all in atom order.
//   vecd_act / vecd_host_eval_act   vecw_act's / vecw_host_eval_act's row sources, output buffers
//                 and draw (first argmax, the same Philox key) applied to the expected Q.
//   vecd_learn    one workgroup per 32 sampled rows: online(s') -> a* = first argmax of its expected
//                 Q; target(s') keeps only p_tgt(s', a*), 64 floats a row (s' is loaded again: the
//                 first pass has reused its tile); online(s) last so f / h / lg stay for the backward.
//                 Projection in its gather form: b_j = (clamp(r + gamma_n (1 - done) z_j) - v_min) / dz,
//                 m_i = sum_j p_j max(0, 1 - |b_j - i|) -- deterministic, no LDS atomics, and a target
//                 atom that lands on a support atom (l == u) is right by construction.
//                 lw = w * ce, ce = -sum_i m_i log_softmax(l(s, a))_i.
//                 delta = |sum_i m_i z_i - Q(s, a)|, the EXPECTED-VALUE TD error and not the
//                 cross-entropy: the actor side (nstep_emit) writes its initial priorities from
//                 expected-Q TD errors, and the learner's priorities live on the same scale in the one
//                 tree.  Backward in the same launch: g = w / B (p - m) for the taken action, dV = g,
//                 dAdv[a'][z] = g[z] ((a' == a) - 1/A) written dense over lg;
//                 dH = (dAdv . Wa2 | dV . Wv2) * relu' on tile_nn (K = 64 per action, and 64), the
//                 result held in registers across a barrier and then written over lg, which every
//                 wave has finished reading; dF as vecw_learn.  Per-sample rows in the vecd layout:
//                 X / F / DF / H / DH, G = g at 64 slots, the action index -- no dense dAdv in memory.
//   vecd_grad     vecw_grad's contraction and tile map for features.0, advantage.0 and value.0;
//                 advantage.2 is A ceil(N / 32) row tiles by 4 column tiles whose left operand
//                 G_b[z] ((act_b == a') - 1/A) is formed in registers (its column sums: the bias
//                 gradient); value.2 is ceil(N / 32) by 4 tiles with G as it is.  One fp64
//                 sum-of-squares partial per workgroup.
//
// LDS: vecd_act 144000 B, vecd_learn 155136 B of gfx950's 163840 (one workgroup per CU), vecd_grad
// 16928 B; no scratch (profiles/vector_dist.md has the registers).
#include "vector_wide_common.h"

namespace apex {

namespace {

using namespace widemfma;

constexpr int kZ = kVecDistMaxAtoms;         // 64 slots per action
constexpr int kDA = kVecDistMaxA;            // 8
constexpr int kPL = kDA * kZ + 4;            // 516 floats = 129 16-byte slots
constexpr int kPZ = kZ + 4;                  // 68 = 17 slots
constexpr int kPV = kZ + 1;                  // 65 (scalar reads)
constexpr int kPQD = kDA + 1;                // 9
static_assert(2 * kRows * kPV <= kRows * kPX, "V and the action mean alias the observation tile");
static_assert(kRows * kPH <= kRows * kPL, "dh is written over the logits image");

struct alignas(16) DistLds {
  float x[kRows * kPX];    // the observation tile; after features.0: V [32][kPV] | action mean [32][kPV]
  float f[kRows * kPF];    // relu(features.0)
  float h[kRows * kPH];    // relu(advantage.0) | relu(value.0)
  float lg[kRows * kPL];   // per action 64 slots: advantage.2 -> l - max; the learner: dAdv, then dh
  float mg[kRows * kPZ];   // the learner: m, then g (zero in [N, 64))
  float s[kRows * kDA];    // sum_z exp(l - max) per (row, action)
  float q[kRows * kPQD];   // expected Q
};

__device__ __forceinline__ float dist_dz(const VecNet& n) { return (n.v_max - n.v_min) / (float)(n.atoms - 1); }

// x rows of the workgroup: row r is ring row id(r); columns [obs, kp) are zero.  out: the live rows
// also go to the X slots of the per-sample rows at out (null: nowhere).
template <class Id>
__device__ __forceinline__ void load_x(DistLds& L, const float* __restrict__ ring, int obs, Id id, float* out,
                                       int live) {
  const int kp = (obs + 7) & ~7;
  for (int i = threadIdx.x; i < kRows * kp; i += kT) {
    const int r = i / kp, k = i - r * kp;
    const float v = k < obs ? ring[(size_t)id(r) * obs + k] : 0.f;
    L.x[r * kPX + k] = v;
    if (out && r < live) out[(size_t)r * vecd::STRIDE + vecd::X + k] = v;
  }
}

// Expected Q of the 32 rows in L.x -> L.f, L.h, L.lg (l - max), L.s, L.q.  L.x is consumed.  Begins
// and ends with a workgroup barrier.
__device__ __forceinline__ void vecd_forward(const VecNet& n, DistLds& L) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const int col = wave * 32 + r;
  const int A = n.A, N = n.atoms;
  __syncthreads();
  {  // features.0: wave w owns units 32w .. 32w + 31
    f32x16 acc[1] = {};
    const float* const wrow[1] = {n.w0 + (size_t)col * n.obs};
    const bool vec[1] = {rows_aligned16(n.w0, n.obs)};
    tile_nt<1>(acc, L.x, kPX, (n.obs + 7) & ~7, wrow, n.obs, vec, lane);
    const float b = n.b0[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) L.f[acc_row(i, hf) * kPF + col] = fmaxf(acc[0][i] + b, 0.f);
  }
  __syncthreads();
  {  // advantage.0 | value.0 as one N = 256 GEMM: wave w owns block w of each head
    f32x16 acc[2] = {};
    const float* const wrow[2] = {n.wa1 + (size_t)col * kH, n.wv1 + (size_t)col * kH};
    const bool vec[2] = {rows_aligned16(n.wa1, kH), rows_aligned16(n.wv1, kH)};
    tile_nt<2>(acc, L.f, kPF, kH, wrow, kH, vec, lane);
    const float ba = n.ba1[col], bv = n.bv1[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float* hr = L.h + acc_row(i, hf) * kPH;
      hr[col] = fmaxf(acc[0][i] + ba, 0.f);
      hr[kH + col] = fmaxf(acc[1][i] + bv, 0.f);
    }
  }
  __syncthreads();
  float* vb = L.x;                    // V [32][kPV] (the observation tile is dead)
  float* mean = L.x + kRows * kPV;    // mean_a Adv [32][kPV]
  // advantage.2 (pair p < A: action p) and value.2 (pair A): two 32-unit tiles over one activation
  for (int p = wave; p <= A; p += 4) {
    const bool isv = p == A;
    const float* w = isv ? n.wv2 : n.wa2 + (size_t)p * N * kH;
    const float* bias = isv ? n.bv2 : n.ba2 + p * N;
    const float* act = L.h + (isv ? kH : 0);
    const bool al = rows_aligned16(w, kH);
    const bool live[2] = {r < N, 32 + r < N};
    f32x16 acc[2] = {};
    if (N > 32) {
      const float* const wrow[2] = {live[0] ? w + (size_t)r * kH : nullptr,
                                    live[1] ? w + (size_t)(32 + r) * kH : nullptr};
      const bool vec[2] = {al, al};
      tile_nt<2>(acc, act, kPH, kH, wrow, kH, vec, lane);
    } else {  // the second tile is all zero operands
      f32x16 one[1] = {};
      const float* const wrow[1] = {live[0] ? w + (size_t)r * kH : nullptr};
      const bool vec[1] = {al};
      tile_nt<1>(one, act, kPH, kH, wrow, kH, vec, lane);
      acc[0] = one[0];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int z = 32 * u + r;
      const float b = live[u] ? bias[z] : 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, hf);
        const float v = live[u] ? acc[u][i] + b : 0.f;
        if (isv) vb[row * kPV + z] = v;
        else L.lg[row * kPL + p * kZ + z] = v;
      }
    }
  }
  __syncthreads();
  // the action mean per (row, z), Adv summed in index order; lanes along z
  for (int row = wave; row < kRows; row += 4) {
    if (lane < N) {
      const float* ar = L.lg + row * kPL + lane;
      float sum = 0.f;
      for (int a = 0; a < A; ++a) sum += ar[a * kZ];
      mean[row * kPV + lane] = sum / (float)A;
    }
  }
  __syncthreads();
  if (t < kRows * A) {  // the dueling combine, the softmax over z and the expected Q of (row, a)
    const int row = t & 31, a = t >> 5;
    float* lr = L.lg + row * kPL + a * kZ;
    const float* vr = vb + row * kPV;
    const float* mr = mean + row * kPV;
    const float dz = dist_dz(n);
    float mx = -INFINITY;
    for (int z = 0; z < N; ++z) {
      const float l = vr[z] + lr[z] - mr[z];
      lr[z] = l;
      mx = fmaxf(mx, l);
    }
    float s = 0.f;
    for (int z = 0; z < N; ++z) {
      const float sh = lr[z] - mx;
      lr[z] = sh;
      s += expf(sh);
    }
    float qv = 0.f;
    for (int z = 0; z < N; ++z) qv += expf(lr[z]) / s * fmaf((float)z, dz, n.v_min);
    L.s[row * kDA + a] = s;
    L.q[row * kPQD + a] = qv;
  }
  __syncthreads();
}

// vec_act_k's draw on the expected Q of row t: first argmax; explore iff !(u0 > eps); min(int(u1 A), A - 1)
__device__ __forceinline__ int dist_draw(const float* row, int A, float* qout, uint64_t seed, uint64_t e,
                                         uint64_t counter, float eps) {
  int best = 0;
  float bv = row[0];
  for (int k = 1; k < A; ++k)
    if (row[k] > bv) { bv = row[k]; best = k; }
  for (int k = 0; k < A; ++k) qout[k] = row[k];
  float u[4];
  uniform4(seed, e, counter, u);
  if (!(u[0] > eps)) {
    const int rr = (int)(u[1] * (float)A);
    best = rr < A ? rr : A - 1;
  }
  return best;
}

// ------------------------------------------------------------------ acting
__global__ __launch_bounds__(kT) void vecd_act_k(VecAct a) {
  __shared__ DistLds L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows;
  // rows past E repeat the last env (never written)
  load_x(L, a.ring, a.net.obs, [&](int r) { return a.hist[min(e0 + r, a.E - 1) * 4 + 3]; }, nullptr, 0);
  vecd_forward(a.net, L);
  const int e = e0 + t;
  if (t < kRows && e < a.E)
    a.actions[e] = dist_draw(L.q + t * kPQD, a.net.A, a.q + (size_t)e * a.net.A, a.seed, (uint64_t)e,
                             a.counter ? (uint64_t)a.counter[0] : 0ull, a.eps[e]);
}

// vecd_act_k for the host-env evaluator (vecw_host_eval_act_k's row source): the observations straight
// from the staging block's reset_obs rows, the step k by value, epsilon 0
__global__ __launch_bounds__(kT) void vecd_host_eval_act_k(VecHostEvalAct a) {
  __shared__ DistLds L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows;
  const int obs = a.net.obs, kp = (obs + 7) & ~7;
  const int live = min(kRows, a.N - e0);   // >= 1: the grid is ceil(N / 32)
  const float* src = a.stage + (size_t)(a.N + e0) * obs;
  for (int i = t; i < kRows * kp; i += kT) {
    const int r = i / kp, k = i - r * kp;
    L.x[r * kPX + k] = k < obs ? src[min(r, live - 1) * obs + k] : 0.f;
  }
  vecd_forward(a.net, L);
  const int e = e0 + t;
  if (t < live)
    a.actions[e] = dist_draw(L.q + t * kPQD, a.net.A, a.q + (size_t)e * a.net.A, a.seed, (uint64_t)e, (uint64_t)a.k,
                             0.f);
}

// ------------------------------------------------------------------ learner
__global__ __launch_bounds__(kT) void vecd_learn_k(VecLearn p) {
  __shared__ DistLds L;
  __shared__ float pt[kRows * kZ];          // p_tgt(s', a*), zero in [N, 64)
  __shared__ float qt[kRows * kPQD];        // target net on s'
  __shared__ float q2[kRows * kPQD];        // online net on s'
  __shared__ float wsc[kRows];              // w_b / B (0 on a padding row)
  __shared__ int sid[kRows], sid2[kRows], ast[kRows], actb[kRows];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const int col = wave * 32 + r;
  const int b0 = blockIdx.x * kRows;
  const int obs = p.on.obs, A = p.on.A, N = p.on.atoms;
  const float v_min = p.on.v_min, v_max = p.on.v_max, dz = dist_dz(p.on);
  const int live = min(kRows, p.B - b0);
  if (blockIdx.x == 0 && t == 0 && p.beta_out) {
    // PER beta of the NEXT step (this step's draw has run): beta_by_frame(step + 1)
    const double st = (double)(p.step ? p.step[0] : 0) + 1.0;
    p.beta_out[0] = (float)fmin(1.0, p.beta0 + st * (1.0 - p.beta0) / p.beta_horizon);
  }
  if (t < kRows) {  // rows past B repeat the last sample (never written)
    const int row = p.idx[min(b0 + t, p.B - 1)];
    sid[t] = p.s_ids[row * 4 + 3];
    sid2[t] = p.s2_ids[row * 4 + 3];
  }
  __syncthreads();
  load_x(L, p.ring, obs, [&](int rr) { return sid2[rr]; }, nullptr, 0);
  vecd_forward(p.on, L);
  for (int i = t; i < kRows * kPQD; i += kT) q2[i] = L.q[i];
  if (t < kRows) {  // a* = first argmax of the online expected Q(s')
    const float* qn = L.q + t * kPQD;
    int astar = 0;
    float best = qn[0];
    for (int k = 1; k < A; ++k)
      if (qn[k] > best) { best = qn[k]; astar = k; }
    ast[t] = astar;
  }
  load_x(L, p.ring, obs, [&](int rr) { return sid2[rr]; }, nullptr, 0);  // (the forward has reused the tile)
  vecd_forward(p.tg, L);
  for (int i = t; i < kRows * kPQD; i += kT) qt[i] = L.q[i];
  for (int i = t; i < kRows * kZ; i += kT) {  // p_tgt(s', a*): all of the target pass that is kept
    const int row = i >> 6, z = i & (kZ - 1), a = ast[row];
    pt[i] = z < N ? expf(L.lg[row * kPL + a * kZ + z]) / L.s[row * kDA + a] : 0.f;
  }
  load_x(L, p.ring, obs, [&](int rr) { return sid[rr]; }, p.vec + (size_t)b0 * vecd::STRIDE, live);
  vecd_forward(p.on, L);  // online(s) last: its f / h / lg stay for the backward
  const int prow = t >> 3, pc = (t & 7) * 8;  // (row, eight atoms) of this thread in the per-atom passes
  {  // the projected target m of row prow, atoms pc .. pc + 7: a gather over j in atom order
    const int sr = p.idx[min(b0 + prow, p.B - 1)];
    const float rew = p.rew[sr], cont = p.gamma_n * (1.f - p.done[sr]);
    float m[8] = {};
    for (int j = 0; j < N; ++j) {
      const float tz = fminf(fmaxf(rew + cont * fmaf((float)j, dz, v_min), v_min), v_max);
      const float bj = (tz - v_min) / dz, pj = pt[prow * kZ + j];
#pragma unroll
      for (int k = 0; k < 8; ++k) m[k] += pj * fmaxf(0.f, 1.f - fabsf(bj - (float)(pc + k)));
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) L.mg[prow * kPZ + pc + k] = pc + k < N ? m[k] : 0.f;
  }
  __syncthreads();
  if (t < kRows) {  // the loss terms of row t
    const int b = b0 + t;
    int a = 0;
    float sc = 0.f;
    if (b < p.B) {
      const int row = p.idx[b];
      a = min(max(p.act[row], 0), A - 1);
      const float* lr = L.lg + t * kPL + a * kZ;
      const float logs = logf(L.s[t * kDA + a]);
      float ce = 0.f, ez = 0.f;
      for (int i = 0; i < N; ++i) {
        const float mi = L.mg[t * kPZ + i];
        ce -= mi * (lr[i] - logs);
        ez += mi * fmaf((float)i, dz, v_min);
      }
      p.delta[b] = fabsf(ez - L.q[t * kPQD + a]);
      p.lw[b] = p.w[b] * ce;
      sc = p.w[b] / (float)p.B;
      for (int k = 0; k < A; ++k) {
        p.q_s[(size_t)b * A + k] = L.q[t * kPQD + k];
        p.q_s2[(size_t)b * A + k] = q2[t * kPQD + k];
        p.qt_s2[(size_t)b * A + k] = qt[t * kPQD + k];
      }
    }
    actb[t] = a;
    wsc[t] = sc;
  }
  __syncthreads();
  {  // g = w / B (p - m) of the taken action -> mg; dAdv[a'][z] = g ((a' == a) - 1/A) dense over lg
    const int a = actb[prow];
    const float sc = wsc[prow], s = L.s[prow * kDA + a], ia = 1.f / (float)A;
    float* lr = L.lg + prow * kPL + pc;
    float g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      g[k] = pc + k < N ? sc * (expf(lr[a * kZ + k]) / s - L.mg[prow * kPZ + pc + k]) : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) L.mg[prow * kPZ + pc + k] = g[k];
    for (int o = 0; o < A; ++o) {
      const float c = (o == a ? 1.f : 0.f) - ia;
#pragma unroll
      for (int k = 0; k < 8; ++k) lr[o * kZ + k] = g[k] * c;
    }
  }
  __syncthreads();
  float* dh = L.lg;  // [32][kPH], once dAdv has been read by every wave
  {  // dH = (dAdv . Wa2 | dV . Wv2) * relu': K = 64 per action, and 64
    const int kpz = (N + 7) & ~7;
    f32x16 acca = {}, accv = {};
    for (int o = 0; o < A; ++o)
      tile_nn(acca, L.lg + o * kZ, kPL, kpz, p.on.wa2 + (size_t)o * N * kH + col, N, lane);
    tile_nn(accv, L.mg, kPZ, kpz, p.on.wv2 + col, N, lane);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(i, hf);
      const float* hr = L.h + row * kPH;
      dh[row * kPH + col] = hr[col] > 0.f ? acca[i] : 0.f;
      dh[row * kPH + kH + col] = hr[kH + col] > 0.f ? accv[i] : 0.f;
    }
  }
  __syncthreads();
  {  // dF = (dHa . Wa1 + dHv . Wv1) * relu', from the accumulators to the per-sample rows
    f32x16 acc = {};
    tile_nn(acc, dh, kPH, kH, p.on.wa1 + col, kH, lane);
    tile_nn(acc, dh + kH, kPH, kH, p.on.wv1 + col, kH, lane);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(i, hf);
      if (row < live)
        p.vec[(size_t)(b0 + row) * vecd::STRIDE + vecd::DF + col] = L.f[row * kPF + col] > 0.f ? acc[i] : 0.f;
    }
  }
  // the rest of the per-sample rows out of LDS, a row's floats on consecutive lanes
  for (int i = t; i < live * kH; i += kT) {
    const int row = i >> 7, k = i & (kH - 1);
    p.vec[(size_t)(b0 + row) * vecd::STRIDE + vecd::F + k] = L.f[row * kPF + k];
  }
  for (int i = t; i < live * 2 * kH; i += kT) {
    const int row = i >> 8, k = i & (2 * kH - 1);
    float* v = p.vec + (size_t)(b0 + row) * vecd::STRIDE;
    v[vecd::H + k] = L.h[row * kPH + k];
    v[vecd::DH + k] = dh[row * kPH + k];
  }
  for (int i = t; i < live * kZ; i += kT) {
    const int row = i >> 6, k = i & (kZ - 1);
    p.vec[(size_t)(b0 + row) * vecd::STRIDE + vecd::G + k] = L.mg[row * kPZ + k];
  }
  if (t < live) p.vec[(size_t)(b0 + t) * vecd::STRIDE + vecd::ACT] = (float)actb[t];
}

// ------------------------------------------------------------------ batch contraction
// The tile of workgroup blk.  kind 1: advantage.2 of action `a` (the tile's tensor is that action's N
// rows), left operand G_b ((act_b == a) - 1/A); kind 2: value.2, left operand G_b; kind 0: vecw's tiles.
struct DistTile {
  GradTile T;
  int kind, a;
};

__device__ __forceinline__ DistTile dist_grad_tile(int blk, int obs, int A, int N) {
  const int nt0 = (obs + 31) / 32, nz = (N + 31) / 32;
  const int64_t o1 = (int64_t)kH * obs, o2 = o1 + kH, o3 = o2 + kH * kH, o4 = o3 + kH,
                o5 = o4 + (int64_t)A * N * kH, o6 = o5 + A * N, o7 = o6 + kH * kH, o8 = o7 + kH,
                o9 = o8 + (int64_t)N * kH;
  DistTile d;
  d.kind = 0;
  d.a = 0;
  int ntn = 4;  // column blocks of the tensor
  if (blk < 4 * nt0)                     { d.T = {0, o1, kH, obs, vecd::DF, vecd::X, 0, 0}; ntn = nt0; }
  else if ((blk -= 4 * nt0) < 16)        { d.T = {o2, o3, kH, kH, vecd::DH, vecd::F, 0, 0}; }
  else if ((blk -= 16) < 4 * A * nz) {
    d.kind = 1;
    d.a = blk / (4 * nz);
    blk -= d.a * 4 * nz;
    d.T = {o4 + (int64_t)d.a * N * kH, o5 + d.a * N, N, kH, vecd::G, vecd::H, 0, 0};
  }
  else if ((blk -= 4 * A * nz) < 16)     { d.T = {o6, o7, kH, kH, vecd::DH + kH, vecd::F, 0, 0}; }
  else                                   { blk -= 16; d.kind = 2; d.T = {o8, o9, N, kH, vecd::G, vecd::H + kH, 0, 0}; }
  d.T.m0 = (blk / ntn) * 32;
  d.T.n0 = (blk % ntn) * 32;
  return d;
}

__global__ __launch_bounds__(kT) void vecd_grad_k(VecDistGrad d) {
  __shared__ GradRed R;
  const VecGrad& g = d.g;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const DistTile D = dist_grad_tile(blockIdx.x, g.obs, g.A, d.atoms);
  const GradTile& T = D.T;
  const int chunk = grad_chunk(g.B);
  const int bs = wave * chunk, be = min(g.B, bs + chunk);
  const bool mok = T.m0 + r < T.rows, nok = T.n0 + r < T.cols;
  const float* pg = g.vec + T.goff + T.m0 + r;
  const float* px = g.vec + T.xoff + T.n0 + r;
  const float* pa = g.vec + vecd::ACT;
  const float ia = 1.f / (float)g.A;
  f32x16 acc = {};
  float bsum = 0.f;
  for (int b = bs; b < be; b += 8) {  // four k steps: their loads are issued before the MFMAs
    float av[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int bb = b + 2 * u + hf;
      const bool in = bb < be;  // the tail is zero operands: nothing is read past the range
      av[u] = in && mok ? pg[(size_t)bb * vecd::STRIDE] : 0.f;
      xv[u] = in && nok ? px[(size_t)bb * vecd::STRIDE] : 0.f;
      if (D.kind == 1 && in)  // dAdv of this tile's action from G, in registers
        av[u] *= ((int)pa[(size_t)bb * vecd::STRIDE] == D.a ? 1.f : 0.f) - ia;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc = mfma32(av[u], xv[u], acc);
      bsum += av[u];
    }
  }
  grad_finish(R, acc, bsum, T, g.grad, g.part);
}

void check_dist_shape(int obs, int A, int atoms, const char* who) {
  if (obs < 1 || obs > kVecWideMaxObs || A < 1 || A > kVecDistMaxA || atoms < 2 || atoms > kVecDistMaxAtoms)
    throw std::invalid_argument(std::string(who) + ": obs in [1, 128], actions in [1, 8] and atoms in [2, 64]");
}

void check_dist_net(const VecNet& n, const char* who) {
  check_dist_shape(n.obs, n.A, n.atoms, who);
  if (!(n.v_min < n.v_max)) throw std::invalid_argument(std::string(who) + ": v_min < v_max");
  if (!n.w0 || !n.b0 || !n.wa1 || !n.ba1 || !n.wa2 || !n.ba2 || !n.wv1 || !n.bv1 || !n.wv2 || !n.bv2)
    throw std::invalid_argument(std::string(who) + ": missing parameter tensor");
}

}  // namespace

// ------------------------------------------------------------------ launchers
void vecd_act(const VecAct& a, hipStream_t s) {
  if (a.ring_bf16) throw std::invalid_argument("vecd_act: a bf16 ring is read by the tall bf16 kernels (vectb_*) only");
  check_dist_net(a.net, "vecd_act");
  if (a.E < 1 || a.E > 4096 || !a.ring || !a.hist || !a.eps || !a.q || !a.actions)
    throw std::invalid_argument("vecd_act: 1 <= E <= 4096 with ring, hist, eps, q and actions");
  vecd_act_k<<<(a.E + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vecd_host_eval_act(const VecHostEvalAct& a, hipStream_t s) {
  check_dist_net(a.net, "vecd_host_eval_act");
  if (a.N < 1 || a.N > 64) throw std::invalid_argument("vecd_host_eval_act: 1 <= N <= 64 evaluator envs");
  if (a.k < 0) throw std::invalid_argument("vecd_host_eval_act: step k >= 0");
  if (!a.stage) throw std::invalid_argument("vecd_host_eval_act: the staging block's device copy");
  if (!a.q || !a.actions) throw std::invalid_argument("vecd_host_eval_act: q and actions");
  vecd_host_eval_act_k<<<(a.N + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vecd_learn(const VecLearn& p, hipStream_t s) {
  if (p.ring_bf16) throw std::invalid_argument("vecd_learn: a bf16 ring is read by the tall bf16 kernels (vectb_*) only");
  check_dist_net(p.on, "vecd_learn (online)");
  check_dist_net(p.tg, "vecd_learn (target)");
  if (p.on.obs != p.tg.obs || p.on.A != p.tg.A || p.on.atoms != p.tg.atoms || p.on.v_min != p.tg.v_min ||
      p.on.v_max != p.tg.v_max)
    throw std::invalid_argument("vecd_learn: nets differ in shape or support");
  if (p.B < 1 || p.B > 1024) throw std::invalid_argument("vecd_learn: batch must be in [1, 1024]");
  if (!p.ring || !p.s_ids || !p.s2_ids || !p.act || !p.rew || !p.done || !p.idx || !p.w || !p.q_s || !p.q_s2 ||
      !p.qt_s2 || !p.vec || !p.delta || !p.lw)
    throw std::invalid_argument("vecd_learn: missing buffer");
  if (p.beta_out && !(p.beta_horizon > 0.0)) throw std::invalid_argument("vecd_learn: beta horizon must be > 0");
  vecd_learn_k<<<(p.B + kRows - 1) / kRows, kT, 0, s>>>(p);
  LAUNCH_CHECK();
}

int64_t vecd_param_count(int obs, int A, int atoms) {
  check_dist_shape(obs, A, atoms, "vecd_param_count");
  return (int64_t)kH * obs + kH + 2 * ((int64_t)kH * kH + kH) + ((int64_t)A * atoms + atoms) * (kH + 1);
}

int vecd_grad_blocks(int obs, int A, int atoms) {
  check_dist_shape(obs, A, atoms, "vecd_grad_blocks");
  return 4 * ((obs + 31) / 32) + 16 + 4 * A * ((atoms + 31) / 32) + 16 + 4 * ((atoms + 31) / 32);
}

void vecd_grad(const VecDistGrad& d, hipStream_t s) {
  const VecGrad& g = d.g;
  check_dist_shape(g.obs, g.A, d.atoms, "vecd_grad");
  if (g.n != vecd_param_count(g.obs, g.A, d.atoms))
    throw std::invalid_argument("vecd_grad: n must be the categorical MLP dueling net's parameter count");
  if (g.B < 1 || g.B > 1024 || !g.vec || !g.grad || !g.part)
    throw std::invalid_argument("vecd_grad: batch in [1, 1024] with vec, grad and part");
  vecd_grad_k<<<vecd_grad_blocks(g.obs, g.A, d.atoms), kT, 0, s>>>(d);
  LAUNCH_CHECK();
}

}  // namespace apex
