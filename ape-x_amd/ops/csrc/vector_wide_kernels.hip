// Wide MLP dueling DQN for the vector-observation Ape-X engine on gfx950: obs <= 128, A <= 32,
// hidden 128, batches to 1024 (reference model.py DuelingDQN for any flat observation and any
// discrete action set).  vector_kernels.hip keeps one observation row per thread in registers and
// runs every layer as fp32 FMA loops; at obs = 128 and B >= 256 the step is five small GEMMs per
// pass and five batch contractions, and they run here on the matrix cores.
//
// Precision: native fp32 MFMA (v_mfma_f32_32x32x2_f32): exact fp32 products, fp32 accumulation in
// an order fixed by the code -- no reduced-precision operand, no atomics, bit-identical reruns.
//
//   vecw_forward  (device) a workgroup of 4 waves owns 32 rows.  Activations live in LDS
//                 (x [32][132], f [32][132], h [32][260]: row pitches of an odd number of 16-byte
//                 slots, so the 32 rows of a ds_read_b128 fall into distinct slots).  For
//                 out[32][N] = act[32][K] . W^T each wave owns 32-unit column blocks of N.  Operands
//                 arrive through a k-permutation: in step group j the half-wave hf = lane / 32
//                 takes k = 8j + 4hf .. 8j + 4hf + 3, so a lane reads W[n][k..k+3] straight from
//                 global (row-major [units][K], L2-resident) and act[m][k..k+3] from LDS as one
//                 16-byte load each, and the pair feeds four MFMAs (MFMA i of the group reduces
//                 k = 8j + i and 8j + 4 + i).  K is padded with zeros in LDS only; weights are
//                 never read past obs.  A weight tensor whose rows are not 16-byte aligned
//                 (features.0 at obs % 4 != 0; value.0 in the flat parameter vector at A % 4 != 0)
//                 takes four dword loads instead.  Bias and ReLU go from the accumulators into the
//                 next layer's LDS image.  advantage.2 is one 32x32 tile on wave 0 (units >= A are
//                 zero operands, never stored), value.2 a second tile on wave 1 (unit 0 only: it
//                 runs beside wave 0's, so it costs no time over a VALU dot), then the dueling
//                 combine with vec_forward's order (sum of A in index order, V + A_k - mean).
//   vecw_act      one workgroup per 32 envs: ring row hist[e][3] -> forward -> q[E][A] and
//                 vec_act_k's epsilon-greedy draw, arithmetic for arithmetic.
//   vecw_host_eval_act  vecw_act for the host-env evaluator (N <= 64 envs, one or two workgroups):
//                 the observations straight from the staging block's reset_obs rows into the x
//                 image, the step k by value as the Philox counter, epsilon 0.  One launch per
//                 evaluator step; Q and the actions are vecw_act's bit for bit.
//   vecw_learn   one workgroup per 32 sampled rows: target(s'), online(s'), online(s) last so its
//                 x / f / h stay in LDS; dqn_loss_k's per-row loss; the backward on MFMA in the
//                 same launch: dH = (dA . Wa2 | dV wv2) * relu', dF = (dHa . Wa1 + dHv . Wv1) * relu'.
//                 These use the weights untransposed: the B operand is W[u][n] with the lanes along
//                 n (coalesced dword loads, 128 bytes per u per half-wave), the A operand keeps the
//                 16-byte LDS read of the k-permutation.  Writes the per-sample rows (vecw layout).
//   vecw_grad     the ten gradient tensors as batch contractions with K = B: one workgroup per
//                 32x32 output tile, its 4 waves take four contiguous batch ranges and reduce
//                 through LDS in wave order.  Both operands come straight from global with the
//                 lanes along the contiguous dimension.  A tile of the first column block also
//                 sums its left operand's columns: the bias gradient.  One fp64 sum-of-squares
//                 partial per workgroup (rmsprop_step's (parts, nparts)).
#include "common.h"
#include "kernels.h"

namespace apex {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kH = kVecHidden;            // 128
constexpr int kT = 256;                   // threads of every workgroup here
constexpr int kRows = 32;                 // rows of a workgroup's tile
constexpr int kPX = kVecWideMaxObs + 4;   // 132 floats = 33 16-byte slots
constexpr int kPF = kH + 4;               // 132
constexpr int kPH = 2 * kH + 4;           // 260 = 65 slots
constexpr int kPQ = kVecWideMaxA + 1;     // 33 (scalar reads down a column)
constexpr int kPA = kVecWideMaxA + 4;     // 36 = 9 slots
constexpr int kRound = 8;                 // step groups (of 8 k) whose operand loads are in flight together

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// accumulator register i of half-wave hf -> tile row (the 32x32 C/D map; column = lane & 31)
__device__ __forceinline__ int acc_row(int i, int hf) { return (i & 3) + 8 * (i >> 2) + 4 * hf; }

__device__ __forceinline__ bool rows_aligned16(const float* w, int ld) {
  return ((reinterpret_cast<uintptr_t>(w) & 15) == 0) && (ld & 3) == 0;
}

// w[k .. k + 3] of a weight row of kw floats (null: a zero row); elements >= kw are zero and are
// not read.  vec: the row is 16-byte aligned and kw a multiple of 4.
__device__ __forceinline__ f32x4 ldw4(const float* w, int k, int kw, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!w) return v;
  if (vec) {
    if (k < kw) v = *reinterpret_cast<const f32x4*>(w + k);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k + i < kw) v[i] = w[k + i];
  }
  return v;
}

// acc[t] += act[32][kp] . W_t^T for NT weight blocks that share the activation: wrow[t] is THIS
// lane's weight row (unit n0_t + lane % 32) of kw floats.  act: LDS, zero in [kw, kp).
template <int NT>
__device__ __forceinline__ void tile_nt(f32x16 (&acc)[NT], const float* act, int pitch, int kp,
                                        const float* const (&wrow)[NT], int kw, const bool (&vec)[NT], int lane) {
  const int r = lane & 31, hf = lane >> 5;
  const float* arow = act + r * pitch + 4 * hf;
  for (int k0 = 0; k0 < kp; k0 += 8 * kRound) {  // a round's loads are all issued before its MFMAs
    f32x4 a[kRound], b[NT][kRound];
#pragma unroll
    for (int j = 0; j < kRound; ++j) {
      const int k = k0 + 8 * j;  // a group past kp is zero operands (wave-uniform): nothing is read
      a[j] = k < kp ? *reinterpret_cast<const f32x4*>(arow + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NT; ++t) b[t][j] = ldw4(k < kp ? wrow[t] : nullptr, k + 4 * hf, kw, vec[t]);
    }
#pragma unroll
    for (int j = 0; j < kRound; ++j) {
      if (k0 + 8 * j < kp) {  // (wave-uniform: a short K issues no MFMA on zero groups)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[t] = mfma32(a[j][i], b[t][j][i], acc[t]);
      }
    }
  }
}

// acc += act[32][kp] . W[0 .. kv)[n]: the weight untransposed, wcol = W + this lane's column
// (row pitch kH); rows >= kv are zero operands and are not read.  act: LDS, zero in [kv, kp).
__device__ __forceinline__ void tile_nn(f32x16& acc, const float* act, int pitch, int kp, const float* wcol, int kv,
                                        int lane) {
  const int r = lane & 31, hf = lane >> 5;
  const float* arow = act + r * pitch + 4 * hf;
  for (int k0 = 0; k0 < kp; k0 += 8 * kRound) {
    f32x4 a[kRound];
    float b[kRound][4];
#pragma unroll
    for (int j = 0; j < kRound; ++j) {
      const int k = k0 + 8 * j;  // a group past kp is zero operands (wave-uniform): nothing is read
      a[j] = k < kp ? *reinterpret_cast<const f32x4*>(arow + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u = k + 4 * hf + i;
        b[j][i] = u < kv ? wcol[(size_t)u * kH] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < kRound; ++j) {
      if (k0 + 8 * j < kp) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = mfma32(a[j][i], b[j][i], acc);
      }
    }
  }
}

// ------------------------------------------------------------------ forward
struct alignas(16) WideLds {
  float x[kRows * kPX];
  float f[kRows * kPF];    // relu(features.0)
  float h[kRows * kPH];    // relu(advantage.0) | relu(value.0)
  float adv[kRows * kPQ];
  float val[kRows];
  float q[kRows * kPQ];
};

// x rows of the workgroup: row r is ring row id(r); columns [obs, kp) are zero
template <class Id>
__device__ __forceinline__ void load_x(WideLds& L, const float* __restrict__ ring, int obs, Id id) {
  const int kp = (obs + 7) & ~7;
  for (int i = threadIdx.x; i < kRows * kp; i += kT) {
    const int r = i / kp, k = i - r * kp;
    L.x[r * kPX + k] = k < obs ? ring[(size_t)id(r) * obs + k] : 0.f;
  }
}

// Q of the 32 rows in L.x -> L.f, L.h, L.q.  Begins and ends with a workgroup barrier.  Inlined: an
// out-of-line copy takes the net's pointers by address, through private memory.
__device__ __forceinline__ void vecw_forward(const VecNet& n, WideLds& L) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const int col = wave * 32 + r;
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
  if (wave < 2) {  // advantage.2 (wave 0: units < A) and value.2 (wave 1: unit 0), one tile each
    f32x16 acc[1] = {};
    const bool live = wave == 0 ? r < n.A : r == 0;
    const float* w = wave == 0 ? n.wa2 : n.wv2;
    const float* const wrow[1] = {live ? w + (size_t)r * kH : nullptr};
    const bool vec[1] = {rows_aligned16(w, kH)};
    tile_nt<1>(acc, L.h + wave * kH, kPH, kH, wrow, kH, vec, lane);
    if (live) {
      const float b = wave == 0 ? n.ba2[r] : n.bv2[0];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, hf);
        if (wave == 0) L.adv[row * kPQ + r] = acc[0][i] + b;
        else L.val[row] = acc[0][i] + b;
      }
    }
  }
  __syncthreads();
  if (t < kRows) {  // dueling combine of row t
    const float* ar = L.adv + t * kPQ;
    float advsum = 0.f;
    for (int o = 0; o < n.A; ++o) advsum += ar[o];
    const float mean = advsum / (float)n.A, val = L.val[t];
    for (int o = 0; o < n.A; ++o) L.q[t * kPQ + o] = val + ar[o] - mean;
  }
  __syncthreads();
}

// ------------------------------------------------------------------ acting
__global__ __launch_bounds__(kT) void vecw_act_k(VecAct a) {
  __shared__ WideLds L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows;
  // rows past E repeat the last env (never written)
  load_x(L, a.ring, a.net.obs, [&](int r) { return a.hist[min(e0 + r, a.E - 1) * 4 + 3]; });
  vecw_forward(a.net, L);
  const int e = e0 + t;
  if (t < kRows && e < a.E) {
    const int A = a.net.A;
    const float* row = L.q + t * kPQ;
    // vec_act_k's draw: first argmax; explore iff !(u0 > eps); min(int(u1 A), A - 1)
    int best = 0;
    float bv = row[0];
    for (int k = 1; k < A; ++k)
      if (row[k] > bv) { bv = row[k]; best = k; }
    for (int k = 0; k < A; ++k) a.q[(size_t)e * A + k] = row[k];
    float u[4];
    uniform4(a.seed, (uint64_t)e, a.counter ? (uint64_t)a.counter[0] : 0ull, u);
    if (!(u[0] > a.eps[e])) {
      const int rr = (int)(u[1] * (float)A);
      best = rr < A ? rr : A - 1;
    }
    a.actions[e] = best;
  }
}

// ------------------------------------------------------------------ greedy act over host envs
// The act half of one evaluator step over HOST envs (engine/vector_host_eval.py), the wide
// vec_host_eval_act_k: vecw_act_k with the observations read straight from the staging block's
// reset_obs rows and the step k by value -- no ring, no hist, no counter in memory.  The live rows of
// a workgroup are one contiguous span of the block (rows N + e0 .. N + e0 + live - 1 of [2 N][obs]),
// so the x image is filled with no index read in front of the observation loads, a row's floats on
// consecutive lanes; a padding row repeats env N - 1 out of that span's last row.  Same forward, same
// draw at epsilon 0 (explore iff !(u0 > 0)): Q and the actions are vecw_act_k's bit for bit.
__global__ __launch_bounds__(kT) void vecw_host_eval_act_k(VecHostEvalAct a) {
  __shared__ WideLds L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows;
  const int obs = a.net.obs, kp = (obs + 7) & ~7;
  const int live = min(kRows, a.N - e0);   // >= 1: the grid is ceil(N / 32)
  const float* src = a.stage + (size_t)(a.N + e0) * obs;
  for (int i = t; i < kRows * kp; i += kT) {
    const int r = i / kp, k = i - r * kp;
    L.x[r * kPX + k] = k < obs ? src[min(r, live - 1) * obs + k] : 0.f;
  }
  vecw_forward(a.net, L);
  const int e = e0 + t;
  if (t < live) {
    const int A = a.net.A;
    const float* row = L.q + t * kPQ;
    // vecw_act_k's draw at eps = 0: first argmax; explore iff !(u0 > 0); min(int(u1 A), A - 1)
    int best = 0;
    float bv = row[0];
    for (int k = 1; k < A; ++k)
      if (row[k] > bv) { bv = row[k]; best = k; }
    for (int k = 0; k < A; ++k) a.q[(size_t)e * A + k] = row[k];
    float u[4];
    uniform4(a.seed, (uint64_t)e, (uint64_t)a.k, u);
    if (!(u[0] > 0.f)) {
      const int rr = (int)(u[1] * (float)A);
      best = rr < A ? rr : A - 1;
    }
    a.actions[e] = best;
  }
}

// ------------------------------------------------------------------ learner
__global__ __launch_bounds__(kT) void vecw_learn_k(VecLearn p) {
  __shared__ WideLds L;
  __shared__ float qt[kRows * kPQ];                   // target net on s'
  __shared__ float q2[kRows * kPQ];                   // online net on s'
  __shared__ __align__(16) float dA[kRows * kPA];     // dL/dA, zero in [A, 32)
  __shared__ float dV[kRows];
  __shared__ __align__(16) float dh[kRows * kPH];     // d(hidden pre-activation), both heads
  __shared__ int sid[kRows], sid2[kRows];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const int col = wave * 32 + r;
  const int b0 = blockIdx.x * kRows;
  const int obs = p.on.obs, A = p.on.A, kp = (obs + 7) & ~7;
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
  load_x(L, p.ring, obs, [&](int rr) { return sid2[rr]; });
  vecw_forward(p.tg, L);
  for (int i = t; i < kRows * kPQ; i += kT) qt[i] = L.q[i];
  vecw_forward(p.on, L);  // (s' is still in L.x)
  for (int i = t; i < kRows * kPQ; i += kT) q2[i] = L.q[i];
  load_x(L, p.ring, obs, [&](int rr) { return sid[rr]; });
  vecw_forward(p.on, L);  // online(s) last: its x / f / h stay for the backward
  if (t < kRows) {
    const int b = b0 + t;
    float g = 0.f;
    int a = 0;
    if (b < p.B) {
      const int row = p.idx[b];
      a = min(max(p.act[row], 0), A - 1);
      const float* qs = L.q + t * kPQ;
      const float* qn = q2 + t * kPQ;
      const float* qtn = qt + t * kPQ;
      int astar = 0;
      float best = qn[0];
      for (int k = 1; k < A; ++k)
        if (qn[k] > best) { best = qn[k]; astar = k; }
      // the arithmetic of dqn_loss_k
      const float y = p.rew[row] + p.gamma_n * qtn[astar] * (1.f - p.done[row]);
      const float qa = qs[a];
      const float delta = fabsf(y - qa);
      const float hub = delta < 1.f ? 0.5f * delta * delta : delta - 0.5f;
      p.delta[b] = delta;
      p.lw[b] = p.w[b] * hub;
      g = p.w[b] / (float)p.B * fminf(fmaxf(qa - y, -1.f), 1.f);
      for (int k = 0; k < A; ++k) {
        p.q_s[(size_t)b * A + k] = qs[k];
        p.q_s2[(size_t)b * A + k] = qn[k];
        p.qt_s2[(size_t)b * A + k] = qtn[k];
      }
    }
    // Q = V + A_a - mean(A): dV = g, dA_k = g (1[k == a] - 1/A)
    for (int k = 0; k < kVecWideMaxA; ++k)
      dA[t * kPA + k] = k < A ? g * ((k == a ? 1.f : 0.f) - 1.f / (float)A) : 0.f;
    dV[t] = g;
  }
  __syncthreads();
  {  // dH: advantage half on MFMA (K = A padded to 8), value half a rank-1 product
    f32x16 acc = {};
    tile_nn(acc, dA, kPA, (A + 7) & ~7, p.on.wa2 + col, A, lane);
    const float wv = p.on.wv2[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(i, hf);
      const float* hr = L.h + row * kPH;
      dh[row * kPH + col] = hr[col] > 0.f ? acc[i] : 0.f;
      dh[row * kPH + kH + col] = hr[kH + col] > 0.f ? dV[row] * wv : 0.f;
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
      if (b0 + row < p.B)
        p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::DF + col] = L.f[row * kPF + col] > 0.f ? acc[i] : 0.f;
    }
  }
  // the rest of the per-sample rows out of LDS, a row's floats on consecutive lanes
  const int live = min(kRows, p.B - b0);
  for (int i = t; i < live * kp; i += kT) {
    const int row = i / kp, k = i - row * kp;
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::X + k] = L.x[row * kPX + k];
  }
  for (int i = t; i < live * kH; i += kT) {
    const int row = i >> 7, k = i & (kH - 1);
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::F + k] = L.f[row * kPF + k];
  }
  for (int i = t; i < live * 2 * kH; i += kT) {
    const int row = i >> 8, k = i & (2 * kH - 1);
    float* v = p.vec + (size_t)(b0 + row) * vecw::STRIDE;
    v[vecw::H + k] = L.h[row * kPH + k];
    v[vecw::DH + k] = dh[row * kPH + k];
  }
  for (int i = t; i < live * (kVecWideMaxA + 1); i += kT) {
    const int row = i / (kVecWideMaxA + 1), k = i - row * (kVecWideMaxA + 1);
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::DA + k] = k < kVecWideMaxA ? dA[row * kPA + k] : dV[row];
  }
}

// ------------------------------------------------------------------ batch contraction
// The 32x32 output tile of workgroup `blk`: flat offsets of the weight and its bias, the tensor's
// shape, the vecw offsets of its left (output-gradient) and right (input) operands.
struct GradTile {
  int64_t woff, boff;
  int rows, cols, goff, xoff, m0, n0;
};

__device__ __forceinline__ GradTile grad_tile(int blk, int obs, int A) {
  const int nt0 = (obs + 31) / 32;
  const int64_t o1 = (int64_t)kH * obs, o2 = o1 + kH, o3 = o2 + kH * kH, o4 = o3 + kH, o5 = o4 + (int64_t)A * kH,
                o6 = o5 + A, o7 = o6 + kH * kH, o8 = o7 + kH, o9 = o8 + kH;
  GradTile g;
  int ntn;  // column blocks of the tensor
  if (blk < 4 * nt0)            { g = {0, o1, kH, obs, vecw::DF, vecw::X, 0, 0}; ntn = nt0; }
  else if ((blk -= 4 * nt0) < 16) { g = {o2, o3, kH, kH, vecw::DH, vecw::F, 0, 0}; ntn = 4; }
  else if ((blk -= 16) < 4)     { g = {o4, o5, A, kH, vecw::DA, vecw::H, 0, 0}; ntn = 4; }
  else if ((blk -= 4) < 16)     { g = {o6, o7, kH, kH, vecw::DH + kH, vecw::F, 0, 0}; ntn = 4; }
  else                          { blk -= 16; g = {o8, o9, 1, kH, vecw::DV, vecw::H + kH, 0, 0}; ntn = 4; }
  g.m0 = (blk / ntn) * 32;
  g.n0 = (blk % ntn) * 32;
  return g;
}

__global__ __launch_bounds__(kT) void vecw_grad_k(VecGrad g) {
  __shared__ float red[4][16][64];
  __shared__ float redb[4][32];
  __shared__ double sq[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const GradTile T = grad_tile(blockIdx.x, g.obs, g.A);
  // wave w contracts the batch range [w c, min(B, (w + 1) c)), c even: a k step is two samples
  const int chunk = (((g.B + 3) >> 2) + 1) & ~1;
  const int bs = wave * chunk, be = min(g.B, bs + chunk);
  const bool mok = T.m0 + r < T.rows, nok = T.n0 + r < T.cols;
  const float* pg = g.vec + T.goff + T.m0 + r;
  const float* px = g.vec + T.xoff + T.n0 + r;
  f32x16 acc = {};
  float bsum = 0.f;
  for (int b = bs; b < be; b += 8) {  // four k steps: their eight loads are issued before the MFMAs
    float av[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int bb = b + 2 * u + hf;
      const bool in = bb < be;  // the tail is zero operands: nothing is read past the range
      av[u] = in && mok ? pg[(size_t)bb * vecw::STRIDE] : 0.f;
      xv[u] = in && nok ? px[(size_t)bb * vecw::STRIDE] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc = mfma32(av[u], xv[u], acc);
      bsum += av[u];
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) red[wave][i][lane] = acc[i];
  bsum += __shfl_xor(bsum, 32, 64);  // the two half-waves' samples of unit m0 + r
  if (hf == 0) redb[wave][r] = bsum;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {  // the four waves' partials in wave order
    const int i = wave + 4 * qd;
    const float v = ((red[0][i][lane] + red[1][i][lane]) + red[2][i][lane]) + red[3][i][lane];
    const int row = T.m0 + acc_row(i, hf), c = T.n0 + r;
    if (row < T.rows && c < T.cols) {
      g.grad[T.woff + (int64_t)row * T.cols + c] = v;
      s += (double)v * (double)v;
    }
  }
  if (T.n0 == 0 && t < 32 && T.m0 + t < T.rows) {  // the bias: column sums of the left operand
    const float v = ((redb[0][t] + redb[1][t]) + redb[2][t]) + redb[3][t];
    g.grad[T.boff + T.m0 + t] = v;
    s += (double)v * (double)v;
  }
  s = wave_sum(s);
  if (lane == 0) sq[wave] = s;
  __syncthreads();
  if (t == 0) g.part[blockIdx.x] = (sq[0] + sq[1]) + (sq[2] + sq[3]);
}

void check_wide_net(const VecNet& n, const char* who) {
  if (n.obs < 1 || n.obs > kVecWideMaxObs || n.A < 1 || n.A > kVecWideMaxA)
    throw std::invalid_argument(std::string(who) + ": obs in [1, 128] and actions in [1, 32]");
  if (!n.w0 || !n.b0 || !n.wa1 || !n.ba1 || !n.wa2 || !n.ba2 || !n.wv1 || !n.bv1 || !n.wv2 || !n.bv2)
    throw std::invalid_argument(std::string(who) + ": missing parameter tensor");
}

}  // namespace

// ------------------------------------------------------------------ launchers
void vecw_act(const VecAct& a, hipStream_t s) {
  check_wide_net(a.net, "vecw_act");
  if (a.E < 1 || a.E > 4096 || !a.ring || !a.hist || !a.eps || !a.q || !a.actions)
    throw std::invalid_argument("vecw_act: 1 <= E <= 4096 with ring, hist, eps, q and actions");
  vecw_act_k<<<(a.E + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vecw_host_eval_act(const VecHostEvalAct& a, hipStream_t s) {
  check_wide_net(a.net, "vecw_host_eval_act");
  if (a.N < 1 || a.N > 64) throw std::invalid_argument("vecw_host_eval_act: 1 <= N <= 64 evaluator envs");
  if (a.k < 0) throw std::invalid_argument("vecw_host_eval_act: step k >= 0");
  if (!a.stage) throw std::invalid_argument("vecw_host_eval_act: the staging block's device copy");
  if (!a.q || !a.actions) throw std::invalid_argument("vecw_host_eval_act: q and actions");
  vecw_host_eval_act_k<<<(a.N + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vecw_learn(const VecLearn& p, hipStream_t s) {
  check_wide_net(p.on, "vecw_learn (online)");
  check_wide_net(p.tg, "vecw_learn (target)");
  if (p.on.obs != p.tg.obs || p.on.A != p.tg.A) throw std::invalid_argument("vecw_learn: nets differ in shape");
  if (p.B < 1 || p.B > 1024) throw std::invalid_argument("vecw_learn: batch must be in [1, 1024]");
  if (!p.ring || !p.s_ids || !p.s2_ids || !p.act || !p.rew || !p.done || !p.idx || !p.w || !p.q_s || !p.q_s2 ||
      !p.qt_s2 || !p.vec || !p.delta || !p.lw)
    throw std::invalid_argument("vecw_learn: missing buffer");
  if (p.beta_out && !(p.beta_horizon > 0.0)) throw std::invalid_argument("vecw_learn: beta horizon must be > 0");
  vecw_learn_k<<<(p.B + kRows - 1) / kRows, kT, 0, s>>>(p);
  LAUNCH_CHECK();
}

int vecw_grad_blocks(int obs, int A) {
  if (obs < 1 || obs > kVecWideMaxObs || A < 1 || A > kVecWideMaxA)
    throw std::invalid_argument("vecw_grad_blocks: obs in [1, 128] and actions in [1, 32]");
  return 4 * ((obs + 31) / 32) + 16 + 4 + 16 + 4;
}

void vecw_grad(const VecGrad& g, hipStream_t s) {
  if (g.obs < 1 || g.obs > kVecWideMaxObs || g.A < 1 || g.A > kVecWideMaxA || g.n != vec_param_count(g.obs, g.A))
    throw std::invalid_argument("vecw_grad: n must be the MLP dueling net's parameter count");
  if (g.B < 1 || g.B > 1024 || !g.vec || !g.grad || !g.part)
    throw std::invalid_argument("vecw_grad: batch in [1, 1024] with vec, grad and part");
  vecw_grad_k<<<vecw_grad_blocks(g.obs, g.A), kT, 0, s>>>(g);
  LAUNCH_CHECK();
}

}  // namespace apex
