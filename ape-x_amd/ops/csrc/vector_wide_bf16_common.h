// Device code shared by the bf16-operand kernels of the MLP dueling DQN: vector_wide_bf16_kernels.hip
// (obs <= 128, the observation tile whole in LDS) and vector_tall_bf16_kernels.hip (obs <= 1024, the
// observation streamed).  The precision contract, the operand scheme (one 16-byte LDS read per MFMA,
// weights packed from fp32 in registers), the LDS pitches and the summation orders are described in
// vector_wide_bf16_kernels.hip's header; everything here is inlined into its callers.
#pragma once
#include "common.h"
#include "kernels.h"

namespace apex {
namespace widebf16 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kH = kVecHidden;            // 128
constexpr int kT = 256;                   // threads of every workgroup here
constexpr int kRows = 32;                 // rows of a workgroup's tile
constexpr int kPX = kVecWideMaxObs + 8;   // 136 bf16 = 17 16-byte slots
constexpr int kPF = kH + 8;               // 136
constexpr int kPH = 2 * kH + 8;           // 264 = 33 slots
constexpr int kPQ = kVecWideMaxA + 1;     // 33 floats (scalar reads down a column)
constexpr int kPA = kVecWideMaxA + 8;     // 40 bf16 = 5 slots
constexpr int kPAf = kVecWideMaxA + 1;    // 33 floats: dA | dV of a row as they go to memory
constexpr int kRound = 4;                 // step groups (of 16 k) whose operand loads are in flight together

__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// accumulator register i of half-wave hf -> tile row (the 32x32 C/D map; column = lane & 31)
__device__ __forceinline__ int acc_row(int i, int hf) { return (i & 3) + 8 * (i >> 2) + 4 * hf; }

// round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ __bf16 to_bf16(float v) { return static_cast<__bf16>(v); }
__device__ __forceinline__ bf16x8 pack8(f32x8 v) { return __builtin_convertvector(v, bf16x8); }

__device__ __forceinline__ bool rows_aligned16(const float* w, int ld) {
  return ((reinterpret_cast<uintptr_t>(w) & 15) == 0) && (ld & 3) == 0;
}

__device__ __forceinline__ int pad16(int k) { return (k + 15) & ~15; }

// w[k .. k + 7] of a weight row of kw floats as fp32 (null: a zero row); elements >= kw are zero and
// are not read.  vec: the row is 16-byte aligned and kw a multiple of 4.
__device__ __forceinline__ f32x8 ldw8(const float* w, int k, int kw, bool vec) {
  f32x8 v = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (!w) return v;
  if (vec) {
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    if (k < kw) lo = *reinterpret_cast<const f32x4*>(w + k);
    if (k + 4 < kw) hi = *reinterpret_cast<const f32x4*>(w + k + 4);
    v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (k + i < kw) v[i] = w[k + i];
  }
  return v;
}

// this lane's A operands of a round: act[r][k0 + 16 j + 8 hf .. + 7], zero for a group past kp
__device__ __forceinline__ void lds_a(bf16x8 (&a)[kRound], const __bf16* arow, int k0, int kp) {
  const bf16x8 z = pack8(f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f});
#pragma unroll
  for (int j = 0; j < kRound; ++j) {
    const int k = k0 + 16 * j;
    a[j] = k < kp ? *reinterpret_cast<const bf16x8*>(arow + k) : z;
  }
}

// acc[t] += act[32][kp] . W_t^T for NT weight blocks that share the activation: wrow[t] is THIS
// lane's weight row (unit n0_t + lane % 32) of kw floats.  act: LDS bf16, zero in [kw, kp); kp is a
// multiple of 16.
template <int NT>
__device__ __forceinline__ void tile_nt(f32x16 (&acc)[NT], const __bf16* act, int pitch, int kp,
                                        const float* const (&wrow)[NT], int kw, const bool (&vec)[NT], int lane) {
  const int r = lane & 31, hf = lane >> 5;
  const __bf16* arow = act + r * pitch + 8 * hf;
  for (int k0 = 0; k0 < kp; k0 += 16 * kRound) {  // a round's loads are all issued before its MFMAs
    bf16x8 a[kRound];
    f32x8 b[NT][kRound];
#pragma unroll
    for (int j = 0; j < kRound; ++j) {
      const int k = k0 + 16 * j;  // a group past kp is zero operands (wave-uniform): nothing is read
#pragma unroll
      for (int t = 0; t < NT; ++t) b[t][j] = ldw8(k < kp ? wrow[t] : nullptr, k + 8 * hf, kw, vec[t]);
    }
    lds_a(a, arow, k0, kp);
#pragma unroll
    for (int j = 0; j < kRound; ++j) {
      if (k0 + 16 * j < kp) {  // (wave-uniform: a short K issues no MFMA on zero groups)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma16(a[j], pack8(b[t][j]), acc[t]);
      }
    }
  }
}

// acc += act[32][kp] . W[0 .. kv)[n]: the weight untransposed, wcol = W + this lane's column
// (row pitch kH); rows >= kv are zero operands and are not read.  act: LDS bf16, zero in [kv, kp).
__device__ __forceinline__ void tile_nn(f32x16& acc, const __bf16* act, int pitch, int kp, const float* wcol, int kv,
                                        int lane) {
  const int r = lane & 31, hf = lane >> 5;
  const __bf16* arow = act + r * pitch + 8 * hf;
  for (int k0 = 0; k0 < kp; k0 += 16 * kRound) {
    bf16x8 a[kRound];
    f32x8 b[kRound];
#pragma unroll
    for (int j = 0; j < kRound; ++j) {
      const int k = k0 + 16 * j;  // a group past kp is zero operands (wave-uniform): nothing is read
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int u = k + 8 * hf + i;
        b[j][i] = k < kp && u < kv ? wcol[(size_t)u * kH] : 0.f;
      }
    }
    lds_a(a, arow, k0, kp);
#pragma unroll
    for (int j = 0; j < kRound; ++j) {
      if (k0 + 16 * j < kp) acc = mfma16(a[j], pack8(b[j]), acc);
    }
  }
}

// ------------------------------------------------------------------ forward after features.0
// Q of the 32 rows whose rounded relu(features.0) is f [32][kPF] -> h [32][kPH] (relu(advantage.0) |
// relu(value.0), rounded), adv [32][kPQ], val [32], q [32][kPQ], all LDS.  Begins (f is complete) and
// ends with a workgroup barrier.
__device__ __forceinline__ void heads_b(const VecNet& n, const __bf16* f, __bf16* h, float* adv, float* val,
                                        float* q) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const int col = wave * 32 + r;
  __syncthreads();
  {  // advantage.0 | value.0 as one N = 256 GEMM: wave w owns block w of each head
    f32x16 acc[2] = {};
    const float* const wrow[2] = {n.wa1 + (size_t)col * kH, n.wv1 + (size_t)col * kH};
    const bool vec[2] = {rows_aligned16(n.wa1, kH), rows_aligned16(n.wv1, kH)};
    tile_nt<2>(acc, f, kPF, kH, wrow, kH, vec, lane);
    const float ba = n.ba1[col], bv = n.bv1[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      __bf16* hr = h + acc_row(i, hf) * kPH;
      hr[col] = to_bf16(fmaxf(acc[0][i] + ba, 0.f));
      hr[kH + col] = to_bf16(fmaxf(acc[1][i] + bv, 0.f));
    }
  }
  __syncthreads();
  if (wave < 2) {  // advantage.2 (wave 0: units < A) and value.2 (wave 1: unit 0), one tile each
    f32x16 acc[1] = {};
    const bool live = wave == 0 ? r < n.A : r == 0;
    const float* w = wave == 0 ? n.wa2 : n.wv2;
    const float* const wrow[1] = {live ? w + (size_t)r * kH : nullptr};
    const bool vec[1] = {rows_aligned16(w, kH)};
    tile_nt<1>(acc, h + wave * kH, kPH, kH, wrow, kH, vec, lane);
    if (live) {
      const float b = wave == 0 ? n.ba2[r] : n.bv2[0];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, hf);
        if (wave == 0) adv[row * kPQ + r] = acc[0][i] + b;
        else val[row] = acc[0][i] + b;
      }
    }
  }
  __syncthreads();
  if (t < kRows) {  // dueling combine of row t
    const float* ar = adv + t * kPQ;
    float advsum = 0.f;
    for (int o = 0; o < n.A; ++o) advsum += ar[o];
    const float mean = advsum / (float)n.A, v = val[t];
    for (int o = 0; o < n.A; ++o) q[t * kPQ + o] = v + ar[o] - mean;
  }
  __syncthreads();
}

// a Q row -> q[e][0 .. A) and vec_act_k's draw: first argmax; explore iff !(u0 > eps);
// min(int(u1 A), A - 1)
__device__ __forceinline__ void draw(const float* row, int e, int A, float eps, uint64_t seed, uint64_t counter,
                                     float* q, int* actions) {
  int best = 0;
  float bv = row[0];
  for (int k = 1; k < A; ++k)
    if (row[k] > bv) { bv = row[k]; best = k; }
  for (int k = 0; k < A; ++k) q[(size_t)e * A + k] = row[k];
  float u[4];
  uniform4(seed, (uint64_t)e, counter, u);
  if (!(u[0] > eps)) {
    const int rr = (int)(u[1] * (float)A);
    best = rr < A ? rr : A - 1;
  }
  actions[e] = best;
}

// ------------------------------------------------------------------ loss and backward of 32 rows
// The learner's second half for the workgroup's rows b0 .. b0 + 31: dqn_loss_k's per-row loss from
// q (online, s), q2 (online, s') and qt (target, s'), then dH and dF on MFMA with online(s)'s rounded
// f / h still in LDS, and the per-sample rows (vecw layout, fp32 in memory) except the observation.
// dAf [32][kPAf], dA [32][kPA], dh [32][kPH]: LDS scratch.  Called after a workgroup barrier.
__device__ __forceinline__ void loss_backward_b(const VecLearn& p, int b0, const __bf16* f, const __bf16* h,
                                                const float* q, const float* qt, const float* q2, float* dAf,
                                                __bf16* dA, __bf16* dh) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const int col = wave * 32 + r;
  const int A = p.on.A;
  if (t < kRows) {
    const int b = b0 + t;
    float g = 0.f;
    int a = 0;
    if (b < p.B) {
      const int row = p.idx[b];
      a = min(max(p.act[row], 0), A - 1);
      const float* qs = q + t * kPQ;
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
    for (int k = 0; k < kVecWideMaxA; ++k) {
      const float d = k < A ? g * ((k == a ? 1.f : 0.f) - 1.f / (float)A) : 0.f;
      dAf[t * kPAf + k] = d;
      dA[t * kPA + k] = to_bf16(d);
    }
    dAf[t * kPAf + kVecWideMaxA] = g;
  }
  __syncthreads();
  {  // dH: advantage half on MFMA (K = A padded to 16), value half a rank-1 product of rounded factors
    f32x16 acc = {};
    tile_nn(acc, dA, kPA, pad16(A), p.on.wa2 + col, A, lane);
    const float wv = (float)to_bf16(p.on.wv2[col]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(i, hf);
      const __bf16* hr = h + row * kPH;
      const float dv = (float)to_bf16(dAf[row * kPAf + kVecWideMaxA]);
      dh[row * kPH + col] = to_bf16((float)hr[col] > 0.f ? acc[i] : 0.f);
      dh[row * kPH + kH + col] = to_bf16((float)hr[kH + col] > 0.f ? dv * wv : 0.f);
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
        p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::DF + col] = (float)f[row * kPF + col] > 0.f ? acc[i] : 0.f;
    }
  }
  // the rest of the per-sample rows out of LDS (fp32 in memory), a row's floats on consecutive lanes
  const int live = min(kRows, p.B - b0);
  for (int i = t; i < live * kH; i += kT) {
    const int row = i >> 7, k = i & (kH - 1);
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::F + k] = (float)f[row * kPF + k];
  }
  for (int i = t; i < live * 2 * kH; i += kT) {
    const int row = i >> 8, k = i & (2 * kH - 1);
    float* v = p.vec + (size_t)(b0 + row) * vecw::STRIDE;
    v[vecw::H + k] = (float)h[row * kPH + k];
    v[vecw::DH + k] = (float)dh[row * kPH + k];
  }
  for (int i = t; i < live * kPAf; i += kT) {  // (DV = DA + 32)
    const int row = i / kPAf, k = i - row * kPAf;
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::DA + k] = dAf[i];
  }
}

// ------------------------------------------------------------------ batch contraction
// The 32x32 output tile of workgroup `blk` (vecw_grad's map; the tall grid only has more tiles of
// dW0): flat offsets of the weight and its bias, the tensor's shape, the vecw offsets of its left
// (output-gradient) and right (input) operands.
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

constexpr int kGradSteps = 2;  // k steps (of 16 samples) whose 16 loads each are in flight together

// wave w of a contraction workgroup takes the batch range [w c, min(B, (w + 1) c)), c a multiple of
// 16: a k step is 16 samples
__device__ __forceinline__ int grad_chunk(int B) { return (((B + 3) >> 2) + 15) & ~15; }

struct GradRed {
  float red[4][16][64];
  float redb[4][32];
  double sq[4];
};

// The four waves' partial tiles (acc) and partial column sums of the left operand (bsum, per lane)
// reduced through LDS in wave order -> the tile of the weight gradient, the bias gradient (tiles of
// the first column block, fp32) and the workgroup's fp64 sum-of-squares partial.
__device__ __forceinline__ void grad_finish(GradRed& R, const f32x16& acc, float bsum, const GradTile& T,
                                            float* grad, double* part) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
#pragma unroll
  for (int i = 0; i < 16; ++i) R.red[wave][i][lane] = acc[i];
  bsum += __shfl_xor(bsum, 32, 64);  // the two half-waves' samples of unit m0 + r
  if (hf == 0) R.redb[wave][r] = bsum;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {  // the four waves' partials in wave order
    const int i = wave + 4 * qd;
    const float v = ((R.red[0][i][lane] + R.red[1][i][lane]) + R.red[2][i][lane]) + R.red[3][i][lane];
    const int row = T.m0 + acc_row(i, hf), c = T.n0 + r;
    if (row < T.rows && c < T.cols) {
      grad[T.woff + (int64_t)row * T.cols + c] = v;
      s += (double)v * (double)v;
    }
  }
  if (T.n0 == 0 && t < 32 && T.m0 + t < T.rows) {  // the bias: column sums of the left operand (fp32)
    const float v = ((R.redb[0][t] + R.redb[1][t]) + R.redb[2][t]) + R.redb[3][t];
    grad[T.boff + T.m0 + t] = v;
    s += (double)v * (double)v;
  }
  s = wave_sum(s);
  if (lane == 0) R.sq[wave] = s;
  __syncthreads();
  if (t == 0) part[blockIdx.x] = (R.sq[0] + R.sq[1]) + (R.sq[2] + R.sq[3]);
}

}  // namespace widebf16
}  // namespace apex
