// The wide MLP dueling DQN of vector_wide_kernels.hip with bf16 matrix-core operands, opt-in
// (VectorEngineConfig.wide_dtype = "bf16"): obs <= 128, A <= 32, hidden 128, batches to 1024.
//
// Precision: "bf16 x bf16 -> fp32 accumulate" on v_mfma_f32_32x32x16_bf16.  Master parameters, the
// target net, biases, Q, the dueling combine, the loss, priorities, the flat gradient, the fp64 norm
// partials and the optimizer stay fp32.  Every matrix-core operand is rounded to bf16 (nearest even,
// v_cvt_pk_bf16_f32) where it becomes an operand: the observation row x, every weight element,
// f = relu(features.0), h = relu(advantage.0 | value.0); in the backward dA | dV, dh and the weights
// again; in vecwb_grad both operands.  Bias add and ReLU act on the fp32 accumulator before the
// rounding; the backward's ReLU masks come from the stored (rounded) activation.  The accumulation
// order is fixed by the code -- no atomics, bit-identical reruns.
//
//   forward       a workgroup of 4 waves owns 32 rows.  The activations live in LDS as bf16 images
//                 (x [32][136], f [32][136], h [32][264]: row pitches of 17 / 17 / 33 16-byte slots,
//                 odd, so the 32 rows of a ds_read_b128 fall into distinct slots).  One MFMA reduces
//                 16 k: in step group j the half-wave hf = lane / 32 holds k = 16j + 8hf .. + 7, so
//                 the A operand of an MFMA is ONE 16-byte LDS read and K = 128 is 8 MFMAs per 32x32
//                 tile (the fp32 kernels: 64).  There is no bf16 shadow of the weights: a lane reads
//                 its weight row's 8 consecutive fp32 from global (two 16-byte loads; dword loads
//                 where rows are not 16-byte aligned: features.0 at obs % 4 != 0, value.0 in the flat
//                 vector at A % 4 != 0) and packs them in registers, so the optimizer, target sync
//                 and publish are untouched and a step keeps its launch count.  A round is 4 step
//                 groups (64 k): its raw fp32 weight loads are all in flight before its first
//                 convert and MFMA.  K is padded with zeros to a multiple of 16 in LDS only; weights
//                 are never read past obs.  The epilogue converts fmaxf(acc + b, 0) once and writes
//                 bf16 into the next layer's image.  advantage.2 / value.2 are one tile each on
//                 waves 0 / 1, then the fp32 dueling combine in vec_forward's order.
//   vecwb_act, vecwb_host_eval_act   vecw_act's / vecw_host_eval_act's geometry and draw over this
//                 forward.
//   vecwb_learn   target(s'), online(s'), online(s); dqn_loss_k's per-row loss; the backward on the
//                 same MFMA with the weights untransposed: dH = (dA . Wa2 | dV wv2) * relu',
//                 dF = (dHa . Wa1 + dHv . Wv1) * relu'.  The lanes run along n; a lane gathers its
//                 column's 8 consecutive u (strided dword loads, coalesced across the half-wave) and
//                 packs them; rows >= kv are zero operands and are not read.  dA (K = A padded to 16)
//                 and dh are bf16 LDS images too.  The per-sample rows (vecw layout) stay fp32 in
//                 memory: x, f, h and dh are written as the rounded values the MFMAs consumed, dF
//                 from the accumulators, dA | dV as computed.
//   vecwb_grad    vecw_grad's tiling (one workgroup per 32x32 output tile, four batch ranges,
//                 wave-order LDS reduction, bias-gradient column sums in fp32, one fp64 sum-of-squares
//                 partial per workgroup) with K = batch on the bf16 MFMA: a lane takes 8 consecutive
//                 batch rows of its column for each operand and packs them; a ragged B is padded
//                 with zero operands.
#include "common.h"
#include "kernels.h"

namespace apex {

namespace {

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

// ------------------------------------------------------------------ forward
struct alignas(16) WideLdsB {
  __bf16 x[kRows * kPX];
  __bf16 f[kRows * kPF];    // relu(features.0)
  __bf16 h[kRows * kPH];    // relu(advantage.0) | relu(value.0)
  float adv[kRows * kPQ];
  float val[kRows];
  float q[kRows * kPQ];
};

__device__ __forceinline__ int pad16(int k) { return (k + 15) & ~15; }

// x rows of the workgroup: row r is src(r)[0 .. obs), rounded; columns [obs, pad16(obs)) are zero
template <class Src>
__device__ __forceinline__ void load_x(WideLdsB& L, int obs, Src src) {
  const int kp = pad16(obs);
  for (int i = threadIdx.x; i < kRows * kp; i += kT) {
    const int r = i / kp, k = i - r * kp;
    L.x[r * kPX + k] = to_bf16(k < obs ? src(r)[k] : 0.f);
  }
}

// Q of the 32 rows in L.x -> L.f, L.h, L.q.  Begins and ends with a workgroup barrier.  Inlined: an
// out-of-line copy takes the net's pointers by address, through private memory.
__device__ __forceinline__ void vecwb_forward(const VecNet& n, WideLdsB& L) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const int col = wave * 32 + r;
  __syncthreads();
  {  // features.0: wave w owns units 32w .. 32w + 31
    f32x16 acc[1] = {};
    const float* const wrow[1] = {n.w0 + (size_t)col * n.obs};
    const bool vec[1] = {rows_aligned16(n.w0, n.obs)};
    tile_nt<1>(acc, L.x, kPX, pad16(n.obs), wrow, n.obs, vec, lane);
    const float b = n.b0[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) L.f[acc_row(i, hf) * kPF + col] = to_bf16(fmaxf(acc[0][i] + b, 0.f));
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
      __bf16* hr = L.h + acc_row(i, hf) * kPH;
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

// row t of L.q -> q[e][0 .. A) and vec_act_k's draw: first argmax; explore iff !(u0 > eps);
// min(int(u1 A), A - 1)
__device__ __forceinline__ void draw(const WideLdsB& L, int t, int e, int A, float eps, uint64_t seed,
                                     uint64_t counter, float* q, int* actions) {
  const float* row = L.q + t * kPQ;
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

// ------------------------------------------------------------------ acting
__global__ __launch_bounds__(kT) void vecwb_act_k(VecAct a) {
  __shared__ WideLdsB L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows;
  // rows past E repeat the last env (never written)
  load_x(L, a.net.obs,
         [&](int r) { return a.ring + (size_t)a.hist[min(e0 + r, a.E - 1) * 4 + 3] * a.net.obs; });
  vecwb_forward(a.net, L);
  const int e = e0 + t;
  if (t < kRows && e < a.E)
    draw(L, t, e, a.net.A, a.eps[e], a.seed, a.counter ? (uint64_t)a.counter[0] : 0ull, a.q, a.actions);
}

// vecw_host_eval_act_k over the bf16 forward: the live rows of a workgroup are rows N + e0 ..
// N + e0 + live - 1 of the staging block's [2 N][obs]; a padding row repeats the span's last row.
__global__ __launch_bounds__(kT) void vecwb_host_eval_act_k(VecHostEvalAct a) {
  __shared__ WideLdsB L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows;
  const int obs = a.net.obs;
  const int live = min(kRows, a.N - e0);   // >= 1: the grid is ceil(N / 32)
  const float* src = a.stage + (size_t)(a.N + e0) * obs;
  load_x(L, obs, [&](int r) { return src + (size_t)min(r, live - 1) * obs; });
  vecwb_forward(a.net, L);
  if (t < live) draw(L, t, e0 + t, a.net.A, 0.f, a.seed, (uint64_t)a.k, a.q, a.actions);
}

// ------------------------------------------------------------------ learner
__global__ __launch_bounds__(kT) void vecwb_learn_k(VecLearn p) {
  __shared__ WideLdsB L;
  __shared__ float qt[kRows * kPQ];                   // target net on s'
  __shared__ float q2[kRows * kPQ];                   // online net on s'
  __shared__ float dAf[kRows * kPAf];                 // dL/dA [0, 32) | dL/dV, fp32 (to memory)
  __shared__ __align__(16) __bf16 dA[kRows * kPA];    // dL/dA rounded, zero in [A, 32)
  __shared__ __align__(16) __bf16 dh[kRows * kPH];    // d(hidden pre-activation), both heads, rounded
  __shared__ int sid[kRows], sid2[kRows];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const int col = wave * 32 + r;
  const int b0 = blockIdx.x * kRows;
  const int obs = p.on.obs, A = p.on.A;
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
  load_x(L, obs, [&](int rr) { return p.ring + (size_t)sid2[rr] * obs; });
  vecwb_forward(p.tg, L);
  for (int i = t; i < kRows * kPQ; i += kT) qt[i] = L.q[i];
  vecwb_forward(p.on, L);  // (s' is still in L.x)
  for (int i = t; i < kRows * kPQ; i += kT) q2[i] = L.q[i];
  load_x(L, obs, [&](int rr) { return p.ring + (size_t)sid[rr] * obs; });
  vecwb_forward(p.on, L);  // online(s) last: its x / f / h stay for the backward
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
      const __bf16* hr = L.h + row * kPH;
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
        p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::DF + col] = (float)L.f[row * kPF + col] > 0.f ? acc[i] : 0.f;
    }
  }
  // the rest of the per-sample rows out of LDS (fp32 in memory), a row's floats on consecutive lanes
  const int live = min(kRows, p.B - b0);
  for (int i = t; i < live * obs; i += kT) {
    const int row = i / obs, k = i - row * obs;
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::X + k] = (float)L.x[row * kPX + k];
  }
  for (int i = t; i < live * kH; i += kT) {
    const int row = i >> 7, k = i & (kH - 1);
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::F + k] = (float)L.f[row * kPF + k];
  }
  for (int i = t; i < live * 2 * kH; i += kT) {
    const int row = i >> 8, k = i & (2 * kH - 1);
    float* v = p.vec + (size_t)(b0 + row) * vecw::STRIDE;
    v[vecw::H + k] = (float)L.h[row * kPH + k];
    v[vecw::DH + k] = (float)dh[row * kPH + k];
  }
  for (int i = t; i < live * kPAf; i += kT) {  // (DV = DA + 32)
    const int row = i / kPAf, k = i - row * kPAf;
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::DA + k] = dAf[i];
  }
}

// ------------------------------------------------------------------ batch contraction
// The 32x32 output tile of workgroup `blk` (vecw_grad's map, vecw_grad_blocks(obs, A) tiles): flat
// offsets of the weight and its bias, the tensor's shape, the vecw offsets of its left
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

__global__ __launch_bounds__(kT) void vecwb_grad_k(VecGrad g) {
  __shared__ float red[4][16][64];
  __shared__ float redb[4][32];
  __shared__ double sq[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const GradTile T = grad_tile(blockIdx.x, g.obs, g.A);
  // wave w contracts the batch range [w c, min(B, (w + 1) c)), c a multiple of 16: a k step is 16 samples
  const int chunk = (((g.B + 3) >> 2) + 15) & ~15;
  const int bs = wave * chunk, be = min(g.B, bs + chunk);
  const bool mok = T.m0 + r < T.rows, nok = T.n0 + r < T.cols;
  const float* pg = g.vec + T.goff + T.m0 + r;
  const float* px = g.vec + T.xoff + T.n0 + r;
  f32x16 acc = {};
  float bsum = 0.f;
  for (int b = bs; b < be; b += 16 * kGradSteps) {
    f32x8 av[kGradSteps], xv[kGradSteps];
#pragma unroll
    for (int u = 0; u < kGradSteps; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int bb = b + 16 * u + 8 * hf + i;
        const bool in = bb < be;  // the tail is zero operands: nothing is read past the range
        av[u][i] = in && mok ? pg[(size_t)bb * vecw::STRIDE] : 0.f;
        xv[u][i] = in && nok ? px[(size_t)bb * vecw::STRIDE] : 0.f;
      }
#pragma unroll
    for (int u = 0; u < kGradSteps; ++u) {
      if (b + 16 * u < be) acc = mfma16(pack8(av[u]), pack8(xv[u]), acc);  // (wave-uniform)
#pragma unroll
      for (int i = 0; i < 8; ++i) bsum += av[u][i];
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
  if (T.n0 == 0 && t < 32 && T.m0 + t < T.rows) {  // the bias: column sums of the left operand (fp32)
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
void vecwb_act(const VecAct& a, hipStream_t s) {
  check_wide_net(a.net, "vecwb_act");
  if (a.E < 1 || a.E > 4096 || !a.ring || !a.hist || !a.eps || !a.q || !a.actions)
    throw std::invalid_argument("vecwb_act: 1 <= E <= 4096 with ring, hist, eps, q and actions");
  vecwb_act_k<<<(a.E + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vecwb_host_eval_act(const VecHostEvalAct& a, hipStream_t s) {
  check_wide_net(a.net, "vecwb_host_eval_act");
  if (a.N < 1 || a.N > 64) throw std::invalid_argument("vecwb_host_eval_act: 1 <= N <= 64 evaluator envs");
  if (a.k < 0) throw std::invalid_argument("vecwb_host_eval_act: step k >= 0");
  if (!a.stage) throw std::invalid_argument("vecwb_host_eval_act: the staging block's device copy");
  if (!a.q || !a.actions) throw std::invalid_argument("vecwb_host_eval_act: q and actions");
  vecwb_host_eval_act_k<<<(a.N + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vecwb_learn(const VecLearn& p, hipStream_t s) {
  check_wide_net(p.on, "vecwb_learn (online)");
  check_wide_net(p.tg, "vecwb_learn (target)");
  if (p.on.obs != p.tg.obs || p.on.A != p.tg.A) throw std::invalid_argument("vecwb_learn: nets differ in shape");
  if (p.B < 1 || p.B > 1024) throw std::invalid_argument("vecwb_learn: batch must be in [1, 1024]");
  if (!p.ring || !p.s_ids || !p.s2_ids || !p.act || !p.rew || !p.done || !p.idx || !p.w || !p.q_s || !p.q_s2 ||
      !p.qt_s2 || !p.vec || !p.delta || !p.lw)
    throw std::invalid_argument("vecwb_learn: missing buffer");
  if (p.beta_out && !(p.beta_horizon > 0.0)) throw std::invalid_argument("vecwb_learn: beta horizon must be > 0");
  vecwb_learn_k<<<(p.B + kRows - 1) / kRows, kT, 0, s>>>(p);
  LAUNCH_CHECK();
}

void vecwb_grad(const VecGrad& g, hipStream_t s) {
  if (g.obs < 1 || g.obs > kVecWideMaxObs || g.A < 1 || g.A > kVecWideMaxA || g.n != vec_param_count(g.obs, g.A))
    throw std::invalid_argument("vecwb_grad: n must be the MLP dueling net's parameter count");
  if (g.B < 1 || g.B > 1024 || !g.vec || !g.grad || !g.part)
    throw std::invalid_argument("vecwb_grad: batch in [1, 1024] with vec, grad and part");
  vecwb_grad_k<<<vecw_grad_blocks(g.obs, g.A), kT, 0, s>>>(g);
  LAUNCH_CHECK();
}

}  // namespace apex
