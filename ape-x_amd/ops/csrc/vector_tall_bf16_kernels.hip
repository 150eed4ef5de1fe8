// Tall mode of the wide MLP dueling DQN with bf16 matrix-core operands (VectorEngineConfig.tall_dtype =
// "bf16"): obs <= 1024 (kVecTallMaxObs), A <= 32, hidden 128, batches to 1024.  The fourth corner beside
// vecw_* (fp32, obs <= 128), vecwb_* (bf16, obs <= 128) and vect_* (fp32, streamed): vect_*'s streaming
// under vecwb_*'s precision contract (the header of vector_wide_bf16_kernels.hip), unchanged -- every
// matrix-core operand rounded to bf16, nearest even, where it becomes an operand; accumulation, bias,
// ReLU, Q, the combine, loss, priorities, the flat gradient and the fp64 norm partials fp32; no bf16
// shadow of the weights; no atomics, bit-identical reruns.
//
// v_mfma_f32_32x32x16_bf16 contracts 128 k in 8 instructions where the fp32 kernels issue 64, so
// features.0 is bound by its operand traffic, not by the matrix core, and the streaming is laid out for
// that:
//
//   tall_features_b (device) a workgroup of 4 waves owns 32 rows; wave w owns units 32w .. 32w + 31 of
//                 features.0 for NT nets at once (one f32x16 accumulator per net, alive across the
//                 whole observation; NT = 2: target and online net on s').
//                 x: slabs of 256 columns as a bf16 LDS image, double-buffered ([2][32][264]: the fp32
//                 slab's footprint at twice the columns, half the barriers; the pitch is 33 16-byte
//                 slots, odd, so the 32 rows of a ds_read_b128 fall in distinct slots).  A thread owns 4
//                 octets of a slab, a row's 256 floats on the 32 lanes of a half-wave.  The global loads
//                 stay fp32 (two 16-byte loads per octet when the rows are 16-byte aligned, dword loads
//                 otherwise), are issued before the current slab's MFMAs, and are converted
//                 (v_cvt_pk_bf16_f32) and stored with one 16-byte LDS write per octet to the other
//                 buffer after them; one barrier per slab.  The last slab is zero beyond obs in LDS only
//                 and contracts pad16(obs - 256 s) columns; neither x nor a weight is read at or past
//                 obs.
//                 W0: a lane reads 8 consecutive fp32 of its row per MFMA and packs them in registers.
//                 A round is R step groups of 16 k (R = 4 for NT = 1, 2 for NT = 2: 32 raw registers).
//                 Two raw register sets alternate, and the pipeline runs over the whole observation,
//                 across slabs and barriers: round g + 1's loads are issued before round g's converts
//                 and MFMAs, so a round waits only on loads issued a whole round earlier.  No branch or
//                 select stands between a load and its use: the address of an element at or past obs is
//                 clamped below obs, and the element is replaced by zero where its octet is converted
//                 (the straddling round and the last slab only).
//                 The epilogue writes to_bf16(fmaxf(acc + b, 0)) into the next layer's bf16 image.
//   vectb_act / vectb_host_eval_act   vect_act / vect_host_eval_act on that forward; heads, combine and
//                 draw are vecwb's (vector_wide_bf16_common.h).
//   vectb_learn   vect_learn's order: s' streamed once for both nets (the online features of s' wait in
//                 the dh image), the two head passes, then online(s) last so that its f / h stay in LDS
//                 for vecwb's loss and backward.  The per-sample rows (vecw layout, fp32 in memory): f, h
//                 and dh as the rounded values the MFMAs consumed, dF from the accumulators, dA | dV as
//                 computed; vecw::X is never written.
//   vectb_grad    vecwb_grad's tiling on vect_grad's grid (vect_grad_blocks(obs, A) workgroups, four
//                 batch ranges, wave-order LDS reduction, fp32 bias sums, one fp64 partial per
//                 workgroup): K = batch on the bf16 MFMA, 8 consecutive batch rows per lane and operand,
//                 kGradSteps k steps of gathered loads in flight.  The 4 ceil(obs / 32) tiles of dW0 take
//                 their right operand from the ring through frame ids staged once per workgroup in LDS;
//                 each value is rounded as it is packed -- the bf16 value the forward consumed.
//
// The bf16 ring (VectorEngineConfig.ring_dtype = "bf16"; ring_bf16 in the VecAct / VecLearn / VecTallGrad
// handles picks the <__bf16> instantiation of vectb_act / vectb_learn / vectb_grad, the <float> one is the code
// above, instruction for instruction).  vec_host_tail has rounded each row once, nearest even, where it wrote
// it -- the rounding the fp32 path applies at every read -- so the ring holds the operand bits and every
// number these kernels produce is bit-equal to the fp32 ring's:
//
//   tall_features_b  the slab path has a load of its own (Slab<__bf16, XW>): an octet is ONE 16-byte load of
//                 8 columns when the rows are 16-byte aligned (obs % 8 == 0): 4 loads and 16 raw registers
//                 per thread and slab where the fp32 ring takes 8 and 32; two 8-byte loads per octet when
//                 obs % 4 == 0, 2-byte loads otherwise.  Addresses are clamped below obs as before; the
//                 elements at and past obs are zeroed on the raw 16-bit lanes (a dword AND / select per
//                 load) where the octet goes to LDS, one ds_write_b128 of the loaded bits.  No v_cvt on
//                 the x side.  Same slabs, seams, barriers, W0 pipeline and summation order.
//                 Prefetch depth: ONE slab of x in flight, as over the fp32 ring.  The 16 freed registers
//                 were not spent on a second slab: the x side is not what bounds the kernel (at obs 1024 /
//                 B 512 halving its bytes moves vectb_learn by 1.3%, profiles/vector_tall_bf16_ring.md);
//                 the W0 stream is, and it is unchanged.
//   vectb_grad    the dW0 tiles gather 2-byte elements straight into the MFMA operand (grad_ring_b): no
//                 rounding at pack time.  Grid, batch ranges, reduction, bias sums and the norm partial
//                 are the same code.
//
// LDS per workgroup (static): slabs 33,792 + f 8,704 + h 16,896 + adv / val / q 8,576 = 67,968 B, + 128 B
// of row ids: vectb_act 68,096 B (vectb_host_eval_act 67,968 B).  vectb_learn adds qt / q2 8,448,
// dA fp32 4,224, dA bf16 2,560, dh 16,896 and 256 B of ids: 100,352 B of gfx950's 163,840.  vectb_grad:
// 16,928 B of reduction images + 4,096 B of ids.  The <__bf16> instantiations: the same totals (68,096 /
// 100,352 / 21,024 B in the compiler's listing); VGPRs 159 / 196 / 56 against 173 / 210 / 70, no scratch.
#include <type_traits>

#include "vector_wide_bf16_common.h"

namespace apex {

namespace {

using namespace widebf16;

constexpr int kSlab = 256;                       // columns of x per slab
constexpr int kPS = kSlab + 8;                   // 264 bf16 = 33 16-byte slots
constexpr int kOct = kRows * kSlab / 8 / kT;     // 4 octets of a slab per thread

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct alignas(16) TallLdsB {
  __bf16 xs[2][kRows * kPS];
  __bf16 f[kRows * kPF];    // relu(features.0)
  __bf16 h[kRows * kPH];    // relu(advantage.0) | relu(value.0)
  float adv[kRows * kPQ];
  float val[kRows];
  float q[kRows * kPQ];
};

// w[k .. k + 7] of a row of kw >= 1 floats, raw, for loads that must overlap what follows them: no
// branch and no select stands between the load and its use.  The address of an element at or past kw
// is clamped below kw, so nothing is read there; zero_past replaces such elements where the octet is
// converted.  VEC: the row is 16-byte aligned and kw a multiple of 4 (two 16-byte loads; else dwords).
template <bool VEC>
__device__ __forceinline__ f32x8 ld8_clamped(const float* w, int k, int kw) {
  f32x8 v;
  if constexpr (VEC) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(w + min(k, kw - 4));
    const f32x4 hi = *reinterpret_cast<const f32x4*>(w + min(k + 4, kw - 4));
    v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = w[min(k + i, kw - 1)];
  }
  return v;
}

__device__ __forceinline__ f32x8 zero_past(f32x8 v, int k, int kw) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = k + i < kw ? v[i] : 0.f;
  return v;
}

// the element type of the rows a RowPtr returns (const float* or const __bf16*)
template <class RowPtr>
using row_elem_t = typename std::remove_cv<
    typename std::remove_pointer<decltype((*static_cast<RowPtr*>(nullptr))(0))>::type>::type;

// elements per global load that rows of ld elements starting at x allow (Slab's XW)
__device__ __forceinline__ int x_width(const float* x, int ld) { return rows_aligned16(x, ld) ? 4 : 1; }
__device__ __forceinline__ int x_width(const __bf16* x, int ld) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(x);
  return (a & 15) == 0 && (ld & 7) == 0 ? 8 : (a & 7) == 0 && (ld & 3) == 0 ? 4 : 1;
}

// ---- a bf16 ring (VecAct / VecLearn / VecTallGrad::ring_bf16): the row already holds the operand bits
// x[k .. k + 7] of a bf16 row of kw >= 1 elements, raw, under ld8_clamped's rule.  W elements per load:
// 8 (one 16-byte load: the row is 16-byte aligned and kw % 8 == 0), 4 (two 8-byte loads: 8-byte aligned,
// kw % 4 == 0) or 1 (2-byte loads).  kw % W == 0, so a load lies wholly below kw or is clamped below it.
template <int W>
__device__ __forceinline__ bf16x8 ld8b_clamped(const __bf16* x, int k, int kw) {
  bf16x8 v;
  if constexpr (W == 8) {
    v = *reinterpret_cast<const bf16x8*>(x + min(k, kw - 8));
  } else if constexpr (W == 4) {
    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(x + min(k, kw - 4));
    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(x + min(k + 4, kw - 4));
    v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = x[min(k + i, kw - 1)];
  }
  return v;
}

// zero_past on the raw 16-bit lanes: dword j of the octet holds elements 2 j (low half) and 2 j + 1.  One
// compare per load of W elements (kw % W == 0); no conversion.
template <int W>
__device__ __forceinline__ bf16x8 zero_past_b(bf16x8 v, int k, int kw) {
  u32x4 d = __builtin_bit_cast(u32x4, v);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (W == 1) d[j] &= (k + 2 * j < kw ? 0xffffu : 0u) | (k + 2 * j + 1 < kw ? 0xffff0000u : 0u);
    else d[j] = k + (2 * j) / W * W < kw ? d[j] : 0u;
  }
  return __builtin_bit_cast(bf16x8, d);
}

// How a slab's octets are loaded, held in flight and written to LDS.  XW: elements of x per global load.
//   fp32 ring (and the staging block): XW = 4 (two 16-byte loads per octet) or 1 (dwords); 8 raw registers
//     per octet, rounded where the octet is stored.
//   bf16 ring: XW = 8 / 4 / 1 (ld8b_clamped); 4 raw registers per octet -- one 16-byte load per octet at
//     XW = 8, half the loads and half the registers of the fp32 ring -- and the LDS write stores the loaded
//     bits (zeroed at and past obs): no convert on this path.
template <class XT, int XW>
struct Slab;
template <int XW>
struct Slab<float, XW> {
  typedef f32x8 Raw;
  static __device__ __forceinline__ Raw load(const float* x, int k, int obs) { return ld8_clamped<XW == 4>(x, k, obs); }
  static __device__ __forceinline__ bf16x8 image(Raw v, int k, int obs) { return pack8(zero_past(v, k, obs)); }
};
template <int XW>
struct Slab<__bf16, XW> {
  typedef bf16x8 Raw;
  static __device__ __forceinline__ Raw load(const __bf16* x, int k, int obs) { return ld8b_clamped<XW>(x, k, obs); }
  static __device__ __forceinline__ bf16x8 image(Raw v, int k, int obs) { return zero_past_b<XW>(v, k, obs); }
};

// octet o of thread t in a slab: row (t + 256 o) / 32, slab columns 8 ((t + 256 o) % 32) .. + 7
template <class S, class RowPtr>
__device__ __forceinline__ void slab_load(typename S::Raw (&pre)[kOct], RowPtr rowp, int c0, int obs) {
#pragma unroll
  for (int o = 0; o < kOct; ++o) {
    const int i = threadIdx.x + kT * o;
    pre[o] = S::load(rowp(i >> 5), c0 + 8 * (i & 31), obs);
  }
}

// the slab at column c0, all 256 columns, as bf16; zero at and past obs
template <class S>
__device__ __forceinline__ void slab_store(__bf16* xs, const typename S::Raw (&pre)[kOct], int c0, int obs) {
#pragma unroll
  for (int o = 0; o < kOct; ++o) {
    const int i = threadIdx.x + kT * o;
    *reinterpret_cast<bf16x8*>(xs + (i >> 5) * kPS + 8 * (i & 31)) = S::image(pre[o], c0 + 8 * (i & 31), obs);
  }
}

// the raw fp32 weights of the round at column k (a multiple of 16) of the NT nets' rows wrow[t]: step
// group j, this half-wave's W0[n][k + 16 j + 8 hf .. + 7] (ld8_clamped)
template <int NT, int R, bool VEC>
__device__ __forceinline__ void load_w(f32x8 (&b)[NT][R], const float* const (&wrow)[NT], int k, int obs, int hf) {
#pragma unroll
  for (int j = 0; j < R; ++j)
#pragma unroll
    for (int t = 0; t < NT; ++t) b[t][j] = ld8_clamped<VEC>(wrow[t], k + 16 * j + 8 * hf, obs);
}

// acc[t] += xs[32][k0 .. k0 + 16 R) . (the round's weights, loaded at column kg)^T.  A weight at or
// past obs is a zero operand (the selects run in the round that straddles obs only: wave-uniform); the
// slab is zero there too.
template <int NT, int R>
__device__ __forceinline__ void round_mfma(f32x16 (&acc)[NT], const __bf16* arow, int k0, const f32x8 (&b)[NT][R],
                                           int kg, int obs, int hf) {
  bf16x8 a[R];
#pragma unroll
  for (int j = 0; j < R; ++j) a[j] = *reinterpret_cast<const bf16x8*>(arow + k0 + 16 * j);
  if (kg + 16 * R <= obs) {
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma16(a[j], pack8(b[t][j]), acc[t]);
  } else {
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = mfma16(a[j], pack8(zero_past(b[t][j], kg + 16 * j + 8 * hf, obs)), acc[t]);
  }
}

// fout[t] [32][kPF] = to_bf16(relu(x . W0_t^T + b0_t)) for the NT nets, x row r = rowp(r)[0 .. obs), fp32 or
// bf16 (the ring's element type).  VEC: every row of the nets' W0 is 16-byte aligned and obs % 4 == 0; XW: what
// the rows of x allow (Slab).  Called after a workgroup barrier (nothing reads xs or fout any more); the
// caller's next barrier completes fout.
template <int NT, bool VEC, int XW, class RowPtr>
__device__ __forceinline__ void tall_features_v(const VecNet* const (&net)[NT], __bf16* const (&fout)[NT],
                                                __bf16 (&xs)[2][kRows * kPS], RowPtr rowp) {
  typedef Slab<row_elem_t<RowPtr>, XW> SL;
  constexpr int R = NT == 1 ? 4 : 2;   // step groups of a round: NT R 8 raw registers, twice
  static_assert(kSlab % (32 * R) == 0, "a slab is a whole number of round pairs");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5;
  const int col = wave * 32 + (lane & 31);
  const int obs = net[0]->obs, S = (obs + kSlab - 1) / kSlab;
  f32x16 acc[NT] = {};
  const float* wrow[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) wrow[t] = net[t]->w0 + (size_t)col * obs;
  const float* const (&wr)[NT] = wrow;
  f32x8 wa[NT][R], wb[NT][R];   // the raw weights of the even / odd rounds
  typename SL::Raw pre[kOct];   // one slab of x in flight (fp32 ring 32 registers, bf16 ring 16)
  load_w<NT, R, VEC>(wa, wr, 0, obs, hf);
  slab_load<SL>(pre, rowp, 0, obs);
  slab_store<SL>(xs[0], pre, 0, obs);
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    const int c0 = s * kSlab, kw = min(kSlab, obs - c0);   // the slab holds kw columns, zeros after them
    if (s + 1 < S) slab_load<SL>(pre, rowp, c0 + kSlab, obs);   // in flight behind this slab's MFMAs
    const __bf16* arow = xs[s & 1] + (lane & 31) * kPS + 8 * hf;
    for (int k0 = 0; k0 < kw; k0 += 32 * R) {   // two rounds; the next round's loads lead by a round
      const int kg = c0 + k0;
      load_w<NT, R, VEC>(wb, wr, kg + 16 * R, obs, hf);
      round_mfma<NT, R>(acc, arow, k0, wa, kg, obs, hf);
      load_w<NT, R, VEC>(wa, wr, kg + 32 * R, obs, hf);   // (the next slab's first round too)
      if (k0 + 16 * R < kw) round_mfma<NT, R>(acc, arow, k0 + 16 * R, wb, kg + 16 * R, obs, hf);
    }
    if (s + 1 < S) slab_store<SL>(xs[(s + 1) & 1], pre, c0 + kSlab, obs);   // (last read before the previous barrier)
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float b = net[t]->b0[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) fout[t][acc_row(i, hf) * kPF + col] = to_bf16(fmaxf(acc[t][i] + b, 0.f));
  }
}

// xw: what every row of x allows (x_width).  An fp32 x takes 16-byte loads only together with W0 (as
// before the bf16 ring); a bf16 x takes its 16- or 8-byte loads whenever W0 takes its own.
template <int NT, class RowPtr>
__device__ __forceinline__ void tall_features_b(const VecNet* const (&net)[NT], __bf16* const (&fout)[NT],
                                                __bf16 (&xs)[2][kRows * kPS], RowPtr rowp, int xw) {
  bool vec = xw >= 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) vec = vec && rows_aligned16(net[t]->w0, net[t]->obs);
  if constexpr (std::is_same<row_elem_t<RowPtr>, __bf16>::value) {   // (every branch workgroup-uniform)
    if (vec && xw == 8) tall_features_v<NT, true, 8>(net, fout, xs, rowp);
    else if (vec) tall_features_v<NT, true, 4>(net, fout, xs, rowp);
    else tall_features_v<NT, false, 1>(net, fout, xs, rowp);
  } else {
    if (vec) tall_features_v<NT, true, 4>(net, fout, xs, rowp);
    else tall_features_v<NT, false, 1>(net, fout, xs, rowp);
  }
}

// Q of the 32 rows rowp(0 .. 31) -> L.f, L.h, L.q.  Called after a barrier, ends with one.
template <class RowPtr>
__device__ __forceinline__ void tall_forward_b(const VecNet& n, TallLdsB& L, RowPtr rowp, int xw) {
  const VecNet* const net[1] = {&n};
  __bf16* const fout[1] = {L.f};
  tall_features_b<1>(net, fout, L.xs, rowp, xw);
  heads_b(n, L.f, L.h, L.adv, L.val, L.q);
}

// The ring of a handle as its element type XT: float, or __bf16 where the handle says ring_bf16 (the
// launchers pick the instantiation; the pointer is typed const float* in the handles either way).
template <class XT>
__device__ __forceinline__ const XT* ring_as(const float* ring) { return reinterpret_cast<const XT*>(ring); }

// ------------------------------------------------------------------ acting
template <class XT>
__global__ __launch_bounds__(kT) void vectb_act_k(VecAct a) {
  __shared__ TallLdsB L;
  __shared__ int rid[kRows];
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows, obs = a.net.obs;
  if (t < kRows) rid[t] = a.hist[min(e0 + t, a.E - 1) * 4 + 3];   // rows past E repeat the last env
  __syncthreads();
  const XT* ring = ring_as<XT>(a.ring);
  tall_forward_b(a.net, L, [&](int r) { return ring + (size_t)rid[r] * obs; }, x_width(ring, obs));
  const int e = e0 + t;
  if (t < kRows && e < a.E)
    draw(L.q + t * kPQ, e, a.net.A, a.eps[e], a.seed, a.counter ? (uint64_t)a.counter[0] : 0ull, a.q, a.actions);
}

// vectb_act_k over the staging block's reset_obs rows (rows N + e0 .. of [2 N][obs]; a padding row
// repeats the workgroup's last live row), the step k by value, epsilon 0.
__global__ __launch_bounds__(kT) void vectb_host_eval_act_k(VecHostEvalAct a) {
  __shared__ TallLdsB L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows, obs = a.net.obs;
  const int live = min(kRows, a.N - e0);   // >= 1: the grid is ceil(N / 32)
  const float* src = a.stage + (size_t)(a.N + e0) * obs;
  tall_forward_b(a.net, L, [&](int r) { return src + (size_t)min(r, live - 1) * obs; },
                 x_width(a.stage, obs));
  if (t < live) draw(L.q + t * kPQ, e0 + t, a.net.A, 0.f, a.seed, (uint64_t)a.k, a.q, a.actions);
}

// ------------------------------------------------------------------ learner
template <class XT>
__global__ __launch_bounds__(kT) void vectb_learn_k(VecLearn p) {
  __shared__ TallLdsB L;
  __shared__ float qt[kRows * kPQ];                   // target net on s'
  __shared__ float q2[kRows * kPQ];                   // online net on s'
  __shared__ float dAf[kRows * kPAf];                 // dL/dA [0, 32) | dL/dV, fp32 (to memory)
  __shared__ __align__(16) __bf16 dA[kRows * kPA];    // dL/dA rounded, zero in [A, 32)
  __shared__ __align__(16) __bf16 dh[kRows * kPH];    // online features of s' first, then d(hidden), rounded
  __shared__ int sid[kRows], sid2[kRows];
  const int t = threadIdx.x;
  const int b0 = blockIdx.x * kRows;
  const int obs = p.on.obs;
  const XT* ring = ring_as<XT>(p.ring);
  const int xw = x_width(ring, obs);
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
  {  // s' once: the target's features into L.f, the online net's into the dh image
    const VecNet* const net[2] = {&p.tg, &p.on};
    __bf16* const fout[2] = {L.f, dh};
    tall_features_b<2>(net, fout, L.xs, [&](int r) { return ring + (size_t)sid2[r] * obs; }, xw);
  }
  heads_b(p.tg, L.f, L.h, L.adv, L.val, L.q);
  for (int i = t; i < kRows * kPQ; i += kT) qt[i] = L.q[i];
  heads_b(p.on, dh, L.h, L.adv, L.val, L.q);
  for (int i = t; i < kRows * kPQ; i += kT) q2[i] = L.q[i];
  // online(s) last: its f / h stay for the backward
  tall_forward_b(p.on, L, [&](int r) { return ring + (size_t)sid[r] * obs; }, xw);
  loss_backward_b(p, b0, L.f, L.h, L.q, qt, q2, dAf, dA, dh);
}

// ------------------------------------------------------------------ batch contraction
// A dW0 tile over a bf16 ring: acc += dF^T . x over the batch rows [bs, be) of one wave, lane r's column of dF
// at pg, of x at px (ring + column), batch row bb at ring row sid[bb].  The loop of vectb_grad_k below with the
// right operand gathered by 2-byte loads straight into the MFMA operand: the bits the forward consumed, no
// rounding at pack time.
__device__ __forceinline__ void grad_ring_b(f32x16& acc, float& bsum, const float* pg, const __bf16* px, const int* sid,
                                            int obs, bool mok, bool nok, int bs, int be, int hf) {
  for (int b = bs; b < be; b += 16 * kGradSteps) {
    f32x8 av[kGradSteps];
    bf16x8 xv[kGradSteps];
#pragma unroll
    for (int u = 0; u < kGradSteps; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int bb = b + 16 * u + 8 * hf + i;
        const bool in = bb < be;  // the tail is zero operands: nothing is read past the range
        av[u][i] = in && mok ? pg[(size_t)bb * vecw::STRIDE] : 0.f;
        xv[u][i] = in && nok ? px[(size_t)sid[bb] * obs] : static_cast<__bf16>(0.f);
      }
#pragma unroll
    for (int u = 0; u < kGradSteps; ++u) {
      if (b + 16 * u < be) acc = mfma16(pack8(av[u]), xv[u], acc);  // (wave-uniform)
#pragma unroll
      for (int i = 0; i < 8; ++i) bsum += av[u][i];
    }
  }
}

template <class XT>
__global__ __launch_bounds__(kT) void vectb_grad_k(VecTallGrad G) {
  __shared__ GradRed R;
  __shared__ int sid[1024];   // frame ids of the batch's observations (the dW0 tiles only)
  const VecGrad& g = G.g;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const GradTile T = grad_tile(blockIdx.x, g.obs, g.A);
  const bool w0 = blockIdx.x < 4 * ((g.obs + 31) / 32);   // (workgroup-uniform) a tile of dW0: x from the ring
  if (w0) {
    for (int i = t; i < g.B; i += kT) sid[i] = G.s_ids[G.idx[i] * 4 + 3];
    __syncthreads();
  }
  const int chunk = grad_chunk(g.B);
  const int bs = wave * chunk, be = min(g.B, bs + chunk);
  const bool mok = T.m0 + r < T.rows, nok = T.n0 + r < T.cols;
  const float* pg = g.vec + T.goff + T.m0 + r;
  f32x16 acc = {};
  float bsum = 0.f;
  if (std::is_same<XT, __bf16>::value && w0) {
    grad_ring_b(acc, bsum, pg, ring_as<__bf16>(G.ring) + T.n0 + r, sid, g.obs, mok, nok, bs, be, hf);
  } else {   // (the fp32 ring's dW0 tiles and, over either ring, the nine tensors contracted against the rows)
    const float* px = w0 ? G.ring + T.n0 + r : g.vec + T.xoff + T.n0 + r;
    for (int b = bs; b < be; b += 16 * kGradSteps) {
      f32x8 av[kGradSteps], xv[kGradSteps];
#pragma unroll
      for (int u = 0; u < kGradSteps; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int bb = b + 16 * u + 8 * hf + i;
          const bool in = bb < be;  // the tail is zero operands: nothing is read past the range
          av[u][i] = in && mok ? pg[(size_t)bb * vecw::STRIDE] : 0.f;
          xv[u][i] = in && nok ? px[w0 ? (size_t)sid[bb] * g.obs : (size_t)bb * vecw::STRIDE] : 0.f;
        }
#pragma unroll
      for (int u = 0; u < kGradSteps; ++u) {
        if (b + 16 * u < be) acc = mfma16(pack8(av[u]), pack8(xv[u]), acc);  // (wave-uniform)
#pragma unroll
        for (int i = 0; i < 8; ++i) bsum += av[u][i];
      }
    }
  }
  grad_finish(R, acc, bsum, T, g.grad, g.part);
}

void check_tall_net(const VecNet& n, const char* who) {
  if (n.obs < 1 || n.obs > kVecTallMaxObs || n.A < 1 || n.A > kVecWideMaxA)
    throw std::invalid_argument(std::string(who) + ": obs in [1, 1024] and actions in [1, 32]");
  if (n.atoms != 0) throw std::invalid_argument(std::string(who) + ": categorical heads (atoms != 0) are vecd_*'s");
  if (!n.w0 || !n.b0 || !n.wa1 || !n.ba1 || !n.wa2 || !n.ba2 || !n.wv1 || !n.bv1 || !n.wv2 || !n.bv2)
    throw std::invalid_argument(std::string(who) + ": missing parameter tensor");
}

}  // namespace

// ------------------------------------------------------------------ launchers
void vectb_act(const VecAct& a, hipStream_t s) {
  check_tall_net(a.net, "vectb_act");
  if (a.E < 1 || a.E > 4096 || !a.ring || !a.hist || !a.eps || !a.q || !a.actions)
    throw std::invalid_argument("vectb_act: 1 <= E <= 4096 with ring, hist, eps, q and actions");
  (a.ring_bf16 ? vectb_act_k<__bf16> : vectb_act_k<float>)<<<(a.E + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vectb_host_eval_act(const VecHostEvalAct& a, hipStream_t s) {
  check_tall_net(a.net, "vectb_host_eval_act");
  if (a.N < 1 || a.N > 64) throw std::invalid_argument("vectb_host_eval_act: 1 <= N <= 64 evaluator envs");
  if (a.k < 0) throw std::invalid_argument("vectb_host_eval_act: step k >= 0");
  if (!a.stage) throw std::invalid_argument("vectb_host_eval_act: the staging block's device copy");
  if (!a.q || !a.actions) throw std::invalid_argument("vectb_host_eval_act: q and actions");
  vectb_host_eval_act_k<<<(a.N + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vectb_learn(const VecLearn& p, hipStream_t s) {
  check_tall_net(p.on, "vectb_learn (online)");
  check_tall_net(p.tg, "vectb_learn (target)");
  if (p.on.obs != p.tg.obs || p.on.A != p.tg.A) throw std::invalid_argument("vectb_learn: nets differ in shape");
  if (p.B < 1 || p.B > 1024) throw std::invalid_argument("vectb_learn: batch must be in [1, 1024]");
  if (!p.ring || !p.s_ids || !p.s2_ids || !p.act || !p.rew || !p.done || !p.idx || !p.w || !p.q_s || !p.q_s2 ||
      !p.qt_s2 || !p.vec || !p.delta || !p.lw)
    throw std::invalid_argument("vectb_learn: missing buffer");
  if (p.beta_out && !(p.beta_horizon > 0.0)) throw std::invalid_argument("vectb_learn: beta horizon must be > 0");
  (p.ring_bf16 ? vectb_learn_k<__bf16> : vectb_learn_k<float>)<<<(p.B + kRows - 1) / kRows, kT, 0, s>>>(p);
  LAUNCH_CHECK();
}

void vectb_grad(const VecTallGrad& G, hipStream_t s) {
  const VecGrad& g = G.g;
  if (g.obs < 1 || g.obs > kVecTallMaxObs || g.A < 1 || g.A > kVecWideMaxA || g.n != vec_param_count(g.obs, g.A))
    throw std::invalid_argument("vectb_grad: n must be the MLP dueling net's parameter count");
  if (g.B < 1 || g.B > 1024 || !g.vec || !g.grad || !g.part || !G.ring || !G.s_ids || !G.idx)
    throw std::invalid_argument("vectb_grad: batch in [1, 1024] with vec, grad, part, ring, s_ids and idx");
  (G.ring_bf16 ? vectb_grad_k<__bf16> : vectb_grad_k<float>)<<<vect_grad_blocks(g.obs, g.A), kT, 0, s>>>(G);
  LAUNCH_CHECK();
}

}  // namespace apex
