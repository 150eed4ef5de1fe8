// The one-sample fp32 Nature-CNN dueling forward inside ONE 1024-thread workgroup (gfx950), shared
// by atari_rollout_k (atari_rollout_kernels.hip) and host_eval_act_k (host_eval_kernels.hip).
//
// Where the data lives (LDS, 160 KiB per CU, one workgroup per CU; the kernel declares the arrays):
//   fr   4 x 7,056 B   the env's 4-frame stack as a 4-slot ring (chan -> slot in `csp`)
//   w1b  48 KiB        conv1 weight, split once into hi / mid / lo bf16 planes [k / 8][n][k % 8]
//                      (one 16-B read per fragment and term): stage_w1()
//   a1   400 x 36 f32  conv1 output NHWC, pixel pitch 36 (16-B aligned, 2-way on conv2's reads);
//                      dead after conv2, so a3 [49][64] (FC1's k order p * 64 + c) reuses it
//   a2   81 x 68 f32   conv2 output, pitch 68 (conflict-free 16-B reads for conv3)
// Weights are read through L2 from the layouts that exist: features.0.weight, the forward
// arena's w2p / w3p / wfc1p (k-contiguous rows), head weights and biases from the master.  The
// weight struct W is any struct with the members w1, b1, w2p, b2, w3p, b3, wfc1p, ba1, bv1, wa2,
// ba2, wv2, bv2 (AtariRollout, HostEvalAct).
//
// conv1 runs on v_mfma_f32_32x32x16_bf16 with the project's exact three-term split: u8 pixels
// are exact in bf16 and a weight is hi + mid + lo exactly, so three products per 16 k, each exact
// in fp32.  conv2 / conv3 run on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate): a wave
// owns a 32 x 32 output tile (M padded to the tile: padded rows read a clamped pixel and are never
// stored) over one k-part; a lane fetches 16 B of A and of B per 8 k and issues 4 MFMAs, lane half
// h supplying k = 8c + 4h + j to MFMA j for both operands.  conv2 splits K over 2 and conv3 over 4
// wave groups that add their tiles into LDS in a fixed order (barrier-separated phases), so the
// result is deterministic.  FC1 is a 256 x 3136 GEMV on the VALU: wave w owns rows 16w .. 16w + 15,
// per k half a lane holds its 7 (then 6) 16-B pieces of a3 in registers and reads each weight row as coalesced 16-B
// loads; the lanes' partial sums meet in wave_sum's fixed butterfly, the two k halves in LDS.
#pragma once

#include "common.h"
#include "kernels.h"

namespace apex {
namespace atari_fwd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bfx8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t pack_bf16_hi(float lo, float hi) {  // two exact bf16 halves
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
__device__ __forceinline__ float trunc_bf16(float x) { return __uint_as_float(__float_as_uint(x) & 0xFFFF0000u); }

constexpr int kT = 1024, kWaves = kT / 64;
constexpr int kFrameDw = 84 * 84 / 4;            // 1764 words of one 84 x 84 u8 frame
constexpr int kP1 = 36, kP2 = 68, kP3 = 64;      // LDS pixel pitches of a1 / a2 / a3 (floats)
constexpr int kA1Floats = 400 * kP1, kA2Floats = 81 * kP2;

// The weights do not change during a launch, so the compiler would hoist their loads out of a
// step loop (and spill them): every step's weight offsets go through this.
__device__ __forceinline__ int opaque_i(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// C/D fragment of the 32x32 MFMA: register i of lane l is row (i & 3) + 8 (i >> 2) + 4 (l >> 5),
// column l & 31.  `phase` of `phases` k-parts: 0 stores, the others add; the last adds bias + ReLU.
template <int M, int POUT>
__device__ __forceinline__ void tile_store(float* out, const f32x16& acc, int mt, int n, int kh, float bias,
                                           bool first, bool last) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh;
    if (m < M) {
      float v = acc[i];
      float* o = out + m * POUT + n;
      if (!first) v += *o;
      if (last) v = fmaxf(v + bias, 0.f);
      *o = v;
    }
  }
}

// conv2 / conv3 from an NHWC fp32 LDS image: out[m = oy * OUTW + ox][n] over k = (ky, kx, c).
// Called by every thread (it holds KPARTS barriers); unit = wave index.
template <int CIN, int KW, int STRIDE, int INW, int OUTW, int M, int PIN, int POUT, int KPARTS>
__device__ __forceinline__ void conv_lds(const float* in, float* out, const float* __restrict__ w,
                                         const float* __restrict__ bias, int unit, int lane) {
  constexpr int K = KW * KW * CIN, MT = (M + 31) / 32, NT = 2, CP = K / 8 / KPARTS;
  static_assert(CP * 8 * KPARTS == K && CP % 2 == 0 && CIN % 8 == 0 && MT * NT * KPARTS <= kWaves, "conv tiling");
  const bool valid = unit < MT * NT * KPARTS;
  const int kpart = unit / (MT * NT), tile = unit % (MT * NT), mt = tile % MT, nt = tile / MT;
  const int r = lane & 31, kh = lane >> 5, n = nt * 32 + r;
  f32x16 acc = {};
  if (valid) {
    const int m = min(mt * 32 + r, M - 1), oy = m / OUTW, ox = m % OUTW;
    const float* arow = in + ((STRIDE * oy) * INW + STRIDE * ox) * PIN + kh * 4;
    const float* brow = w + opaque_i(n * K + kh * 4);
    auto load = [&](int ch, f32x4& a, f32x4& b) {
      const int k0 = ch * 8, tap = k0 / CIN, c0 = k0 % CIN, ky = tap / KW, kx = tap % KW;
      a = *reinterpret_cast<const f32x4*>(arow + (ky * INW + kx) * PIN + c0);
      b = *reinterpret_cast<const f32x4*>(brow + k0);
    };
    // two chunks per iteration, the next two in flight under the 8 MFMAs (the last iteration
    // re-reads its own chunks instead of branching)
    const int c0 = kpart * CP, c1 = c0 + CP;
    f32x4 a0, b0, a1, b1;
    load(c0, a0, b0);
    load(c0 + 1, a1, b1);
#pragma unroll 1
    for (int ch = c0; ch < c1; ch += 2) {
      const int nx = min(ch + 2, c1 - 2);
      f32x4 na0, nb0, na1, nb1;
      load(nx, na0, nb0);
      load(nx + 1, na1, nb1);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc, 0, 0, 0);
      a0 = na0; b0 = nb0; a1 = na1; b1 = nb1;
    }
  }
  const float bv = valid ? bias[n] : 0.f;
#pragma unroll
  for (int ph = 0; ph < KPARTS; ++ph) {
    if (valid && kpart == ph) tile_store<M, POUT>(out, acc, mt, n, kh, bv, ph == 0, ph == KPARTS - 1);
    __syncthreads();
  }
}

// conv1 weight (32, 4, 8, 8) -> the three bf16 planes: w = hi + mid + lo exactly (truncation:
// 8 + 8 + 8 bits).  Every thread calls it; the caller's barrier publishes the planes.
__device__ __forceinline__ void stage_w1(const float* __restrict__ w1, uint16_t (*w1b)[256 * 32], int tid) {
  for (int i = tid; i < 32 * 256; i += kT) {
    const int n = i >> 8, k = i & 255, at = ((k >> 3) * 32 + n) * 8 + (k & 7);
    const float w = w1[i], hi = trunc_bf16(w), r = w - hi, mid = trunc_bf16(r);
    w1b[0][at] = (uint16_t)(__float_as_uint(hi) >> 16);
    w1b[1][at] = (uint16_t)(__float_as_uint(mid) >> 16);
    w1b[2][at] = (uint16_t)(__float_as_uint(r - mid) >> 16);
  }
}

// conv1 .. heads of the stack `fr` (channel c in LDS slot (csp >> 2c) & 3): leaves the A advantage
// outputs and the value in advs[0 .. A], published by the closing barrier.  Every thread calls it
// (a fixed number of workgroup-uniform barriers).  zs [512], hs [256], advs [32].
template <class W>
__device__ __forceinline__ void forward(const W& R, const uint32_t* fr, int csp, const uint16_t (*w1b)[256 * 32],
                                        float* a1, float* a2, float* zs, float* hs, float* advs, int A, int tid,
                                        int lane, int wave) {
  float* a3 = a1;
  // ---- conv1: M = 400 (13 tiles), N = 32, K = 256 = (c, ky, kx) on v_mfma_f32_32x32x16_bf16 with
  // the exact three-term weight split: u8 pixels are exact in bf16, every product is exact in
  // fp32, only the fp32 accumulation rounds.  A 16-k step is two pixel rows (lane half h: row
  // ky = (2s + h) & 7, its 8 kx) of channel s >> 2.
  if (wave < 13) {
    const int r = lane & 31, kh = lane >> 5;
    const int m = min(wave * 32 + r, 399), oy = m / 20, ox = m % 20;
    const uint32_t* arow = fr + (4 * oy) * 21 + ox;
    f32x16 acc = {};
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const int c = s >> 2, ky = (2 * s + kh) & 7;
      const uint32_t* px = arow + ((csp >> (2 * c)) & 3) * kFrameDw + ky * 21;
      const uint32_t p0 = px[0], p1 = px[1];
      float f[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f[j] = (float)((p0 >> (8 * j)) & 255u);
        f[4 + j] = (float)((p1 >> (8 * j)) & 255u);
      }
      const bfx8 a = __builtin_bit_cast(bfx8, make_uint4(pack_bf16_hi(f[0], f[1]), pack_bf16_hi(f[2], f[3]),
                                                          pack_bf16_hi(f[4], f[5]), pack_bf16_hi(f[6], f[7])));
      const int at = ((2 * s + kh) * 32 + r) * 8;
#pragma unroll
      for (int t = 2; t >= 0; --t)  // lo, mid, hi
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a, __builtin_bit_cast(bfx8, *reinterpret_cast<const uint4*>(&w1b[t][at])), acc, 0, 0, 0);
    }
    tile_store<400, kP1>(a1, acc, wave, r, kh, R.b1[r], true, true);
  }
  __syncthreads();
  // ---- conv2: 81 x 64 x 512 (2 k-parts); conv3: 49 x 64 x 576 (4 k-parts) into a3 (a1 is dead)
  conv_lds<32, 4, 2, 20, 9, 81, kP1, kP2, 2>(a1, a2, R.w2p, R.b2, wave, lane);
  conv_lds<64, 3, 1, 9, 7, 49, kP2, kP3, 4>(a2, a3, R.w3p, R.b3, wave, lane);
  // ---- FC1: h[n] = relu(sum_k a3[k] wfc1p[n][k] + b), k = p * 64 + c (3136 = 784 x 16 B)
  // (two k halves, so a lane holds 7 pieces of a3 beside the 7 loads in flight)
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    f32x4 x[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int q = lane + 64 * (7 * half + i);
      x[i] = q < 784 ? reinterpret_cast<const f32x4*>(a3)[q] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int j = 0; j < 16; ++j) {
      const int n = wave * 16 + j;
      const f32x4* wr = reinterpret_cast<const f32x4*>(R.wfc1p + opaque_i(n * 3136));
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        const int q = lane + 64 * (7 * half + i);
        if (q < 784) {
          const f32x4 wv = wr[q];
          s += x[i][0] * wv[0] + x[i][1] * wv[1] + x[i][2] * wv[2] + x[i][3] * wv[3];
        }
      }
      s = wave_sum(s);
      if (lane == 0) zs[half * 256 + n] = s;
    }
  }
  __syncthreads();
  if (tid < 256) hs[tid] = fmaxf(zs[tid] + zs[256 + tid] + (tid < 128 ? R.ba1[tid] : R.bv1[tid - 128]), 0.f);
  __syncthreads();
  // ---- heads: A advantage rows over h[0..127], the value row over h[128..255]
  for (int o = wave; o <= A; o += kWaves) {
    const float* wrow = (o < A ? R.wa2 + o * 128 : R.wv2) + opaque_i(0);
    const float* hh = hs + (o < A ? 0 : 128);
    float s = hh[2 * lane] * wrow[2 * lane] + hh[2 * lane + 1] * wrow[2 * lane + 1];
    s = wave_sum(s);
    if (lane == 0) advs[o] = s + (o < A ? R.ba2[o] : R.bv2[0]);
  }
  __syncthreads();
}

// One thread: the dueling combine of advs[0 .. A] into qs[0 .. A) and the action by select_actions_k's
// rule and draw -- first argmax; explore iff !(u0 > eps); then min(int(u1 A), A - 1); Philox key
// (act_seed, e, step).
__device__ __forceinline__ int combine_select(const float* advs, float* qs, int A, uint64_t act_seed, int e,
                                              int64_t step, float eps) {
  float mean = 0.f;
  for (int a = 0; a < A; ++a) mean += advs[a];
  mean /= (float)A;
  const float val = advs[A];
  int best = 0;
  float bvq = 0.f;
  for (int a = 0; a < A; ++a) {
    const float qv = val + (advs[a] - mean);
    qs[a] = qv;
    if (a == 0 || qv > bvq) { bvq = qv; best = a; }
  }
  float u[4];
  uniform4(act_seed, (uint64_t)e, (uint64_t)step, u);
  if (!(u[0] > eps)) {
    const int rr = (int)(u[1] * (float)A);
    best = rr < A ? rr : A - 1;
  }
  return best;
}

}  // namespace atari_fwd
}  // namespace apex
