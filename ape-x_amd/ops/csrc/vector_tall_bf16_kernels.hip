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
// LDS per workgroup (static): slabs 33,792 + f 8,704 + h 16,896 + adv / val / q 8,576 = 67,968 B, + 128 B
// of row ids: vectb_act 68,096 B (vectb_host_eval_act 67,968 B).  vectb_learn adds qt / q2 8,448,
// dA fp32 4,224, dA bf16 2,560, dh 16,896 and 256 B of ids: 100,352 B of gfx950's 163,840.  vectb_grad:
// 16,928 B of reduction images + 4,096 B of ids.
#include "vector_wide_bf16_common.h"

namespace apex {

namespace {

using namespace widebf16;

constexpr int kSlab = 256;                       // columns of x per slab
constexpr int kPS = kSlab + 8;                   // 264 bf16 = 33 16-byte slots
constexpr int kOct = kRows * kSlab / 8 / kT;     // 4 octets of a slab per thread

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

// octet o of thread t in a slab: row (t + 256 o) / 32, slab columns 8 ((t + 256 o) % 32) .. + 7
template <bool VEC, class RowPtr>
__device__ __forceinline__ void slab_load(f32x8 (&pre)[kOct], RowPtr rowp, int c0, int obs) {
#pragma unroll
  for (int o = 0; o < kOct; ++o) {
    const int i = threadIdx.x + kT * o;
    pre[o] = ld8_clamped<VEC>(rowp(i >> 5), c0 + 8 * (i & 31), obs);
  }
}

// the slab at column c0, all 256 columns, rounded; zero at and past obs
__device__ __forceinline__ void slab_store(__bf16* xs, const f32x8 (&pre)[kOct], int c0, int obs) {
#pragma unroll
  for (int o = 0; o < kOct; ++o) {
    const int i = threadIdx.x + kT * o;
    *reinterpret_cast<bf16x8*>(xs + (i >> 5) * kPS + 8 * (i & 31)) = pack8(zero_past(pre[o], c0 + 8 * (i & 31), obs));
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

// fout[t] [32][kPF] = to_bf16(relu(x . W0_t^T + b0_t)) for the NT nets, x row r = rowp(r)[0 .. obs).
// VEC: every row of x and of the nets' W0 is 16-byte aligned and obs % 4 == 0.  Called after a workgroup
// barrier (nothing reads xs or fout any more); the caller's next barrier completes fout.
template <int NT, bool VEC, class RowPtr>
__device__ __forceinline__ void tall_features_v(const VecNet* const (&net)[NT], __bf16* const (&fout)[NT],
                                                __bf16 (&xs)[2][kRows * kPS], RowPtr rowp) {
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
  f32x8 pre[kOct];
  load_w<NT, R, VEC>(wa, wr, 0, obs, hf);
  slab_load<VEC>(pre, rowp, 0, obs);
  slab_store(xs[0], pre, 0, obs);
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    const int c0 = s * kSlab, kw = min(kSlab, obs - c0);   // the slab holds kw columns, zeros after them
    if (s + 1 < S) slab_load<VEC>(pre, rowp, c0 + kSlab, obs);   // in flight behind this slab's MFMAs
    const __bf16* arow = xs[s & 1] + (lane & 31) * kPS + 8 * hf;
    for (int k0 = 0; k0 < kw; k0 += 32 * R) {   // two rounds; the next round's loads lead by a round
      const int kg = c0 + k0;
      load_w<NT, R, VEC>(wb, wr, kg + 16 * R, obs, hf);
      round_mfma<NT, R>(acc, arow, k0, wa, kg, obs, hf);
      load_w<NT, R, VEC>(wa, wr, kg + 32 * R, obs, hf);   // (the next slab's first round too)
      if (k0 + 16 * R < kw) round_mfma<NT, R>(acc, arow, k0 + 16 * R, wb, kg + 16 * R, obs, hf);
    }
    if (s + 1 < S) slab_store(xs[(s + 1) & 1], pre, c0 + kSlab, obs);   // (last read before the previous barrier)
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float b = net[t]->b0[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) fout[t][acc_row(i, hf) * kPF + col] = to_bf16(fmaxf(acc[t][i] + b, 0.f));
  }
}

// xvec: every row of x is 16-byte aligned (and obs % 4 == 0)
template <int NT, class RowPtr>
__device__ __forceinline__ void tall_features_b(const VecNet* const (&net)[NT], __bf16* const (&fout)[NT],
                                                __bf16 (&xs)[2][kRows * kPS], RowPtr rowp, bool xvec) {
  bool vec = xvec;
#pragma unroll
  for (int t = 0; t < NT; ++t) vec = vec && rows_aligned16(net[t]->w0, net[t]->obs);
  if (vec) tall_features_v<NT, true>(net, fout, xs, rowp);   // (workgroup-uniform)
  else tall_features_v<NT, false>(net, fout, xs, rowp);
}

// Q of the 32 rows rowp(0 .. 31) -> L.f, L.h, L.q.  Called after a barrier, ends with one.
template <class RowPtr>
__device__ __forceinline__ void tall_forward_b(const VecNet& n, TallLdsB& L, RowPtr rowp, bool xvec) {
  const VecNet* const net[1] = {&n};
  __bf16* const fout[1] = {L.f};
  tall_features_b<1>(net, fout, L.xs, rowp, xvec);
  heads_b(n, L.f, L.h, L.adv, L.val, L.q);
}

// ------------------------------------------------------------------ acting
__global__ __launch_bounds__(kT) void vectb_act_k(VecAct a) {
  __shared__ TallLdsB L;
  __shared__ int rid[kRows];
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows, obs = a.net.obs;
  if (t < kRows) rid[t] = a.hist[min(e0 + t, a.E - 1) * 4 + 3];   // rows past E repeat the last env
  __syncthreads();
  tall_forward_b(a.net, L, [&](int r) { return a.ring + (size_t)rid[r] * obs; }, rows_aligned16(a.ring, obs));
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
                 rows_aligned16(a.stage, obs));
  if (t < live) draw(L.q + t * kPQ, e0 + t, a.net.A, 0.f, a.seed, (uint64_t)a.k, a.q, a.actions);
}

// ------------------------------------------------------------------ learner
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
  const bool xvec = rows_aligned16(p.ring, obs);
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
    tall_features_b<2>(net, fout, L.xs, [&](int r) { return p.ring + (size_t)sid2[r] * obs; }, xvec);
  }
  heads_b(p.tg, L.f, L.h, L.adv, L.val, L.q);
  for (int i = t; i < kRows * kPQ; i += kT) qt[i] = L.q[i];
  heads_b(p.on, dh, L.h, L.adv, L.val, L.q);
  for (int i = t; i < kRows * kPQ; i += kT) q2[i] = L.q[i];
  // online(s) last: its f / h stay for the backward
  tall_forward_b(p.on, L, [&](int r) { return p.ring + (size_t)sid[r] * obs; }, xvec);
  loss_backward_b(p, b0, L.f, L.h, L.q, qt, q2, dAf, dA, dh);
}

// ------------------------------------------------------------------ batch contraction
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
  const float* px = w0 ? G.ring + T.n0 + r : g.vec + T.xoff + T.n0 + r;
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
        xv[u][i] = in && nok ? px[w0 ? (size_t)sid[bb] * g.obs : (size_t)bb * vecw::STRIDE] : 0.f;
      }
#pragma unroll
    for (int u = 0; u < kGradSteps; ++u) {
      if (b + 16 * u < be) acc = mfma16(pack8(av[u]), pack8(xv[u]), acc);  // (wave-uniform)
#pragma unroll
      for (int i = 0; i < 8; ++i) bsum += av[u][i];
    }
  }
  grad_finish(R, acc, bsum, T, g.grad, g.part);
}

void check_tall_net(const VecNet& n, const char* who) {
  if (n.obs < 1 || n.obs > kVecTallMaxObs || n.A < 1 || n.A > kVecWideMaxA)
    throw std::invalid_argument(std::string(who) + ": obs in [1, 1024] and actions in [1, 32]");
  if (!n.w0 || !n.b0 || !n.wa1 || !n.ba1 || !n.wa2 || !n.ba2 || !n.wv1 || !n.bv1 || !n.wv2 || !n.bv2)
    throw std::invalid_argument(std::string(who) + ": missing parameter tensor");
}

}  // namespace

// ------------------------------------------------------------------ launchers
void vectb_act(const VecAct& a, hipStream_t s) {
  check_tall_net(a.net, "vectb_act");
  if (a.E < 1 || a.E > 4096 || !a.ring || !a.hist || !a.eps || !a.q || !a.actions)
    throw std::invalid_argument("vectb_act: 1 <= E <= 4096 with ring, hist, eps, q and actions");
  vectb_act_k<<<(a.E + kRows - 1) / kRows, kT, 0, s>>>(a);
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
  vectb_learn_k<<<(p.B + kRows - 1) / kRows, kT, 0, s>>>(p);
  LAUNCH_CHECK();
}

void vectb_grad(const VecTallGrad& G, hipStream_t s) {
  const VecGrad& g = G.g;
  if (g.obs < 1 || g.obs > kVecTallMaxObs || g.A < 1 || g.A > kVecWideMaxA || g.n != vec_param_count(g.obs, g.A))
    throw std::invalid_argument("vectb_grad: n must be the MLP dueling net's parameter count");
  if (g.B < 1 || g.B > 1024 || !g.vec || !g.grad || !g.part || !G.ring || !G.s_ids || !G.idx)
    throw std::invalid_argument("vectb_grad: batch in [1, 1024] with vec, grad, part, ring, s_ids and idx");
  vectb_grad_k<<<vect_grad_blocks(g.obs, g.A), kT, 0, s>>>(G);
  LAUNCH_CHECK();
}

}  // namespace apex
