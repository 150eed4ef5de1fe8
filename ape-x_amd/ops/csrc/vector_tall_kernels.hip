// Tall mode of the wide MLP dueling DQN on gfx950: obs <= 1024 (kVecTallMaxObs), A <= 32, hidden 128,
// batches to 1024.  The wide kernels (vector_wide_kernels.hip) keep a workgroup's whole 32-row
// observation tile in LDS and copy every sampled observation into its per-sample row; both stop at
// obs = 128.  Here features.0 -- with K = obs the largest GEMM of the step -- streams the observation,
// and its weight gradient reads the observation where it lies, in the replay's ring.
//
// Precision: native fp32 MFMA (v_mfma_f32_32x32x2_f32), exact fp32 products, fp32 accumulation in an
// order that depends on the shapes only; no atomics; bit-identical reruns.
//
//   tall_features (device) a workgroup of 4 waves owns 32 rows; wave w owns units 32w .. 32w + 31 of
//                 features.0 for NT nets at once (one f32x16 accumulator per net, alive across the
//                 whole observation).  x goes through LDS in slabs of 128 columns, double-buffered
//                 ([2][32][132], the wide x image's pitch of 33 16-byte slots).  A slab is 4 quads of 4
//                 floats per thread, a row's 128 floats on the 32 lanes of a half-wave: one 16-byte
//                 global load per quad when the rows are 16-byte aligned (obs % 4 == 0), four dword
//                 loads otherwise.  Slab s + 1's loads are issued before slab s's MFMAs and stored to
//                 the other buffer after them; one barrier per slab.  Inside a slab the operands are
//                 tile_nt's: a 16-byte LDS read and a 16-byte weight read (W[n][128 s + k .. + 3]) feed
//                 four MFMAs.  The last slab is zero beyond obs in LDS only and contracts
//                 ceil8(obs - 128 s) columns; neither x nor a weight is read past obs.
//   vect_act / vect_host_eval_act   vecw_act / vecw_host_eval_act on that forward: the rows are ring
//                 rows hist[e][3] / the staged reset_obs rows, the heads are wide_heads, the draw is
//                 vec_act's arithmetic.
//   vect_learn    one workgroup per 32 sampled rows.  s' is streamed ONCE for both nets (NT = 2: the
//                 target's and the online net's weight rows against one slab); the online features of
//                 s' wait in the dh image, which the backward fills only later.  Then the two head
//                 passes, then online(s) -- streamed with NT = 1 -- last so that its f / h stay in LDS,
//                 then wide_loss_backward: vecw_learn's loss, dA / dV, dH, dF and per-sample rows.
//                 The observation is NOT copied into the rows (vecw::X stays unwritten).
//   vect_grad     vecw_grad's 32x32 output tiles, 4 waves over four contiguous batch ranges, reduced
//                 through LDS in wave order.  The 4 ceil(obs / 32) tiles of dW0 = dF^T . x take their
//                 right operand from the ring: the batch's frame ids are staged once per workgroup in
//                 LDS, a half-wave reads 32 consecutive floats of one sample's observation.  Up to
//                 128 + 40 workgroups, fewer than the CUs of the device; per wave B / 8 dependent MFMAs.
//
// LDS per workgroup (static): slabs 33,792 + f 16,896 + h 33,280 + adv / val / q 8,576 = 92,544 B,
// + 128 B of row ids: vect_act and vect_host_eval_act 92,672 B.  vect_learn adds qt / q2 8,448,
// dA 4,608, dV 128, dh 33,280 and 256 B of ids: 139,264 B of gfx950's 163,840.  vect_grad: 16,928 B of
// reduction images + 4,096 B of ids.
#include "vector_wide_common.h"

namespace apex {

namespace {

using namespace widemfma;

constexpr int kSlab = kVecWideMaxObs;   // 128 columns of x per slab (pitch kPX)
constexpr int kQuads = kRows * kSlab / 4 / kT;   // 4 quads of a slab per thread

struct alignas(16) TallLds {
  float xs[2][kRows * kPX];
  float f[kRows * kPF];    // relu(features.0)
  float h[kRows * kPH];    // relu(advantage.0) | relu(value.0)
  float adv[kRows * kPQ];
  float val[kRows];
  float q[kRows * kPQ];
};

// quad qd of thread t in a slab: row (t + 256 qd) / 32, slab columns 4 ((t + 256 qd) % 32) .. + 3
template <class RowPtr>
__device__ __forceinline__ void slab_load(f32x4 (&pre)[kQuads], RowPtr rowp, int c0, int obs, bool vec) {
#pragma unroll
  for (int qd = 0; qd < kQuads; ++qd) {
    const int i = threadIdx.x + kT * qd;
    pre[qd] = ldw4(rowp(i >> 5), c0 + 4 * (i & 31), obs, vec);   // zero at and past obs, not read there
  }
}

__device__ __forceinline__ void slab_store(float* xs, const f32x4 (&pre)[kQuads]) {
#pragma unroll
  for (int qd = 0; qd < kQuads; ++qd) {
    const int i = threadIdx.x + kT * qd;
    *reinterpret_cast<f32x4*>(xs + (i >> 5) * kPX + 4 * (i & 31)) = pre[qd];
  }
}

// fout[t] [32][kPF] = relu(x . W0_t^T + b0_t) for the NT nets, x row r = rowp(r)[0 .. obs) (xvec: every
// row 16-byte aligned and obs % 4 == 0).  Called after a workgroup barrier (nothing reads xs or fout
// any more); the caller's next barrier completes fout.
template <int NT, class RowPtr>
__device__ __forceinline__ void tall_features(const VecNet* const (&net)[NT], float* const (&fout)[NT],
                                              float (&xs)[2][kRows * kPX], RowPtr rowp, bool xvec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5;
  const int col = wave * 32 + (lane & 31);
  const int obs = net[0]->obs, S = (obs + kSlab - 1) / kSlab;
  f32x16 acc[NT] = {};
  bool vec[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) vec[t] = rows_aligned16(net[t]->w0, obs);
  f32x4 pre[kQuads];
  slab_load(pre, rowp, 0, obs, xvec);
  slab_store(xs[0], pre);
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    const int c0 = s * kSlab, kw = min(kSlab, obs - c0);
    if (s + 1 < S) slab_load(pre, rowp, c0 + kSlab, obs, xvec);   // in flight behind this slab's MFMAs
    const size_t woff = (size_t)col * obs + c0;   // (a multiple of 4 floats whenever vec[t])
    if constexpr (NT == 1) {
      const float* const wrow[1] = {net[0]->w0 + woff};
      tile_nt<1>(acc, xs[s & 1], kPX, (kw + 7) & ~7, wrow, kw, vec, lane);
    } else {
      const float* const wrow[2] = {net[0]->w0 + woff, net[1]->w0 + woff};
      tile_nt<2>(acc, xs[s & 1], kPX, (kw + 7) & ~7, wrow, kw, vec, lane);
    }
    if (s + 1 < S) slab_store(xs[(s + 1) & 1], pre);   // (last read before the previous barrier)
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float b = net[t]->b0[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) fout[t][acc_row(i, hf) * kPF + col] = fmaxf(acc[t][i] + b, 0.f);
  }
}

// Q of the 32 rows rowp(0 .. 31) -> L.f, L.h, L.q.  Called after a barrier, ends with one.
template <class RowPtr>
__device__ __forceinline__ void tall_forward(const VecNet& n, TallLds& L, RowPtr rowp, bool xvec) {
  const VecNet* const net[1] = {&n};
  float* const fout[1] = {L.f};
  tall_features<1>(net, fout, L.xs, rowp, xvec);
  wide_heads(n, L.f, L.h, L.adv, L.val, L.q);
}

// vec_act_k's draw on a Q row: first argmax; explore iff !(u0 > eps); min(int(u1 A), A - 1)
__device__ __forceinline__ int greedy_draw(const float* row, int A, float* qout, uint64_t seed, uint64_t e,
                                           uint64_t ctr, float eps) {
  int best = 0;
  float bv = row[0];
  for (int k = 1; k < A; ++k)
    if (row[k] > bv) { bv = row[k]; best = k; }
  for (int k = 0; k < A; ++k) qout[k] = row[k];
  float u[4];
  uniform4(seed, e, ctr, u);
  if (!(u[0] > eps)) {
    const int rr = (int)(u[1] * (float)A);
    best = rr < A ? rr : A - 1;
  }
  return best;
}

// ------------------------------------------------------------------ acting
__global__ __launch_bounds__(kT) void vect_act_k(VecAct a) {
  __shared__ TallLds L;
  __shared__ int rid[kRows];
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows, obs = a.net.obs;
  if (t < kRows) rid[t] = a.hist[min(e0 + t, a.E - 1) * 4 + 3];   // rows past E repeat the last env
  __syncthreads();
  tall_forward(a.net, L, [&](int r) { return a.ring + (size_t)rid[r] * obs; }, rows_aligned16(a.ring, obs));
  const int e = e0 + t;
  if (t < kRows && e < a.E)
    a.actions[e] = greedy_draw(L.q + t * kPQ, a.net.A, a.q + (size_t)e * a.net.A, a.seed, (uint64_t)e,
                               a.counter ? (uint64_t)a.counter[0] : 0ull, a.eps[e]);
}

// vect_act_k over the staging block's reset_obs rows (rows N + e0 .. of [2 N][obs]; a padding row
// repeats the workgroup's last live row), the step k by value, epsilon 0.
__global__ __launch_bounds__(kT) void vect_host_eval_act_k(VecHostEvalAct a) {
  __shared__ TallLds L;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kRows, obs = a.net.obs;
  const int live = min(kRows, a.N - e0);   // >= 1: the grid is ceil(N / 32)
  const float* src = a.stage + (size_t)(a.N + e0) * obs;
  tall_forward(a.net, L, [&](int r) { return src + (size_t)min(r, live - 1) * obs; }, rows_aligned16(a.stage, obs));
  if (t < live)
    a.actions[e0 + t] = greedy_draw(L.q + t * kPQ, a.net.A, a.q + (size_t)(e0 + t) * a.net.A, a.seed,
                                    (uint64_t)(e0 + t), (uint64_t)a.k, 0.f);
}

// ------------------------------------------------------------------ learner
__global__ __launch_bounds__(kT) void vect_learn_k(VecLearn p) {
  __shared__ TallLds L;
  __shared__ float qt[kRows * kPQ];                   // target net on s'
  __shared__ float q2[kRows * kPQ];                   // online net on s'
  __shared__ __align__(16) float dA[kRows * kPA];     // dL/dA, zero in [A, 32)
  __shared__ float dV[kRows];
  __shared__ __align__(16) float dh[kRows * kPH];     // online features of s' first, then d(hidden)
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
    float* const fout[2] = {L.f, dh};
    tall_features<2>(net, fout, L.xs, [&](int r) { return p.ring + (size_t)sid2[r] * obs; }, xvec);
  }
  wide_heads(p.tg, L.f, L.h, L.adv, L.val, L.q);
  for (int i = t; i < kRows * kPQ; i += kT) qt[i] = L.q[i];
  wide_heads(p.on, dh, L.h, L.adv, L.val, L.q);
  for (int i = t; i < kRows * kPQ; i += kT) q2[i] = L.q[i];
  // online(s) last: its f / h stay for the backward
  tall_forward(p.on, L, [&](int r) { return p.ring + (size_t)sid[r] * obs; }, xvec);
  wide_loss_backward(p, b0, L.f, L.h, L.q, qt, q2, dA, dV, dh);
}

// ------------------------------------------------------------------ batch contraction
__global__ __launch_bounds__(kT) void vect_grad_k(VecTallGrad G) {
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
  for (int b = bs; b < be; b += 8) {  // four k steps: their eight loads are issued before the MFMAs
    float av[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int bb = b + 2 * u + hf;
      const bool in = bb < be;  // the tail is zero operands: nothing is read past the range
      av[u] = in && mok ? pg[(size_t)bb * vecw::STRIDE] : 0.f;
      xv[u] = in && nok ? px[w0 ? (size_t)sid[bb] * g.obs : (size_t)bb * vecw::STRIDE] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc = mfma32(av[u], xv[u], acc);
      bsum += av[u];
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
void vect_act(const VecAct& a, hipStream_t s) {
  if (a.ring_bf16) throw std::invalid_argument("vect_act: a bf16 ring is read by the tall bf16 kernels (vectb_*) only");
  check_tall_net(a.net, "vect_act");
  if (a.E < 1 || a.E > 4096 || !a.ring || !a.hist || !a.eps || !a.q || !a.actions)
    throw std::invalid_argument("vect_act: 1 <= E <= 4096 with ring, hist, eps, q and actions");
  vect_act_k<<<(a.E + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vect_host_eval_act(const VecHostEvalAct& a, hipStream_t s) {
  check_tall_net(a.net, "vect_host_eval_act");
  if (a.N < 1 || a.N > 64) throw std::invalid_argument("vect_host_eval_act: 1 <= N <= 64 evaluator envs");
  if (a.k < 0) throw std::invalid_argument("vect_host_eval_act: step k >= 0");
  if (!a.stage) throw std::invalid_argument("vect_host_eval_act: the staging block's device copy");
  if (!a.q || !a.actions) throw std::invalid_argument("vect_host_eval_act: q and actions");
  vect_host_eval_act_k<<<(a.N + kRows - 1) / kRows, kT, 0, s>>>(a);
  LAUNCH_CHECK();
}

void vect_learn(const VecLearn& p, hipStream_t s) {
  if (p.ring_bf16) throw std::invalid_argument("vect_learn: a bf16 ring is read by the tall bf16 kernels (vectb_*) only");
  check_tall_net(p.on, "vect_learn (online)");
  check_tall_net(p.tg, "vect_learn (target)");
  if (p.on.obs != p.tg.obs || p.on.A != p.tg.A) throw std::invalid_argument("vect_learn: nets differ in shape");
  if (p.B < 1 || p.B > 1024) throw std::invalid_argument("vect_learn: batch must be in [1, 1024]");
  if (!p.ring || !p.s_ids || !p.s2_ids || !p.act || !p.rew || !p.done || !p.idx || !p.w || !p.q_s || !p.q_s2 ||
      !p.qt_s2 || !p.vec || !p.delta || !p.lw)
    throw std::invalid_argument("vect_learn: missing buffer");
  if (p.beta_out && !(p.beta_horizon > 0.0)) throw std::invalid_argument("vect_learn: beta horizon must be > 0");
  vect_learn_k<<<(p.B + kRows - 1) / kRows, kT, 0, s>>>(p);
  LAUNCH_CHECK();
}

int vect_grad_blocks(int obs, int A) {
  if (obs < 1 || obs > kVecTallMaxObs || A < 1 || A > kVecWideMaxA)
    throw std::invalid_argument("vect_grad_blocks: obs in [1, 1024] and actions in [1, 32]");
  return 4 * ((obs + 31) / 32) + 16 + 4 + 16 + 4;
}

void vect_grad(const VecTallGrad& G, hipStream_t s) {
  if (G.ring_bf16) throw std::invalid_argument("vect_grad: a bf16 ring is read by the tall bf16 kernels (vectb_*) only");
  const VecGrad& g = G.g;
  if (g.obs < 1 || g.obs > kVecTallMaxObs || g.A < 1 || g.A > kVecWideMaxA || g.n != vec_param_count(g.obs, g.A))
    throw std::invalid_argument("vect_grad: n must be the MLP dueling net's parameter count");
  if (g.B < 1 || g.B > 1024 || !g.vec || !g.grad || !g.part || !G.ring || !G.s_ids || !G.idx)
    throw std::invalid_argument("vect_grad: batch in [1, 1024] with vec, grad, part, ring, s_ids and idx");
  vect_grad_k<<<vect_grad_blocks(g.obs, g.A), kT, 0, s>>>(G);
  LAUNCH_CHECK();
}

}  // namespace apex
