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
#include "vector_wide_common.h"

namespace apex {

namespace {

using namespace widemfma;  // the operand scheme, the heads, loss + backward, the contraction tiles

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
  wide_heads(n, L.f, L.h, L.adv, L.val, L.q);
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
  const int t = threadIdx.x;
  const int b0 = blockIdx.x * kRows;
  const int obs = p.on.obs, kp = (obs + 7) & ~7;
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
  wide_loss_backward(p, b0, L.f, L.h, L.q, qt, q2, dA, dV, dh);
  // the observation rows out of LDS, a row's floats on consecutive lanes
  const int live = min(kRows, p.B - b0);
  for (int i = t; i < live * kp; i += kT) {
    const int row = i / kp, k = i - row * kp;
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::X + k] = L.x[row * kPX + k];
  }
}

// ------------------------------------------------------------------ batch contraction
__global__ __launch_bounds__(kT) void vecw_grad_k(VecGrad g) {
  __shared__ GradRed R;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, hf = lane >> 5;
  const GradTile T = grad_tile(blockIdx.x, g.obs, g.A);
  const int chunk = grad_chunk(g.B);
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
  grad_finish(R, acc, bsum, T, g.grad, g.part);
}

void check_wide_net(const VecNet& n, const char* who) {
  if (n.obs < 1 || n.obs > kVecWideMaxObs || n.A < 1 || n.A > kVecWideMaxA)
    throw std::invalid_argument(std::string(who) + ": obs in [1, 128] and actions in [1, 32]");
  if (n.atoms != 0) throw std::invalid_argument(std::string(who) + ": categorical heads (atoms != 0) are vecd_*'s");
  if (!n.w0 || !n.b0 || !n.wa1 || !n.ba1 || !n.wa2 || !n.ba2 || !n.wv1 || !n.bv1 || !n.wv2 || !n.bv2)
    throw std::invalid_argument(std::string(who) + ": missing parameter tensor");
}

}  // namespace

// ------------------------------------------------------------------ launchers
void vecw_act(const VecAct& a, hipStream_t s) {
  if (a.ring_bf16) throw std::invalid_argument("vecw_act: a bf16 ring is read by the tall bf16 kernels (vectb_*) only");
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
  if (p.ring_bf16) throw std::invalid_argument("vecw_learn: a bf16 ring is read by the tall bf16 kernels (vectb_*) only");
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
