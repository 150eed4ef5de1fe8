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
//
// Everything after features.0 (the heads, the draw, the loss and backward, the contraction's tile map
// and reduction) is in vector_wide_bf16_common.h, shared with the tall mode's bf16 kernels.
#include "vector_wide_bf16_common.h"

namespace apex {

namespace {

using namespace widebf16;

// ------------------------------------------------------------------ forward
struct alignas(16) WideLdsB {
  __bf16 x[kRows * kPX];
  __bf16 f[kRows * kPF];    // relu(features.0)
  __bf16 h[kRows * kPH];    // relu(advantage.0) | relu(value.0)
  float adv[kRows * kPQ];
  float val[kRows];
  float q[kRows * kPQ];
};

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
  heads_b(n, L.f, L.h, L.adv, L.val, L.q);
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
    draw(L.q + t * kPQ, e, a.net.A, a.eps[e], a.seed, a.counter ? (uint64_t)a.counter[0] : 0ull, a.q, a.actions);
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
  if (t < live) draw(L.q + t * kPQ, e0 + t, a.net.A, 0.f, a.seed, (uint64_t)a.k, a.q, a.actions);
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
  const int t = threadIdx.x;
  const int b0 = blockIdx.x * kRows;
  const int obs = p.on.obs;
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
  // the observation's row as the rounded values the MFMAs consumed (L.x is complete and stays)
  const int live = min(kRows, p.B - b0);
  for (int i = t; i < live * obs; i += kT) {
    const int row = i / obs, k = i - row * obs;
    p.vec[(size_t)(b0 + row) * vecw::STRIDE + vecw::X + k] = (float)L.x[row * kPX + k];
  }
  loss_backward_b(p, b0, L.f, L.h, L.q, qt, q2, dAf, dA, dh);
}

// ------------------------------------------------------------------ batch contraction
__global__ __launch_bounds__(kT) void vecwb_grad_k(VecGrad g) {
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
void vecwb_act(const VecAct& a, hipStream_t s) {
  if (a.ring_bf16) throw std::invalid_argument("vecwb_act: a bf16 ring is read by the tall bf16 kernels (vectb_*) only");
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
  if (p.ring_bf16) throw std::invalid_argument("vecwb_learn: a bf16 ring is read by the tall bf16 kernels (vectb_*) only");
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
