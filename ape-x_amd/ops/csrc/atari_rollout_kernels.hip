// atari_rollout: n_steps greedy steps of every Atari evaluator env in ONE launch (gfx950).
//
// The stepwise evaluator (GPUEvaluator.step) pays about 8 launches per env step: conv1, conv2,
// conv3, FC1 and heads of F32DuelingNet, then vec_env_step and frame_hist_step.  Here one
// 1024-thread workgroup owns one env for the whole launch and loops
//   forward (one sample, inside the workgroup) -> first argmax / epsilon draw -> env step ->
//   render -> observation-stack advance
// with the stepwise kernels' Philox keys (select_actions at counter + k; the env's words
// (counter + k) * 16 + 2 + f and + 7 through atari_env_dev.h), so the env buffers after the
// launch are those n_steps stepwise steps leave, bit for bit, whenever both nets pick the same
// actions.  (Q itself is fp32-class in another accumulation order, not bit-equal.)
//
// The forward -- LDS layout, conv1 on v_mfma_f32_32x32x16_bf16 with the exact three-term split,
// conv2 / conv3 on v_mfma_f32_32x32x2_f32 with fixed-order k-part adds, FC1 and the heads on the
// VALU -- is atari_fwd_dev.h's, shared with host_eval_act_k.  Here the 4-frame stack `fr` is loaded
// once through hist, then only the rendered frame is added per step.
//
// No workgroup writes a word another workgroup of the launch reads: env e owns state row e, its
// hist / log rows and the frame-ring slots j * E + e; the step counter is only read.  The step
// loop is bounded by n_steps with a fixed number of workgroup-uniform barriers per iteration.
#include <stdexcept>

#include "atari_env_dev.h"
#include "atari_fwd_dev.h"
#include "common.h"
#include "kernels.h"

namespace apex {
namespace {

using namespace atari_fwd;

__global__ __launch_bounds__(kT) void atari_rollout_k(AtariRollout R) {
  __shared__ __attribute__((aligned(16))) uint32_t fr[4 * kFrameDw];
  __shared__ __attribute__((aligned(16))) uint16_t w1b[3][256 * 32];  // hi / mid / lo bf16 planes
  __shared__ __attribute__((aligned(16))) float a1[400 * kP1];  // a3 [49][64] after conv2
  __shared__ __attribute__((aligned(16))) float a2[81 * kP2];
  __shared__ float zs[512], hs[256], advs[32], qs[32], sst[S_STRIDE], s_log[4], s_rew;
  __shared__ int s_hist[4], s_done, s_act, s_gslot;
  const VecEnvParams& p = R.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = blockIdx.x;
  const int A = p.n_actions, E = p.E;
  const int64_t step0 = R.counter[0];

  // ---- stage once: conv1 weight, the 4-frame stack, the env's state / log / hist rows
  stage_w1(R.w1, w1b, tid);
  for (int c = 0; c < 4; ++c) {
    const int id = min(max(R.hist[e * 4 + c], 0), p.F - 1);  // (a frame id is always a ring slot)
    const uint32_t* src = reinterpret_cast<const uint32_t*>(R.frames + (size_t)id * p.frame_bytes);
    for (int i = tid; i < kFrameDw; i += kT) fr[c * kFrameDw + i] = src[i];
  }
  if (tid < S_STRIDE) sst[tid] = R.env_state[(size_t)e * S_STRIDE + tid];
  if (tid < 4) {
    s_log[tid] = R.ep_log[e * 4 + tid];
    s_hist[tid] = R.hist[e * 4 + tid];
  }
  int csp = 0 | (1 << 2) | (2 << 4) | (3 << 6);  // LDS slot of stack channel c: (csp >> 2c) & 3
  __syncthreads();

  for (int k = 0; k < R.n_steps; ++k) {
    const int64_t step = step0 + k;
    forward(R, fr, csp, w1b, a1, a2, zs, hs, advs, A, tid, lane, wave);
    // ---- dueling combine, action (select_actions' rule and draw), env step (thread 0)
    if (tid == 0) {
      const int best = combine_select(advs, qs, A, R.act_seed, e, step, R.eps[e]);
      float st[S_STRIDE];
#pragma unroll
      for (int i = 0; i < S_STRIDE; ++i) st[i] = sst[i];
      const EnvStepOut o = env_step_state(st, best, R.env_seed, e, step, p);
#pragma unroll
      for (int i = 0; i < S_STRIDE; ++i) sst[i] = st[i];
      if (o.done) {
        if (R.ep_ring) {
          float* ring = R.ep_ring + ((size_t)e * R.ring_R + (int)s_log[2] % R.ring_R) * 2;
          ring[0] = o.ep_ret;
          ring[1] = o.ep_len;
        }
        s_log[0] = o.ep_ret;
        s_log[1] = o.ep_len;
        s_log[2] += 1.f;
      }
      const int gslot = (int)(((int64_t)(step + 1) * E + e) % p.F);
      if (o.done) {
        s_hist[0] = s_hist[1] = s_hist[2] = s_hist[3] = gslot;
      } else {
        s_hist[0] = s_hist[1]; s_hist[1] = s_hist[2]; s_hist[2] = s_hist[3]; s_hist[3] = gslot;
      }
      s_done = o.done ? 1 : 0;
      s_rew = o.reward;
      s_act = best;
      s_gslot = gslot;
      if (R.trace_q && k < R.trace_T) {
        const size_t row = (size_t)e * R.trace_T + k;
        R.trace_act[row] = best;
        R.trace_rew[row] = o.reward;
        R.trace_done[row] = o.done ? 1.f : 0.f;
      }
    }
    __syncthreads();
    if (R.trace_q && k < R.trace_T && tid < A) R.trace_q[((size_t)e * R.trace_T + k) * A + tid] = qs[tid];
    // ---- render into a free LDS slot (one no channel of the next stack but the newest uses) and
    // the global ring; the stack becomes 4 x the new frame on done, else shifts
    {
      const int used = (1 << ((csp >> 2) & 3)) | (1 << ((csp >> 4) & 3)) | (1 << ((csp >> 6) & 3));
      const int ns = !(used & 1) ? 0 : !(used & 2) ? 1 : !(used & 4) ? 2 : 3;
      csp = s_done ? ns * 0x55 : ((csp >> 2) | (ns << 6));
      render_frame(sst, R.frames + (size_t)s_gslot * p.frame_bytes, fr + ns * kFrameDw);
    }
    __syncthreads();
  }
  // ---- leave every buffer as the stepwise kernels do
  if (tid < S_STRIDE) R.env_state[(size_t)e * S_STRIDE + tid] = sst[tid];
  if (tid < 4) {
    R.ep_log[e * 4 + tid] = s_log[tid];
    R.hist[e * 4 + tid] = s_hist[tid];
  }
  if (tid == 0) {
    R.new_frame[e] = s_gslot;
    R.reward[e] = s_rew;
    R.done[e] = s_done ? 1.f : 0.f;
    R.actions[e] = s_act;
  }
}

}  // namespace

// Limits: 1 <= n_steps <= 10000, 1 <= E <= 64 envs, 18 or <= 6 actions, an 8 E-slot ring of
// 84 x 84 frames (the evaluator's), 16-byte aligned arena weights.
void atari_rollout(const AtariRollout& r, hipStream_t s) {
  const VecEnvParams& p = r.p;
  if (r.n_steps < 1 || r.n_steps > 10000) throw std::invalid_argument("atari_rollout: 1 <= n_steps <= 10000");
  if (p.E < 1 || p.E > 64) throw std::invalid_argument("atari_rollout: 1 <= E <= 64");
  if (p.n_actions < 1 || (p.n_actions != 18 && p.n_actions > 6))
    throw std::invalid_argument("atari_rollout: 18 or <= 6 actions");
  if (p.F != 8 * p.E) throw std::invalid_argument("atari_rollout: the frame ring holds F = 8 E frames");
  if (p.frame_bytes != kScreen * kScreen) throw std::invalid_argument("atari_rollout: 84x84 frames");
  if (!r.w1 || !r.b1 || !r.w2p || !r.b2 || !r.w3p || !r.b3 || !r.wfc1p || !r.ba1 || !r.bv1 || !r.wa2 || !r.ba2 ||
      !r.wv2 || !r.bv2)
    throw std::invalid_argument("atari_rollout: missing weights");
  if ((reinterpret_cast<uintptr_t>(r.w2p) | reinterpret_cast<uintptr_t>(r.w3p) |
       reinterpret_cast<uintptr_t>(r.wfc1p)) & 15)
    throw std::invalid_argument("atari_rollout: w2p / w3p / wfc1p must be 16-byte aligned");
  if (!r.eps || !r.counter || !r.env_state || !r.hist || !r.frames || !r.new_frame || !r.ep_log || !r.reward ||
      !r.done || !r.actions)
    throw std::invalid_argument("atari_rollout: missing env buffers");
  if (reinterpret_cast<uintptr_t>(r.frames) & 3)
    throw std::invalid_argument("atari_rollout: frames must be 4-byte aligned");
  if (r.ep_ring && r.ring_R < 1) throw std::invalid_argument("atari_rollout: ring_R >= 1 with an episode ring");
  const int ntr = (r.trace_q != nullptr) + (r.trace_act != nullptr) + (r.trace_rew != nullptr) +
                  (r.trace_done != nullptr);
  if (ntr != 0 && ntr != 4) throw std::invalid_argument("atari_rollout: all four trace pointers or none");
  if (ntr == 4 && r.trace_T < 1) throw std::invalid_argument("atari_rollout: trace_T >= 1");
  atari_rollout_k<<<p.E, kT, 0, s>>>(r);
  LAUNCH_CHECK();
}

}  // namespace apex
