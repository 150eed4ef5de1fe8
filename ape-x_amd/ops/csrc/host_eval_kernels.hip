// host_eval_act: the act half of one evaluator step over HOST emulators in ONE launch (gfx950).
//
// A host-env evaluator step built from the existing kernels is 7 launches: host_env_ingest,
// frame_hist_step, then conv1 / conv2 / conv3 / FC1 / heads of F32DuelingNet.  Here the last six
// are one launch behind the ingest: one 1024-thread workgroup per evaluator env
//   observation-stack advance (frame_hist_step_k's rule) -> stage the 4 frames from the private
//   ring -> the in-workgroup fp32 forward (atari_fwd_dev.h, atari_rollout_k's) -> Q row and the
//   action by select_actions_k's rule and draw at Philox key (act_seed, e, step).
// `step` is passed by value (the evaluator launches eagerly and knows its step); with advance != 0
// thread 0 of workgroup 0 stores counter[0] = step for the NEXT launch of host_env_ingest to read.
// No thread of this kernel reads the counter, so the store cannot race.
//
// No workgroup writes a word another workgroup of the launch reads: env e owns hist row e, q row e
// and actions[e]; the ring, new_frame, done and eps are only read.  LDS is the rollout kernel's
// (about 156 KiB of the CU's 160 KiB), so one workgroup per CU.
#include <stdexcept>
#include <string>

#include "atari_fwd_dev.h"
#include "common.h"
#include "kernels.h"

namespace apex {
namespace {

using namespace atari_fwd;

__global__ __launch_bounds__(kT) void host_eval_act_k(HostEvalAct R) {
  __shared__ __attribute__((aligned(16))) uint32_t fr[4 * kFrameDw];
  __shared__ __attribute__((aligned(16))) uint16_t w1b[3][256 * 32];  // hi / mid / lo bf16 planes
  __shared__ __attribute__((aligned(16))) float a1[kA1Floats];  // a3 [49][64] after conv2
  __shared__ __attribute__((aligned(16))) float a2[kA2Floats];
  __shared__ float zs[512], hs[256], advs[32], qs[32];
  __shared__ int s_hist[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = blockIdx.x;
  const int A = R.A;

  // ---- the env's hist row, advanced as frame_hist_step_k does; the counter for the next ingest
  if (tid == 0) {
    int h0 = R.hist[e * 4 + 0], h1 = R.hist[e * 4 + 1], h2 = R.hist[e * 4 + 2], h3 = R.hist[e * 4 + 3];
    if (R.advance) {
      const int f = R.new_frame[e];
      if (R.done[e] > 0.f) {
        h0 = h1 = h2 = h3 = f;
      } else {
        h0 = h1; h1 = h2; h2 = h3; h3 = f;
      }
      R.hist[e * 4 + 0] = h0; R.hist[e * 4 + 1] = h1; R.hist[e * 4 + 2] = h2; R.hist[e * 4 + 3] = h3;
      if (e == 0) R.counter[0] = R.step;
    }
    s_hist[0] = h0; s_hist[1] = h1; s_hist[2] = h2; s_hist[3] = h3;
  }
  stage_w1(R.w1, w1b, tid);
  __syncthreads();
  // ---- stage the 4-frame stack (a frame id is clamped to a ring slot: never a read outside the ring)
  for (int c = 0; c < 4; ++c) {
    const int id = min(max(s_hist[c], 0), R.F - 1);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(R.frames + (size_t)id * R.frame_bytes);
    for (int i = tid; i < kFrameDw; i += kT) fr[c * kFrameDw + i] = src[i];
  }
  __syncthreads();
  constexpr int csp = 0 | (1 << 2) | (2 << 4) | (3 << 6);  // stack channel c sits in LDS slot c
  forward(R, fr, csp, w1b, a1, a2, zs, hs, advs, A, tid, lane, wave);
  if (tid == 0) R.actions[e] = combine_select(advs, qs, A, R.act_seed, e, R.step, R.eps[e]);
  __syncthreads();
  if (tid < A) R.q[(size_t)e * A + tid] = qs[tid];
}

}  // namespace

// Limits: 1 <= N <= 64 envs, 1 <= A <= 18 actions, an 8 N-slot ring of 84 x 84 frames, 16-byte
// aligned arena weights, a 4-byte aligned ring, every pointer present.
void host_eval_act(const HostEvalAct& r, hipStream_t s) {
  if (r.N < 1 || r.N > 64) throw std::invalid_argument("host_eval_act: 1 <= N <= 64");
  if (r.A < 1 || r.A > 18) throw std::invalid_argument("host_eval_act: 1 <= A <= 18");
  if (r.F != 8 * r.N) throw std::invalid_argument("host_eval_act: the frame ring holds F = 8 N frames");
  if (r.frame_bytes != 84 * 84) throw std::invalid_argument("host_eval_act: 84x84 frames");
  if (r.step < 0) throw std::invalid_argument("host_eval_act: step >= 0");
  if (!r.w1 || !r.b1 || !r.w2p || !r.b2 || !r.w3p || !r.b3 || !r.wfc1p || !r.ba1 || !r.bv1 || !r.wa2 || !r.ba2 ||
      !r.wv2 || !r.bv2)
    throw std::invalid_argument("host_eval_act: missing weights");
  if ((reinterpret_cast<uintptr_t>(r.w2p) | reinterpret_cast<uintptr_t>(r.w3p) |
       reinterpret_cast<uintptr_t>(r.wfc1p)) & 15)
    throw std::invalid_argument("host_eval_act: w2p / w3p / wfc1p must be 16-byte aligned");
  if (!r.eps || !r.frames || !r.hist || !r.new_frame || !r.done || !r.counter || !r.q || !r.actions)
    throw std::invalid_argument("host_eval_act: missing env buffers");
  if (reinterpret_cast<uintptr_t>(r.frames) & 3)
    throw std::invalid_argument("host_eval_act: frames must be 4-byte aligned");
  host_eval_act_k<<<r.N, kT, 0, s>>>(r);
  LAUNCH_CHECK();
}

}  // namespace apex
