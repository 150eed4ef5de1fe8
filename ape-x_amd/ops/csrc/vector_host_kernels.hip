// Vector-observation Ape-X acting over HOST environments (engine/vector_host.py): the device half
// of one acting step whose dynamics ran on the CPU.
//
// vec_host_tail_k is vec_classic_step_k (vector_kernels.hip) with classic_dynamics replaced by the
// staged result of a gym-API vector env (envs/host_vector.py): one H2D copy brought
//
//   next_obs [E][obs] | reset_obs [E][obs] | reward [E] | done [E] | ended [E]
//
// of all E envs into `stage`, and this launch leaves the shard's per-step buffers exactly as
// vec_classic_step_k leaves them for nstep_emit:
//
//   ring row ((step + 1) E + e) mod F = reset_obs[e]  (classic_env_step's slot rule; the observation
//       the next action is chosen from: the new episode's first one after an end), new_frame[e]
//       the row;
//   reward[e] copied, done[e] the env's own flag as 1.f / 0.f -- a length-cap reset (`ended` set,
//       `done` clear) keeps done = 0;
//   the running return / length of env e (fp32, step order, as gst[EPRET] / gst[EPLEN]); on `ended`
//       ep_log[e] = (return, length, count + 1, untouched) and the pair is cleared.
//
// The reset form (vec_classic_reset_k's contract) writes reset_obs into row (step E + e) mod F, all
// four hist[e] entries and new_frame[e] to that row, and zeroes ep_log[e] and the running pair.
//
// One thread per (env, component): the staged block is read and the ring row written with
// consecutive lanes on consecutive addresses; the k == 0 lane of an env does its scalars.  No
// workgroup depends on another (nstep_emit bumps the step counter afterwards).  Only device memory
// is touched, with vector loads and stores; every index is bounded by E, obs and F (checked by
// the launcher).
#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace apex {
namespace {

constexpr int kTailThreads = 256;

__global__ __launch_bounds__(kTailThreads) void vec_host_tail_k(VecHostTail T, int reset) {
  const int i = blockIdx.x * kTailThreads + threadIdx.x;
  const int E = T.E, obs = T.obs;
  if (i >= E * obs) return;
  const int e = i / obs, k = i - e * obs;
  const float* reset_obs = T.stage + (size_t)E * obs;
  const int64_t step = T.step[0] + (reset ? 0 : 1);
  const int slot = (int)((step * E + e) % T.F);
  T.ring[(size_t)slot * obs + k] = reset_obs[i];
  if (k != 0) return;
  T.new_frame[e] = slot;
  float* lg = T.ep_log + (size_t)e * 4;
  if (reset) {
    for (int c = 0; c < 4; ++c) T.hist[e * 4 + c] = slot;
    for (int c = 0; c < 4; ++c) lg[c] = 0.f;
    T.ep_ret[e] = 0.f;
    T.ep_len[e] = 0.f;
    return;
  }
  const float* reward = reset_obs + (size_t)E * obs;
  const float r = reward[e];
  const float done = reward[E + e];
  const bool ended = reward[2 * E + e] != 0.f;
  T.reward[e] = r;
  T.done[e] = done != 0.f ? 1.f : 0.f;
  const float ep_ret = T.ep_ret[e] + r;
  const float ep_len = T.ep_len[e] + 1.f;
  if (ended) {
    lg[0] = ep_ret;
    lg[1] = ep_len;
    lg[2] += 1.f;
    T.ep_ret[e] = 0.f;
    T.ep_len[e] = 0.f;
  } else {
    T.ep_ret[e] = ep_ret;
    T.ep_len[e] = ep_len;
  }
}

}  // namespace

void vec_host_tail(const VecHostTail& a, bool reset, hipStream_t s) {
  if (a.E < 1 || a.E > 4096) throw std::invalid_argument("vec_host_tail: 1 <= envs <= 4096");
  if (a.obs < 1 || a.obs > kVecMaxObs) throw std::invalid_argument("vec_host_tail: 1 <= obs <= 8");
  if (a.F < 2 * a.E) throw std::invalid_argument("vec_host_tail: ring must hold >= 2 E rows");
  if (!a.stage || !a.ring || !a.step || !a.reward || !a.done || !a.new_frame || !a.hist || !a.ep_log || !a.ep_ret ||
      !a.ep_len)
    throw std::invalid_argument("vec_host_tail: missing buffers");
  const int n = a.E * a.obs;
  vec_host_tail_k<<<(n + kTailThreads - 1) / kTailThreads, kTailThreads, 0, s>>>(a, reset ? 1 : 0);
  LAUNCH_CHECK();
}

}  // namespace apex
