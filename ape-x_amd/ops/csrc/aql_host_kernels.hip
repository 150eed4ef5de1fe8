// AQL acting over HOST environments (engine/aql_host.py): the device half of one acting step
// whose dynamics ran on the CPU.
//
// aql_host_tail_k is aql_act_tail_k (aql_engine_kernels.hip) without the selection (aql_select
// ran before the actions went to the host) and with env_dynamics replaced by the staged result of
// a gym-API vector env (envs/host_vector.py): one H2D copy brought next_obs | reset_obs | reward |
// done | ended of all E envs into `stage`, and this launch turns them into replay rows.
//
//   workgroups 0 .. ceil(E/4) - 1 : a wave per env.  The raw transition (the observation acted
//       on, the candidate set, the chosen candidate, reward, done, the step's observation -- the
//       terminal one when the episode ended) into ring slot (filled + e) mod C, the slot into
//       slots[e]; env_step_wave's episode bookkeeping with `ended` (done or the length cap) as
//       its end-of-episode flag; obs_buf[e] = reset_obs[e] (the new episode's first observation
//       after an end, the step's observation otherwise).
//   workgroup ceil(E/4)           : the E ring leaves at the max priority and their levels
//       (ring_write_block, tree_dev.h: the tree block of aql_act_tail_k) + the learner's PER beta.
//   the last workgroup to finish  : filled += E, counter += 1, iter += 1, ticket = 0 (every
//       workgroup has read filled by then).
//
// Only device memory is touched, with vector loads and stores; every index is bounded by E, obs,
// T * adim and C (checked by the launcher).
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "tree_dev.h"

namespace apex {
namespace {

__global__ __launch_bounds__(256) void aql_host_tail_k(AqlHostTail A) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int E = A.E, obs = A.obs;
  const int nenv = (E + 3) / 4;
  if ((int)blockIdx.x < nenv) {
    const int e = blockIdx.x * 4 + wave;
    if (e < E) {  // wave-uniform
      const AqlInsert& I = A.I;
      const float* next_obs = A.stage;
      const float* reset_obs = next_obs + (size_t)E * obs;
      const float* reward = reset_obs + (size_t)E * obs;
      const float r = reward[e], done = reward[E + e];
      const bool ended = reward[2 * E + e] != 0.f;
      const int64_t slot = (A.filled[0] + e) % I.C;
      if (lane < obs) {
        I.st[slot * obs + lane] = A.obs_buf[(size_t)e * obs + lane];
        I.st2[slot * obs + lane] = next_obs[(size_t)e * obs + lane];
      }
      const int TA = A.T * A.adim;
      for (int k = lane; k < TA; k += 64) I.amu[slot * TA + k] = A.amu[(size_t)e * TA + k];
      if (lane < obs) A.obs_buf[(size_t)e * obs + lane] = reset_obs[(size_t)e * obs + lane];
      if (lane == 0) {
        I.act[slot] = A.act_idx[e];
        I.rew[slot] = r;
        I.done[slot] = done != 0.f ? 1.f : 0.f;
        I.slots[e] = (int)slot;
        const int len = A.ep_len[e] + 1;
        if (ended) {
          const int k = atomicAdd(A.ep_count, 1);
          float* lg = A.ep_log + (size_t)(k % A.log_cap) * 2;
          lg[0] = A.ep_ret[e] + r;
          lg[1] = (float)len;
          A.ep_len[e] = 0;
          A.ep_ret[e] = 0.f;
        } else {
          A.ep_len[e] = len;
          A.ep_ret[e] += r;
        }
      }
    }
  } else {
    if (t == 0 && A.beta_out)
      A.beta_out[0] = tail_beta(A.iter[0], A.beta0, A.beta_omb, A.beta_max_step, A.beta_workers);
    ring_write_block(A.tree, A.filled[0], A.I.C, E, *A.max_prio, A.alpha);
  }
  __syncthreads();
  if (t == 0) {
    __threadfence();
    if (atomicAdd(A.ticket, 1) == (int)gridDim.x - 1) {  // the last workgroup: every read of the counters is done
      A.filled[0] += E;
      A.counter[0] += 1;
      if (A.iter) A.iter[0] += 1;
      A.ticket[0] = 0;
    }
  }
}

}  // namespace

void aql_host_tail(const AqlHostTail& a, hipStream_t s) {
  if (a.E > 1024) throw std::invalid_argument("aql_host_tail: at most 1024 envs (one tree workgroup)");
  if (a.obs < 1 || a.obs > 64) throw std::invalid_argument("aql_host_tail: 1 <= obs <= 64");
  if (a.adim < 1 || a.adim > 8) throw std::invalid_argument("aql_host_tail: 1 <= action dim <= 8");
  if (a.T < 1 || a.log_cap < 1) throw std::invalid_argument("aql_host_tail: T >= 1, log_cap >= 1");
  const AqlInsert& I = a.I;
  if (I.C < a.E) throw std::invalid_argument("aql_host_tail: replay capacity < envs");
  if (I.C > ((int64_t)1 << 31) || a.tree.size[0] < I.C || a.tree.levels < 1)
    throw std::invalid_argument("aql_host_tail: the tree must cover the ring");
  if (!I.st || !I.st2 || !I.rew || !I.done || !I.amu || !I.act || !I.slots)
    throw std::invalid_argument("aql_host_tail: replay tables");
  if (!a.filled || (const void*)a.filled != (const void*)I.filled)
    throw std::invalid_argument("aql_host_tail: filled must be the ring's fill count");
  if (!a.stage || !a.obs_buf || !a.amu || !a.act_idx || !a.ep_len || !a.ep_ret || !a.ep_count || !a.ep_log ||
      !a.max_prio || !a.counter || !a.ticket || (a.beta_out && !a.iter))
    throw std::invalid_argument("aql_host_tail: missing buffers");
  if (a.E < 1) return;
  aql_host_tail_k<<<(a.E + 3) / 4 + 1, 256, 0, s>>>(a);
  LAUNCH_CHECK();
}

}  // namespace apex
