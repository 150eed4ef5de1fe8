// Front end for host (gym-API) Atari emulators under the fused Ape-X engine, gfx950.
//
// A host env hands over, per agent step, the two unpooled RGB emulator frames whose
// element-wise max is the observation ([E][2][H][W][3] u8, copied H2D by the engine), the raw
// window reward and the agent-level done.  host_env_ingest_k does the pixel work of the host
// pipeline (envs/preprocess.py: max-pool, grey, separable area resize, round, channels-first
// transpose) in fp64 and writes the 84x84 plane into the HBM frame ring at the slot
// vec_env_step_k would have used, with the same reward / done / new_frame / ep_log outputs:
// everything downstream (conv1 on the ring, nstep_emit, the tree, the learner) is shared.
//
// Grid (n, 84 / kBand) over the env range [e0, e0 + n): one workgroup warps kBand = 4 output rows h
// of env e0 + blockIdx.x.  Slots, raw addressing, the bounds guard and the bookkeeping rows all use
// the absolute env index over the whole shard's buffers, so a range launch writes exactly what the
// whole launch (e0 = 0, n = E) writes for those envs and nothing else.  The workgroup stages the
// input rows those need (two frames) into LDS with aligned 32-bit loads -- the band is one
// contiguous byte range per frame -- runs the row pass over the band (grey formed on the
// fly), then the column pass, and stores the 4 bytes of each output column w as one word:
// the plane is transposed (frames[slot][w * 84 + h]) and h0 is a multiple of 4.
#include "common.h"
#include "kernels.h"

namespace apex {

namespace {
constexpr int kOut = kHostEnvOut;
constexpr int kTaps = kHostEnvTaps;
constexpr int kBand = 4;           // output rows per workgroup
constexpr int kMaxLds = 64 * 1024;

// input rows a band of kBand output rows can span at scale H / 84
inline int band_rows(int H) { return (kBand * H + kOut - 1) / kOut + 2; }
// staged bytes per frame: the band + up to 3 bytes of alignment slack in front, whole words
inline int region_words(int H, int W) { return (band_rows(H) * W * 3 + 3 + 3) / 4; }
}  // namespace

__global__ __launch_bounds__(256) void host_env_ingest_k(
    const uint8_t* __restrict__ raw, const float* __restrict__ reward_in, const float* __restrict__ done_in,
    HostEnvTaps rows, HostEnvTaps cols, uint8_t* __restrict__ frames, HostEnvParams p,
    const int64_t* __restrict__ step_counter, int reset, int band, int reg_words, int e0, float* reward,
    float* done, int* new_frame, int* hist, float* acc, float* ep_log) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int e = e0 + blockIdx.x, h0 = blockIdx.y * kBand, tid = threadIdx.x;
  const int H = p.H, W = p.W;
  const int64_t step = step_counter[0];
  const int slot = (int)(((step + (reset ? 0 : 1)) * (int64_t)p.E + e) % p.F);

  // LDS: [2][reg_words] staged raw words | [kBand][W] fp64 row-pass results | [84][kBand] bytes
  uint32_t* stage = reinterpret_cast<uint32_t*>(smem);
  double* tmp = reinterpret_cast<double*>(smem + (size_t)((2 * reg_words + 1) / 2) * 8);
  uint8_t* outb = reinterpret_cast<uint8_t*>(tmp + kBand * W);

  // the band's input rows [i0, i1), clamped so a bad table can never index outside the stage
  const int hl_last = h0 + kBand - 1;
  int i0 = min(max(rows.first[h0], 0), H);
  int i1 = min(min(rows.first[hl_last] + min(rows.count[hl_last], kTaps), H), i0 + band);
  i1 = max(i1, i0);
  const int64_t frame_len = (int64_t)H * W * 3, total = (int64_t)p.E * 2 * frame_len;
  int shift[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int64_t g0 = ((int64_t)e * 2 + f) * frame_len + (int64_t)i0 * W * 3;
    const int64_t g1 = g0 + (int64_t)(i1 - i0) * W * 3;
    const int64_t a0 = g0 & ~(int64_t)3;
    shift[f] = (int)(g0 - a0);
    const int nw = min((int)((g1 - a0 + 3) >> 2), reg_words);
    for (int k = tid; k < nw; k += blockDim.x) {
      const int64_t off = a0 + 4 * (int64_t)k;
      uint32_t v;
      if (off + 4 <= total) {
        v = *reinterpret_cast<const uint32_t*>(raw + off);
      } else {  // the last word of the whole buffer: never read past its end
        v = 0;
        for (int j = 0; j < 4; ++j)
          if (off + j < total) v |= (uint32_t)raw[off + j] << (8 * j);
      }
      stage[f * reg_words + k] = v;
    }
  }
  __syncthreads();

  // row pass: tmp[hl][j] = sum_t rows[h][t] * grey(max(raw0, raw1))[first + t][j]
  const uint8_t* s0 = reinterpret_cast<const uint8_t*>(stage) + shift[0];
  const uint8_t* s1 = reinterpret_cast<const uint8_t*>(stage + reg_words) + shift[1];
  for (int it = tid; it < kBand * W; it += blockDim.x) {
    const int hl = it / W, j = it - hl * W, h = h0 + hl;
    const int fi = rows.first[h], c = min(rows.count[h], kTaps);
    double a = 0.0;
    for (int t = 0; t < c; ++t) {
      const int i = fi + t;
      if (i < i0 || i >= i1) continue;
      const int q = ((i - i0) * W + j) * 3;
      const double r = (double)max(s0[q], s1[q]);
      const double g = (double)max(s0[q + 1], s1[q + 1]);
      const double b = (double)max(s0[q + 2], s1[q + 2]);
      const double grey = 0.299 * r + 0.587 * g + 0.114 * b;
      a += rows.weight[h * kTaps + t] * grey;
    }
    tmp[it] = a;
  }
  __syncthreads();

  // column pass, round half to even, clamp
  for (int it = tid; it < kOut * kBand; it += blockDim.x) {
    const int w = it / kBand, hl = it - w * kBand;
    const int fj = cols.first[w], c = min(cols.count[w], kTaps);
    double a = 0.0;
    for (int t = 0; t < c; ++t) {
      const int j = fj + t;
      if (j < 0 || j >= W) continue;
      a += cols.weight[w * kTaps + t] * tmp[hl * W + j];
    }
    a = fmin(fmax(rint(a), 0.0), 255.0);
    outb[it] = (uint8_t)(int)a;
  }
  __syncthreads();
  if (tid < kOut) {
    uint8_t* dst = frames + (size_t)slot * p.frame_bytes + tid * kOut + h0;
    *reinterpret_cast<uint32_t*>(dst) = reinterpret_cast<const uint32_t*>(outb)[tid];
  }

  // bookkeeping, one lane per env (vec_env_step_k's outputs)
  if (blockIdx.y == 0 && tid == 0) {
    float* ac = acc + e * 4;  // clipped return, raw return, length
    new_frame[e] = slot;
    if (reset) {
      for (int c = 0; c < 4; ++c) {
        hist[e * 4 + c] = slot;
        ep_log[e * 4 + c] = 0.f;
        ac[c] = 0.f;
      }
    } else {
      const float rr = reward_in[e];
      const float r = p.clip_rewards ? (rr > 0.f ? 1.f : (rr < 0.f ? -1.f : 0.f)) : rr;
      const bool d = done_in[e] > 0.5f;
      reward[e] = r;
      done[e] = d ? 1.f : 0.f;
      ac[0] += r;
      ac[1] += rr;
      ac[2] += 1.f;
      if (d) {
        ep_log[e * 4 + 0] = ac[0];
        ep_log[e * 4 + 1] = ac[2];
        ep_log[e * 4 + 2] += 1.f;
        ep_log[e * 4 + 3] = ac[1];
        ac[0] = ac[1] = ac[2] = 0.f;
      }
    }
  }
}

void host_env_ingest_range(const uint8_t* raw, const float* reward_in, const float* done_in, const HostEnvTaps& rows,
                           const HostEnvTaps& cols, uint8_t* frames, const HostEnvParams& p,
                           const int64_t* step_counter, bool reset, float* reward, float* done, int* new_frame,
                           int* hist, float* acc, float* ep_log, int e0, int n, hipStream_t s) {
  if (p.H < kOut || p.W < kOut) throw std::invalid_argument("host_env_ingest: the warp only shrinks (H, W >= 84)");
  if (rows.max_count > kTaps || cols.max_count > kTaps || rows.max_count < 1 || cols.max_count < 1)
    throw std::invalid_argument("host_env_ingest: tap count above the table width (" + std::to_string(kTaps) + ")");
  if (p.E <= 0 || p.F <= 0 || p.frame_bytes < kOut * kOut || p.frame_bytes % 4)
    throw std::invalid_argument("host_env_ingest: bad E / F / frame_bytes");
  if (e0 < 0 || n < 1 || (int64_t)e0 + n > p.E)
    throw std::invalid_argument("host_env_ingest: env range [" + std::to_string(e0) + ", " +
                                std::to_string((int64_t)e0 + n) + ") outside [0, " + std::to_string(p.E) + ")");
  if ((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(frames)) & 3)
    throw std::invalid_argument("host_env_ingest: raw and frames must be 4-byte aligned");
  const int band = band_rows(p.H), rw = region_words(p.H, p.W);
  const size_t lds = (size_t)((2 * rw + 1) / 2) * 8 + (size_t)kBand * p.W * 8 + kOut * kBand;
  if (lds > (size_t)kMaxLds) throw std::invalid_argument("host_env_ingest: frame too large for the LDS stage");
  host_env_ingest_k<<<dim3(n, kOut / kBand), 256, lds, s>>>(raw, reward_in, done_in, rows, cols, frames, p,
                                                            step_counter, reset ? 1 : 0, band, rw, e0, reward, done,
                                                            new_frame, hist, acc, ep_log);
  LAUNCH_CHECK();
}

void host_env_ingest(const uint8_t* raw, const float* reward_in, const float* done_in, const HostEnvTaps& rows,
                     const HostEnvTaps& cols, uint8_t* frames, const HostEnvParams& p, const int64_t* step_counter,
                     bool reset, float* reward, float* done, int* new_frame, int* hist, float* acc, float* ep_log,
                     hipStream_t s) {
  host_env_ingest_range(raw, reward_in, done_in, rows, cols, frames, p, step_counter, reset, reward, done, new_frame,
                        hist, acc, ep_log, 0, p.E, s);
}

}  // namespace apex
