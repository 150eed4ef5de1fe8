// NoisyNet heads for the MLP dueling DQN of the vector engines (gfx950): the factorised-Gaussian noise of
// model.py's NoisyLinear on advantage.{0,2} and value.{0,2}, kept OUT of the forward and backward kernels.
//
// NoisyLinear draws one noise sample per forward, shared over the batch, so the layer is F.linear(x, mu +
// sigma * eps): every existing launch (vec_* / vecw_* / vecwb_* / vect_* / vectb_*) runs unchanged over an
// "effective" plain parameter set, and two small launches per SGD step do the rest:
//
//   vecn_compose  noise reset + effective weights of 1..3 nets (online, target, acting) in one launch.  A
//                 workgroup owns a band of 8 output rows of one noisy layer of one net: threads 0..127 draw the
//                 layer's eps_in[128], threads 128..135 the band's eps_out, threads 136..143 the band's bias
//                 draws (each value drawn by exactly one thread of the group), all into LDS; then the 8 x 128
//                 band is one 16-byte column group per thread: weight_epsilon = eps_out * eps_in (the model's
//                 buffer, the record of the noise in use) and W_eff = fmaf(sigma, eps, mu).  The Philox key is
//                 (seed, net, layer, kind, index, step counter + ahead): a replayed graph draws new noise every
//                 step from the device counter alone.  features.0 is copied by workgroups of 4096 floats.
//                 Mode 2 re-composes from the noise in the buffers (after a target sync), mode 0 writes W_eff =
//                 mu (greedy evaluation).
//   vecn_grad     the flat gradient over the effective layout -> the master layout, same bands: d mu = g,
//                 d sigma = g * eps, features.0 passed through, + one fp64 sum-of-squares partial of the MASTER
//                 gradient per workgroup (wave butterfly, then the four waves in a fixed order): the norm the
//                 optimizer clips by is the noisy net's, not the effective set's.
//
// The flat layouts put value.0 behind advantage.2's A-row tensors, so a tensor's base is 16-byte aligned only
// for some A: each workgroup checks its own four pointers once (uniform) and takes the 16-byte or the scalar
// form of the same loads and stores.
#include "common.h"
#include "kernels.h"

namespace apex {

namespace {

constexpr int kH = kVecHidden;      // 128: every noisy layer's input width
constexpr int kT = 256;             // 8 rows x 32 column groups of 4
constexpr int kCopy = 4 * 4 * kT;   // features.0 floats per copy workgroup (4 x 16 bytes per thread)
static_assert(kVecnBand * (kH / 4) == kT, "one 16-byte column group per thread and band");

// offsets (floats) of the tensors in the effective and the master layouts
struct Lay {
  int64_t n0;                                    // features.0: weight + bias, leading both layouts
  int out[kVecnLayers];
  int64_t ew[kVecnLayers], eb[kVecnLayers];      // effective: weight, bias
  int64_t mu[kVecnLayers], sg[kVecnLayers];      // master: weight_mu, weight_sigma
  int64_t bm[kVecnLayers], bs[kVecnLayers];      // master: bias_mu, bias_sigma
  int nf;                                        // features.0 copy workgroups
  int first[kVecnLayers + 1];                    // first workgroup of each layer's bands; [4] = the count
};

__host__ __device__ __forceinline__ Lay make_lay(int obs, int A) {
  Lay L;
  L.n0 = (int64_t)kH * obs + kH;
  L.out[0] = kH; L.out[1] = A; L.out[2] = kH; L.out[3] = 1;
  int64_t e = L.n0, m = L.n0;
  L.nf = (int)((L.n0 + kCopy - 1) / kCopy);
  int b = L.nf;
  for (int l = 0; l < kVecnLayers; ++l) {
    const int64_t nw = (int64_t)L.out[l] * kH;
    L.ew[l] = e; L.eb[l] = e + nw; e += nw + L.out[l];
    L.mu[l] = m; L.sg[l] = m + nw; L.bm[l] = m + 2 * nw; L.bs[l] = L.bm[l] + L.out[l]; m += 2 * nw + 2 * L.out[l];
    L.first[l] = b;
    b += (L.out[l] + kVecnBand - 1) / kVecnBand;
  }
  L.first[kVecnLayers] = b;
  return L;
}

__device__ __forceinline__ float4 ld4(const float* p, bool v16) {
  if (v16) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void st4(float* p, float4 v, bool v16) {
  if (v16) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
}
__device__ __forceinline__ bool al16(const void* a, const void* b, const void* c, const void* d) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}
// the layer whose bands hold workgroup bid (bid >= L.nf)
__device__ __forceinline__ int layer_of(const Lay& L, int bid) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < kVecnLayers; ++k) l += bid >= L.first[k];
  return l;
}

__global__ __launch_bounds__(kT) void vecn_compose_k(VecnCompose c) {
  __shared__ float s_in[kH];
  __shared__ float s_out[kVecnBand];
  const Lay L = make_lay(c.obs, c.A);
  const int nper = L.first[kVecnLayers];
  const int ni = (int)blockIdx.x / nper, bid = (int)blockIdx.x - ni * nper, t = threadIdx.x;
  const VecnSet& S = c.set[ni];
  if (bid < L.nf) {  // features.0: both flat buffers start 16-byte aligned (checked by the launcher), n0 % 4 == 0
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = (int64_t)bid * kCopy + (int64_t)(k * kT + t) * 4;
      if (i < L.n0) *reinterpret_cast<float4*>(S.eff + i) = *reinterpret_cast<const float4*>(S.master + i);
    }
    return;
  }
  const int l = layer_of(L, bid), out = L.out[l], r0 = (bid - L.first[l]) * kVecnBand;
  const float *wmu = S.master + L.mu[l], *wsg = S.master + L.sg[l], *bmu = S.master + L.bm[l], *bsg = S.master + L.bs[l];
  float *weff = S.eff + L.ew[l], *beff = S.eff + L.eb[l];
  float *weps = S.weps[l], *beps = S.beps[l];
  const int mode = c.mode;
  const int rb = r0 + (t & (kVecnBand - 1));   // the row of a draw / bias thread
  const bool bias_thread = t >= kH + kVecnBand && t < kH + 2 * kVecnBand && rb < out;
  if (mode == 1) {
    const uint64_t ctr = (uint64_t)(c.step[0] + c.ahead);
    const int key = (S.net << 8) | l;
    if (t < kH) {
      s_in[t] = scaled_noise(c.seed, key, 1, t, ctr);
    } else if (t < kH + kVecnBand) {
      if (rb < out) s_out[t - kH] = scaled_noise(c.seed, key, 0, rb, ctr);
    } else if (bias_thread) {
      const float e = scaled_noise(c.seed, key, 2, rb, ctr);
      beps[rb] = e;
      beff[rb] = fmaf(bsg[rb], e, bmu[rb]);
    }
    __syncthreads();   // (mode is launch-uniform)
  } else if (bias_thread) {
    beff[rb] = mode == 2 ? fmaf(bsg[rb], beps[rb], bmu[rb]) : bmu[rb];
  }
  const int rl = t >> 5, row = r0 + rl, c4 = (t & 31) * 4;
  if (row >= out) return;
  const int64_t o = (int64_t)row * kH + c4;
  const bool v16 = al16(wmu, wsg, weff, mode ? weps : nullptr);
  const float4 m = ld4(wmu + o, v16);
  if (mode == 0) {
    st4(weff + o, m, v16);
    return;
  }
  const float4 sg = ld4(wsg + o, v16);
  float4 e;
  if (mode == 1) {
    const float eo = s_out[rl];
    e = make_float4(eo * s_in[c4], eo * s_in[c4 + 1], eo * s_in[c4 + 2], eo * s_in[c4 + 3]);
    st4(weps + o, e, v16);
  } else {
    e = ld4(weps + o, v16);
  }
  st4(weff + o, make_float4(fmaf(sg.x, e.x, m.x), fmaf(sg.y, e.y, m.y), fmaf(sg.z, e.z, m.z), fmaf(sg.w, e.w, m.w)),
      v16);
}

__device__ __forceinline__ double sq(float v) { return (double)v * (double)v; }

__global__ __launch_bounds__(kT) void vecn_grad_k(VecnGrad G) {
  __shared__ double red[kT / 64];
  const Lay L = make_lay(G.obs, G.A);
  const int bid = blockIdx.x, t = threadIdx.x;
  double acc = 0.0;
  if (bid < L.nf) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = (int64_t)bid * kCopy + (int64_t)(k * kT + t) * 4;
      if (i < L.n0) {
        const float4 g = *reinterpret_cast<const float4*>(G.g_eff + i);
        *reinterpret_cast<float4*>(G.g_master + i) = g;
        acc += (sq(g.x) + sq(g.y)) + (sq(g.z) + sq(g.w));
      }
    }
  } else {
    const int l = layer_of(L, bid), out = L.out[l], r0 = (bid - L.first[l]) * kVecnBand;
    const float *gw = G.g_eff + L.ew[l], *weps = G.weps[l];
    float *dmu = G.g_master + L.mu[l], *dsg = G.g_master + L.sg[l];
    const int row = r0 + (t >> 5), c4 = (t & 31) * 4;
    if (row < out) {
      const int64_t o = (int64_t)row * kH + c4;
      const bool v16 = al16(gw, weps, dmu, dsg);
      const float4 g = ld4(gw + o, v16), e = ld4(weps + o, v16);
      const float4 d = make_float4(g.x * e.x, g.y * e.y, g.z * e.z, g.w * e.w);
      st4(dmu + o, g, v16);
      st4(dsg + o, d, v16);
      acc += ((sq(g.x) + sq(g.y)) + (sq(g.z) + sq(g.w))) + ((sq(d.x) + sq(d.y)) + (sq(d.z) + sq(d.w)));
    }
    if (t < kVecnBand && r0 + t < out) {   // the band's biases
      const int r = r0 + t;
      const float g = G.g_eff[L.eb[l] + r], d = g * G.beps[l][r];
      G.g_master[L.bm[l] + r] = g;
      G.g_master[L.bs[l] + r] = d;
      acc += sq(g) + sq(d);
    }
  }
  acc = wave_sum(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) G.part[bid] = (red[0] + red[1]) + (red[2] + red[3]);
}

void check_shape(int obs, int A, const char* who) {
  if (obs < 1 || obs > kVecTallMaxObs || A < 1 || A > kVecWideMaxA)
    throw std::invalid_argument(std::string(who) + ": obs in [1, 1024] and actions in [1, 32]");
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

int64_t vecn_param_count(int obs, int A) {
  check_shape(obs, A, "vecn_param_count");
  const Lay L = make_lay(obs, A);
  return L.bs[kVecnLayers - 1] + L.out[kVecnLayers - 1];
}

int vecn_blocks(int obs, int A) {
  check_shape(obs, A, "vecn_blocks");
  return make_lay(obs, A).first[kVecnLayers];
}

void vecn_compose(const VecnCompose& c, hipStream_t s) {
  check_shape(c.obs, c.A, "vecn_compose");
  if (c.n_nets < 1 || c.n_nets > kVecnMaxNets) throw std::invalid_argument("vecn_compose: one to three nets");
  if (c.mode < 0 || c.mode > 2) throw std::invalid_argument("vecn_compose: mode 0 (mu), 1 (draw) or 2 (keep)");
  if (c.mode == 1 && (!c.step || c.ahead < 0)) throw std::invalid_argument("vecn_compose: the draw needs the step counter");
  for (int i = 0; i < c.n_nets; ++i) {
    const VecnSet& S = c.set[i];
    if (!S.master || !S.eff || misaligned(S.master) || misaligned(S.eff))
      throw std::invalid_argument("vecn_compose: master and effective buffers, 16-byte aligned");
    if (S.net < 0 || S.net > 255) throw std::invalid_argument("vecn_compose: net id in [0, 255]");
    for (int l = 0; l < kVecnLayers && c.mode != 0; ++l)
      if (!S.weps[l] || !S.beps[l]) throw std::invalid_argument("vecn_compose: missing epsilon buffer");
    for (int j = 0; j < i; ++j)
      if (c.set[j].eff == S.eff) throw std::invalid_argument("vecn_compose: two nets share an effective buffer");
  }
  vecn_compose_k<<<vecn_blocks(c.obs, c.A) * c.n_nets, kT, 0, s>>>(c);
  LAUNCH_CHECK();
}

void vecn_grad(const VecnGrad& g, hipStream_t s) {
  check_shape(g.obs, g.A, "vecn_grad");
  if (!g.g_eff || !g.g_master || !g.part || misaligned(g.g_eff) || misaligned(g.g_master))
    throw std::invalid_argument("vecn_grad: gradients (16-byte aligned) and partials");
  for (int l = 0; l < kVecnLayers; ++l)
    if (!g.weps[l] || !g.beps[l]) throw std::invalid_argument("vecn_grad: missing epsilon buffer");
  vecn_grad_k<<<vecn_blocks(g.obs, g.A), kT, 0, s>>>(g);
  LAUNCH_CHECK();
}

}  // namespace apex
