// Device digest of a contiguous byte range for full-state checkpoints (utils/engine_state.py).
//
// The definition is ``digest_host`` in engine_state.py: the range is read as little-endian
// 64-bit words (the tail zero-padded), word i becomes mix64(word + (i + 1) * kDigestSalt), the
// results are summed modulo 2^64 and mix64(nbytes ^ kDigestLenSalt) is added.  mix64 is the
// splitmix64 finalizer (a bijection: a changed word always changes its term); the index salt
// makes the sum sensitive to position; the sum commutes, so the grid-stride order, the wave
// reduction and the partial combine need no fixed tree.
//
// Words are counted from the base pointer, which may have any alignment (a slice of a u8
// tensor).  The body is read as aligned 16-byte chunks: an aligned base maps chunk j to the
// word pair j directly; otherwise pair j is funnel-shifted out of chunks j and j + 1 of the
// base rounded down to 16 (both hold at least one byte of the range, so both lie inside the
// allocation; the bytes in front of the base are loaded and shifted away).  The last
// nbytes % 16 bytes are read byte by byte.
#include <mutex>
#include <unordered_map>

#include "common.h"
#include "kernels.h"

namespace apex {

namespace {

constexpr uint64_t kDigestSalt = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kDigestLenSalt = 0xD6E8FEB86659FD93ull;
constexpr int kDigestThreads = 256;
constexpr int kDigestUnroll = 4;
constexpr int kDigestMaxBlocks = 2048;  // 8 workgroups per CU

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ uint64_t digest_term(uint64_t word, uint64_t index) {
  return mix64(word + (index + 1) * kDigestSalt);
}

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

// word pair j of the range: chunk j of an aligned base, or bytes [mis, mis + 16) of chunks j, j + 1
__device__ __forceinline__ uint64_t pair_terms(const u32v4* __restrict__ chunks, int64_t j, int mis) {
  const u32v4 a = __builtin_nontemporal_load(chunks + j);
  uint64_t w0 = u64_of(a.x, a.y), w1 = u64_of(a.z, a.w);
  if (mis) {
    const u32v4 b = __builtin_nontemporal_load(chunks + j + 1);
    const uint64_t b0 = u64_of(b.x, b.y), b1 = u64_of(b.z, b.w);
    const uint64_t x = mis < 8 ? w0 : w1, y = mis < 8 ? w1 : b0, z = mis < 8 ? b0 : b1;
    const int sh = (mis & 7) * 8;
    w0 = sh ? (x >> sh) | (y << (64 - sh)) : x;
    w1 = sh ? (y >> sh) | (z << (64 - sh)) : y;
  }
  return digest_term(w0, 2 * (uint64_t)j) + digest_term(w1, 2 * (uint64_t)j + 1);
}

__global__ void __launch_bounds__(kDigestThreads)
state_digest_k(const u32v4* __restrict__ chunks, int mis, int64_t npairs, uint64_t* __restrict__ partials) {
  __shared__ uint64_t wsum[kDigestThreads / APEX_WAVE];
  const int64_t stride = (int64_t)gridDim.x * kDigestThreads;
  int64_t j = (int64_t)blockIdx.x * kDigestThreads + threadIdx.x;
  uint64_t acc = 0;
  for (; j + (kDigestUnroll - 1) * stride < npairs; j += kDigestUnroll * stride) {
    uint64_t t[kDigestUnroll];
#pragma unroll
    for (int u = 0; u < kDigestUnroll; ++u) t[u] = pair_terms(chunks, j + u * stride, mis);
#pragma unroll
    for (int u = 0; u < kDigestUnroll; ++u) acc += t[u];
  }
  for (; j < npairs; j += stride) acc += pair_terms(chunks, j, mis);
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int i = 0; i < kDigestThreads / APEX_WAVE; ++i) t += wsum[i];
    partials[blockIdx.x] = t;
  }
}

// one workgroup: the partials, the byte-wise tail (words 2 * npairs ..) and the length term
__global__ void __launch_bounds__(kDigestThreads)
state_digest_fin_k(const uint64_t* __restrict__ partials, int nparts, const uint8_t* __restrict__ base,
                   int64_t npairs, int64_t nbytes, uint64_t* __restrict__ out) {
  __shared__ uint64_t wsum[kDigestThreads / APEX_WAVE];
  uint64_t acc = 0;
  for (int i = threadIdx.x; i < nparts; i += kDigestThreads) acc += partials[i];
  if (threadIdx.x == 0) {
    const int64_t t0 = npairs * 16;
    const int tail = (int)(nbytes - t0);  // 0..15
    uint64_t w[2] = {0, 0};
    for (int b = 0; b < tail; ++b) w[b >> 3] |= (uint64_t)base[t0 + b] << (8 * (b & 7));
    if (tail > 0) acc += digest_term(w[0], 2 * (uint64_t)npairs);
    if (tail > 8) acc += digest_term(w[1], 2 * (uint64_t)npairs + 1);
    acc += mix64((uint64_t)nbytes ^ kDigestLenSalt);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int i = 0; i < kDigestThreads / APEX_WAVE; ++i) t += wsum[i];
    out[0] = t;
  }
}

// partials + result, allocated once per device and kept: a digest call neither allocates nor
// frees (hipFree waits for the whole device).  The mutex covers the call: one digest at a time.
std::mutex g_scratch_mutex;
std::unordered_map<int, uint64_t*> g_scratch;

uint64_t* digest_scratch() {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  auto it = g_scratch.find(dev);
  if (it != g_scratch.end()) return it->second;
  void* raw = nullptr;
  HIP_CHECK(hipMalloc(&raw, sizeof(uint64_t) * (size_t)(kDigestMaxBlocks + 1)));
  return g_scratch[dev] = static_cast<uint64_t*>(raw);
}

}  // namespace

uint64_t state_digest(const void* ptr, int64_t nbytes, hipStream_t s) {
  if (nbytes < 0 || (!ptr && nbytes)) throw std::invalid_argument("state_digest: bad pointer or size");
  const uintptr_t addr = reinterpret_cast<uintptr_t>(ptr);
  const int mis = (int)(addr & 15);
  const int64_t npairs = nbytes / 16;
  const int64_t want = (npairs + (int64_t)kDigestThreads * kDigestUnroll - 1) / ((int64_t)kDigestThreads * kDigestUnroll);
  const int nblocks = (int)(want < kDigestMaxBlocks ? want : kDigestMaxBlocks);
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  uint64_t* partials = digest_scratch();
  uint64_t* out = partials + kDigestMaxBlocks;
  if (nblocks) {
    state_digest_k<<<nblocks, kDigestThreads, 0, s>>>(reinterpret_cast<const u32v4*>(addr - mis), mis, npairs, partials);
    LAUNCH_CHECK();
  }
  state_digest_fin_k<<<1, kDigestThreads, 0, s>>>(partials, nblocks, static_cast<const uint8_t*>(ptr), npairs, nbytes,
                                                  out);
  LAUNCH_CHECK();
  uint64_t host = 0;
  HIP_CHECK(hipMemcpyAsync(&host, out, sizeof(host), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return host;
}

}  // namespace apex
