// HBM pattern test: complementary pseudo-random patterns written over a region and read back
// bit-exactly, 16-byte accesses, kHbmUnroll of them in flight per lane; and the pattern pass every
// user of these kernels enqueues (the claim probe, the xGMI checks, the sweep).
#pragma once

#include <algorithm>
#include <cstdint>

#include "options.h"  // kHbmPattern, kMaxPatterns
#include "report.h"   // HbmResult
#include "types.h"

namespace {

// ------------------------------------------------------------------ HBM pattern test
__host__ __device__ __forceinline__ uint32_t pattern_word(uint64_t idx, uint32_t seed) {
  // Cheap invertible mix of the word index: distinct per address, dense in both bit values.
  uint32_t x = static_cast<uint32_t>(idx) * 0x9E3779B1u ^ static_cast<uint32_t>(idx >> 32) * 0x85EBCA77u;
  x ^= seed;
  x ^= x >> 15;
  x *= 0x2C1B3C6Du;
  x ^= x >> 12;
  return x;
}

// Pattern of one 16-byte chunk. kPat 0: an independent mix per 32-bit word (3 integer multiplies
// per word; v_mul_lo_u32 is quarter rate, so 12 of them per 16 B). kPat 1: one multiply per 16 B —
// a bijective mix of the chunk index, its 4 words byte rotations of it XOR fixed masks. Both keep
// every chunk distinct from every other (an aliased address line reads another chunk's pattern)
// and both bit values dense; the complementary pass (flip) drives every bit to 0 and 1 either way.
// __host__ too: the host-link phase recomputes a sample of the pattern on the CPU (hostlink.h).
template <int kPat>
__host__ __device__ __forceinline__ u32x4 pattern16(uint64_t i16, uint32_t seed, uint32_t flip) {
  u32x4 v;
  if constexpr (kPat == 0) {
    uint64_t w = i16 * 4;
    v.x = pattern_word(w, seed) ^ flip;
    v.y = pattern_word(w + 1, seed) ^ flip;
    v.z = pattern_word(w + 2, seed) ^ flip;
    v.w = pattern_word(w + 3, seed) ^ flip;
  } else {
    uint32_t h = (static_cast<uint32_t>(i16) ^ seed) * 0x9E3779B1u;
    h ^= __builtin_rotateleft32(static_cast<uint32_t>(i16 >> 32), 7);
    h ^= h >> 15;
    v.x = h ^ flip;
    v.y = __builtin_rotateleft32(h, 8) ^ 0xA5A5A5A5u ^ flip;
    v.z = __builtin_rotateleft32(h, 16) ^ 0x3C96C396u ^ flip;
    v.w = __builtin_rotateleft32(h, 24) ^ 0x5A0FF05Au ^ flip;
  }
  return v;
}
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

constexpr int kHbmThreads = 256;
constexpr int kHbmUnroll = 4;

// Layouts (probe option "hbmLayout", in-process A/B): 0 grid-stride — each unrolled access of a
// thread is a whole grid (MiBs) apart; 1 tiled — a workgroup's kHbmUnroll accesses per iteration
// cover one contiguous 16 KiB tile (more row-buffer locality per workgroup).
constexpr uint64_t kHbmTile = static_cast<uint64_t>(kHbmThreads) * kHbmUnroll;  // 16-B vectors

// Resets the first ``nreset`` result-counter pairs [bad bits = 0, first bad = all-ones] from block
// 0 on its way (null/0: none), so the claim-time probe enqueues no memsets ahead of its first fill.
__device__ __forceinline__ void reset_pairs(unsigned long long* __restrict__ cnt, int nreset) {
  if (blockIdx.x == 0 && static_cast<int>(threadIdx.x) < 2 * nreset)
    cnt[threadIdx.x] = (threadIdx.x & 1) ? ~0ull : 0ull;
}

template <int kPat = kHbmPattern, int kLayout = 0>
__global__ __launch_bounds__(kHbmThreads) void hbm_fill(u32x4* __restrict__ p, uint64_t n16,
                                                        uint32_t seed, uint32_t flip,
                                                        unsigned long long* __restrict__ reset, int nreset) {
  reset_pairs(reset, nreset);
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kHbmThreads;
  if constexpr (kLayout == 1) {
    const uint64_t tiles = n16 / kHbmTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
      const uint64_t base = t * kHbmTile + threadIdx.x;
#pragma unroll
      for (int u = 0; u < kHbmUnroll; ++u) {
        const uint64_t j = base + static_cast<uint64_t>(u) * kHbmThreads;
        __builtin_nontemporal_store(pattern16<kPat>(j, seed, flip), &p[j]);
      }
    }
    for (uint64_t i = tiles * kHbmTile + static_cast<uint64_t>(blockIdx.x) * kHbmThreads + threadIdx.x; i < n16;
         i += stride)
      __builtin_nontemporal_store(pattern16<kPat>(i, seed, flip), &p[i]);
    return;
  }
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * kHbmThreads + threadIdx.x;
  for (; i + (kHbmUnroll - 1) * stride < n16; i += kHbmUnroll * stride) {
#pragma unroll
    for (int u = 0; u < kHbmUnroll; ++u) {
      uint64_t j = i + u * stride;
      __builtin_nontemporal_store(pattern16<kPat>(j, seed, flip), &p[j]);
    }
  }
  for (; i < n16; i += stride) __builtin_nontemporal_store(pattern16<kPat>(i, seed, flip), &p[i]);
}

__device__ __forceinline__ uint32_t mismatches16(u32x4 v, u32x4 e) {
  return __builtin_popcount(v.x ^ e.x) + __builtin_popcount(v.y ^ e.y) +
         __builtin_popcount(v.z ^ e.z) + __builtin_popcount(v.w ^ e.w);
}

// Counts flipped BITS; records the lowest faulting 16-byte index. One atomic per wave.
template <int kPat = kHbmPattern, int kLayout = 0>
__global__ __launch_bounds__(kHbmThreads) void hbm_verify(const u32x4* __restrict__ p, uint64_t n16,
                                                          uint32_t seed, uint32_t flip,
                                                          unsigned long long* __restrict__ bad_bits,
                                                          unsigned long long* __restrict__ first_bad) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kHbmThreads;
  uint32_t bad = 0;
  uint64_t first = ~0ull;
  auto check = [&](u32x4 v, uint64_t j) {
    uint32_t m = mismatches16(v, pattern16<kPat>(j, seed, flip));
    if (m) {
      bad += m;
      first = umin64(first, j);
    }
  };
  if constexpr (kLayout == 1) {
    const uint64_t tiles = n16 / kHbmTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
      const uint64_t base = t * kHbmTile + threadIdx.x;
      u32x4 v[kHbmUnroll];
#pragma unroll
      for (int u = 0; u < kHbmUnroll; ++u) v[u] = __builtin_nontemporal_load(&p[base + static_cast<uint64_t>(u) * kHbmThreads]);
#pragma unroll
      for (int u = 0; u < kHbmUnroll; ++u) check(v[u], base + static_cast<uint64_t>(u) * kHbmThreads);
    }
    for (uint64_t i = tiles * kHbmTile + static_cast<uint64_t>(blockIdx.x) * kHbmThreads + threadIdx.x; i < n16;
         i += stride)
      check(__builtin_nontemporal_load(&p[i]), i);
  } else {
    uint64_t i = static_cast<uint64_t>(blockIdx.x) * kHbmThreads + threadIdx.x;
    for (; i + (kHbmUnroll - 1) * stride < n16; i += kHbmUnroll * stride) {
      u32x4 v[kHbmUnroll];
#pragma unroll
      for (int u = 0; u < kHbmUnroll; ++u) v[u] = __builtin_nontemporal_load(&p[i + u * stride]);
#pragma unroll
      for (int u = 0; u < kHbmUnroll; ++u) check(v[u], i + u * stride);
    }
    for (; i < n16; i += stride) check(__builtin_nontemporal_load(&p[i]), i);
  }
  // wave64 reduction
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bad += __shfl_xor(bad, off, 64);
    first = umin64(first, static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(first), off, 64)));
  }
  if ((threadIdx.x & 63) == 0 && bad) {
    atomicAdd(bad_bits, static_cast<unsigned long long>(bad));
    atomicMin(first_bad, static_cast<unsigned long long>(first));
  }
}
// ---- fault injection (test hooks: prove the checkers catch corruption on real hardware)
// Flips bit (i % 32) of word i*stride for i < count: distinct words, so exactly ``count`` bits.
__global__ void inject_bit_flips(unsigned int* __restrict__ p, uint64_t nwords, int count) {
  const uint64_t stride = nwords / static_cast<uint64_t>(count + 1);
  for (int i = threadIdx.x; i < count; i += blockDim.x) p[static_cast<uint64_t>(i + 1) * stride] ^= 1u << (i % 32);
}

// ------------------------------------------------------------------ host side: the pattern pass
static_assert(2 * kMaxPatterns <= kHbmThreads, "hbm_fill resets the HBM pairs from one block");

// Workgroups of an HBM kernel: ``per_cu`` per CU, never more than the region has blocks of work.
inline int hbm_grid(int cus, long long per_cu, uint64_t n16) {
  return static_cast<int>(std::min<uint64_t>(static_cast<uint64_t>(cus) * static_cast<uint64_t>(per_cu),
                                             (n16 + kHbmThreads - 1) / kHbmThreads));
}

// Counter pairs [flipped bits, first bad 16-B index] reset by memsets (the claim probe's default is
// the fill kernel's own reset_pairs): ``zero_words`` words to 0, then each pair's second to all-ones.
inline void memset_pairs(hipStream_t s, unsigned long long* cnt, int zero_words, int npairs) {
  PROBE_CHECK(hipMemsetAsync(cnt, 0, zero_words * sizeof(unsigned long long), s));
  for (int pi = 0; pi < npairs; ++pi)
    PROBE_CHECK(hipMemsetAsync(cnt + 2 * pi + 1, 0xFF, sizeof(unsigned long long), s));
}

// One region under test on one stream. Pass ``pi`` writes and checks the pattern of ``seed`` in
// polarity pi & 1 (complementary on odd passes); the caller orders fills, hooks, verifies and
// events on the stream.
struct PatternPass {
  hipStream_t s = nullptr;
  u32x4* buf = nullptr;
  uint64_t n16 = 0;
  uint32_t seed = 0;
  int fill_grid = 1, verify_grid = 1;
  bool cheap = kHbmPattern == 1, tiled = false;  // "hbmPattern", "hbmLayout" (in-process A/B)

  static uint32_t flip_of(int pi) { return (pi & 1) ? 0xFFFFFFFFu : 0u; }

  // ``reset``: the fill also resets the first ``nreset`` counter pairs there.
  void fill(int pi, unsigned long long* reset = nullptr, int nreset = 0) const {
    const dim3 grid(fill_grid), block(kHbmThreads);
    if (tiled) hipLaunchKernelGGL((hbm_fill<1, 1>), grid, block, 0, s, buf, n16, seed, flip_of(pi), reset, nreset);
    else if (cheap) hipLaunchKernelGGL(hbm_fill<1>, grid, block, 0, s, buf, n16, seed, flip_of(pi), reset, nreset);
    else hipLaunchKernelGGL(hbm_fill<0>, grid, block, 0, s, buf, n16, seed, flip_of(pi), reset, nreset);
  }

  void verify(int pi, unsigned long long* pair) const {
    const dim3 grid(verify_grid), block(kHbmThreads);
    const u32x4* p = buf;
    if (tiled) hipLaunchKernelGGL((hbm_verify<1, 1>), grid, block, 0, s, p, n16, seed, flip_of(pi), pair, pair + 1);
    else if (cheap) hipLaunchKernelGGL(hbm_verify<1>, grid, block, 0, s, p, n16, seed, flip_of(pi), pair, pair + 1);
    else hipLaunchKernelGGL(hbm_verify<0>, grid, block, 0, s, p, n16, seed, flip_of(pi), pair, pair + 1);
  }

  // test hooks: ``count`` single-bit flips spread over the region / bit 0 of one chunk
  void inject_flips(int count) const {
    hipLaunchKernelGGL(inject_bit_flips, dim3(1), dim3(256), 0, s, reinterpret_cast<unsigned int*>(buf), n16 * 4, count);
  }
  void inject_flip_at(uint64_t chunk) const {
    // inject_bit_flips on the words from the chunk on, with a stride of 0 words: flips bit 0 of p[0]
    hipLaunchKernelGGL(inject_bit_flips, dim3(1), dim3(256), 0, s, reinterpret_cast<unsigned int*>(buf + chunk),
                       uint64_t{0}, 1);
  }
};

// The counters of ``patterns`` passes, copied back: all flipped bits, the lowest bad chunk.
inline void fold_pairs(const unsigned long long* pairs, int patterns, HbmResult* r) {
  for (int pi = 0; pi < patterns; ++pi) {
    r->bad_bits += pairs[2 * pi];
    r->first_bad = std::min(r->first_bad, pairs[2 * pi + 1]);
  }
}

// ...and their times: ev[0] before the first write, ev[1 + 2 pi] after pass pi's write, ev[2 + 2 pi]
// after its verify. After the stream's synchronise.
inline HbmResult fold_passes(const hipEvent_t* ev, const unsigned long long* pairs, int patterns, uint64_t n16) {
  HbmResult r;
  r.n16 = n16;
  r.patterns = patterns;
  for (int pi = 0; pi < patterns; ++pi) {
    float w, rd;
    PROBE_CHECK(hipEventElapsedTime(&w, ev[2 * pi], ev[1 + 2 * pi]));
    PROBE_CHECK(hipEventElapsedTime(&rd, ev[1 + 2 * pi], ev[2 + 2 * pi]));
    r.write_ms += w;
    r.read_ms += rd;
  }
  fold_pairs(pairs, patterns, &r);
  return r;
}

}  // namespace
