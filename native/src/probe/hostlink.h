// Host-link (PCIe) phase of the probe, opt-in with "hostLinkBytes": the GPU writes the HBM test's
// address-dependent pattern into pinned host memory over the link (device -> host), reads it back
// over the link (host -> device) and verifies every bit, in both polarities. Shares the HBM test's
// pattern16<kHbmPattern>, mismatches16, umin64 and reset_pairs (hbm.h) and the fold of its passes.
//
// Shaped for the link, not for HBM: the link moves ~63 GB/s per direction (Gen5 x16) with
// microseconds of latency, a hundredth of what hbm_fill / hbm_verify are laid out for, and the phase
// runs beside the HBM and MFMA phases, whose CUs it must not take. So the grid is a handful of
// workgroups, each walking contiguous tiles of kThreads * kUnroll 16-byte chunks: one wave
// instruction covers 64 consecutive chunks = 1 KiB of contiguous link payload, and every lane keeps
// kUnroll independent 16-byte accesses in flight to cover the link's latency.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>

#include "arena.h"    // align4k
#include "ctx.h"      // DeviceCtx: the phase's stream, events, counters and pinned buffer
#include "hbm.h"      // pattern16, mismatches16, umin64, reset_pairs, fold_passes
#include "report.h"   // HostLinkResult
#include "options.h"  // hostlink::Plan and the measured defaults of its options
#include "types.h"

namespace {
namespace hostlink {

constexpr int kThreads = 256;

template <bool kNT>
__device__ __forceinline__ void store16(u32x4* p, u32x4 v) {
  if constexpr (kNT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

template <bool kNT>
__device__ __forceinline__ u32x4 load16(const u32x4* p) {
  if constexpr (kNT) return __builtin_nontemporal_load(p);
  else return *p;
}

// Resets the first ``nreset`` counter pairs on its way, as hbm_fill does (no memset in the phase).
// n16 == 0: only the reset.
template <int kU, bool kNT>
__global__ __launch_bounds__(kThreads) void hostlink_write(u32x4* __restrict__ p, uint64_t n16, uint32_t seed,
                                                           uint32_t flip, unsigned long long* __restrict__ reset,
                                                           int nreset) {
  reset_pairs(reset, nreset);
  constexpr uint64_t kTile = static_cast<uint64_t>(kThreads) * kU;  // 16-B chunks per workgroup tile
  const uint64_t tiles = n16 / kTile;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t base = t * kTile + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const uint64_t j = base + static_cast<uint64_t>(u) * kThreads;
      store16<kNT>(&p[j], pattern16<kHbmPattern>(j, seed, flip));
    }
  }
  for (uint64_t i = tiles * kTile + static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n16;
       i += static_cast<uint64_t>(gridDim.x) * kThreads)
    store16<kNT>(&p[i], pattern16<kHbmPattern>(i, seed, flip));
}

// Reports like hbm_verify: flipped BITS, the lowest faulting 16-byte chunk, one atomic pair per wave.
template <int kU, bool kNT>
__global__ __launch_bounds__(kThreads) void hostlink_verify(const u32x4* __restrict__ p, uint64_t n16, uint32_t seed,
                                                            uint32_t flip, unsigned long long* __restrict__ bad_bits,
                                                            unsigned long long* __restrict__ first_bad) {
  constexpr uint64_t kTile = static_cast<uint64_t>(kThreads) * kU;
  const uint64_t tiles = n16 / kTile;
  uint32_t bad = 0;
  uint64_t first = ~0ull;
  auto check = [&](u32x4 v, uint64_t j) {
    const uint32_t m = mismatches16(v, pattern16<kHbmPattern>(j, seed, flip));
    if (m) {
      bad += m;
      first = umin64(first, j);
    }
  };
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t base = t * kTile + threadIdx.x;
    u32x4 v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) v[u] = load16<kNT>(&p[base + static_cast<uint64_t>(u) * kThreads]);
#pragma unroll
    for (int u = 0; u < kU; ++u) check(v[u], base + static_cast<uint64_t>(u) * kThreads);
  }
  for (uint64_t i = tiles * kTile + static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n16;
       i += static_cast<uint64_t>(gridDim.x) * kThreads)
    check(load16<kNT>(&p[i]), i);
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

inline int grid_for(const Plan& pl) {
  const uint64_t blocks = (pl.n16 + kThreads - 1) / kThreads;
  return static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(static_cast<uint64_t>(pl.grid), blocks)));
}

template <int kU, bool kNT>
void launch_write_as(hipStream_t s, int grid, u32x4* p, uint64_t n16, uint32_t seed, uint32_t flip,
                     unsigned long long* reset, int nreset) {
  hipLaunchKernelGGL((hostlink_write<kU, kNT>), dim3(grid), dim3(kThreads), 0, s, p, n16, seed, flip, reset, nreset);
}

template <int kU, bool kNT>
void launch_verify_as(hipStream_t s, int grid, const u32x4* p, uint64_t n16, uint32_t seed, uint32_t flip,
                      unsigned long long* bad_bits, unsigned long long* first_bad) {
  hipLaunchKernelGGL((hostlink_verify<kU, kNT>), dim3(grid), dim3(kThreads), 0, s, p, n16, seed, flip, bad_bits,
                     first_bad);
}

// An unroll that is not 4 or 16 runs the 8-deep kernels.
inline void launch_write(hipStream_t s, const Plan& pl, u32x4* p, uint64_t n16, uint32_t flip, unsigned long long* reset,
                         int nreset) {
  const int g = grid_for(pl);
  if (pl.unroll == 4)
    pl.nt ? launch_write_as<4, true>(s, g, p, n16, pl.seed, flip, reset, nreset)
          : launch_write_as<4, false>(s, g, p, n16, pl.seed, flip, reset, nreset);
  else if (pl.unroll == 16)
    pl.nt ? launch_write_as<16, true>(s, g, p, n16, pl.seed, flip, reset, nreset)
          : launch_write_as<16, false>(s, g, p, n16, pl.seed, flip, reset, nreset);
  else
    pl.nt ? launch_write_as<8, true>(s, g, p, n16, pl.seed, flip, reset, nreset)
          : launch_write_as<8, false>(s, g, p, n16, pl.seed, flip, reset, nreset);
}

inline void launch_verify(hipStream_t s, const Plan& pl, const u32x4* p, uint32_t flip, unsigned long long* bad_bits,
                          unsigned long long* first_bad) {
  const int g = grid_for(pl);
  if (pl.unroll == 4)
    pl.nt ? launch_verify_as<4, true>(s, g, p, pl.n16, pl.seed, flip, bad_bits, first_bad)
          : launch_verify_as<4, false>(s, g, p, pl.n16, pl.seed, flip, bad_bits, first_bad);
  else if (pl.unroll == 16)
    pl.nt ? launch_verify_as<16, true>(s, g, p, pl.n16, pl.seed, flip, bad_bits, first_bad)
          : launch_verify_as<16, false>(s, g, p, pl.n16, pl.seed, flip, bad_bits, first_bad);
  else
    pl.nt ? launch_verify_as<8, true>(s, g, p, pl.n16, pl.seed, flip, bad_bits, first_bad)
          : launch_verify_as<8, false>(s, g, p, pl.n16, pl.seed, flip, bad_bits, first_bad);
}

// ------------------------------------------------------------------ the phase: ensure / launch / finish
constexpr int kSamples = 1024;

// Makes the phase's events, counters and a pinned, device-mapped buffer of at least ``bytes``.
// The only place the buffer is freed or replaced: the caller holds the device's probe lock, and
// every stream a kernel with the old pointer could be on is drained first. Returns the cost of the
// pinned allocation when this call made or grew it, else 0.
inline double ensure(DeviceCtx& c, uint64_t bytes, bool coherent) {
  if (!c.hl_res) {  // set last: a failure half way is picked up by the next probe that asks
    for (auto& e : c.hev)
      if (!e) PROBE_CHECK(hipEventCreate(&e));
    if (!c.hl_cnt)
      PROBE_CHECK(hipMalloc(reinterpret_cast<void**>(&c.hl_cnt), 2 * kMaxPatterns * sizeof(unsigned long long)));
    PROBE_CHECK(hipHostMalloc(reinterpret_cast<void**>(&c.hl_res), 2 * kMaxPatterns * sizeof(unsigned long long)));
  }
  if (c.hl_buf && c.hl_bytes >= bytes && c.hl_coherent == coherent) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  if (c.hl_buf) {
    if (c.hl_stream) PROBE_CHECK(hipStreamSynchronize(c.hl_stream));
    PROBE_CHECK(hipStreamSynchronize(c.stream));
    PROBE_CHECK(hipStreamSynchronize(c.stream2));
    void* old = c.hl_buf;
    c.hl_buf = c.hl_dev = nullptr;
    c.hl_bytes = 0;
    PROBE_CHECK(hipHostFree(old));
  }
  void* host = nullptr;
  void* devp = nullptr;
  const uint64_t cap = align4k(bytes);
  PROBE_CHECK(hipHostMalloc(&host, cap, hipHostMallocMapped | (coherent ? hipHostMallocCoherent : hipHostMallocNonCoherent)));
  if (hipHostGetDevicePointer(&devp, host, 0) != hipSuccess || !devp) {
    (void)hipHostFree(host);
    throw ProbeError("hipHostGetDevicePointer failed for the host-link buffer");
  }
  c.hl_buf = host;
  c.hl_dev = devp;
  c.hl_bytes = cap;
  c.hl_coherent = coherent;
  return ms_since(t0);
}

// Enqueues the phase on stream s: per pass a write (device -> host), an event, a verify (host ->
// device), an event; then the counters' copy. No host synchronise, except for the flip hook.
inline void launch(DeviceCtx& c, hipStream_t s, const Plan& pl) {
  auto* buf = static_cast<u32x4*>(c.hl_dev);
  PROBE_CHECK(hipEventRecord(c.hev[0], s));
  for (int pi = 0; pi < pl.patterns; ++pi) {
    const uint32_t flip = PatternPass::flip_of(pi);
    unsigned long long* reset = pi == 0 ? c.hl_cnt : nullptr;
    // a preload keeps the caller's data: the write kernel only resets the counters (n16 = 0)
    launch_write(s, pl, buf, pl.preload ? 0 : pl.n16, flip, reset, reset ? pl.patterns : 0);
    PROBE_CHECK(hipEventRecord(c.hev[1 + 2 * pi], s));
    if (pi == 0 && pl.inject_chunk >= 0 && static_cast<uint64_t>(pl.inject_chunk) < pl.n16) {
      // test hook: the HOST flips bit 0 of a chunk once the write pass has landed
      PROBE_CHECK(hipStreamSynchronize(s));
      static_cast<volatile uint32_t*>(c.hl_buf)[static_cast<uint64_t>(pl.inject_chunk) * 4] ^= 1u;
      std::atomic_thread_fence(std::memory_order_seq_cst);
    }
    launch_verify(s, pl, buf, flip, c.hl_cnt + 2 * pi, c.hl_cnt + 2 * pi + 1);
    PROBE_CHECK(hipEventRecord(c.hev[2 + 2 * pi], s));
  }
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipMemcpyAsync(c.hl_res, c.hl_cnt, 2 * pl.patterns * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
}

// After the stream's synchronise: the passes' fold and the host's sample of what landed in its DRAM
// (the last pass's pattern at kSamples evenly spaced chunks plus the first and the last: the GPU's
// stores reached host memory, not a device-side cache) -> the "hostLink" block's result.
inline HostLinkResult finish(DeviceCtx& c, const Plan& pl) {
  HostLinkResult r;
  r.passes = fold_passes(c.hev, c.hl_res, pl.patterns, pl.n16);
  r.seed = pl.seed;
  r.preload = pl.preload;
  r.alloc_ms = pl.alloc_ms;
  if (pl.preload) return r;
  const uint32_t flip = PatternPass::flip_of(pl.patterns - 1);
  const auto* host = static_cast<const uint32_t*>(c.hl_buf);
  auto sample = [&](uint64_t j) {
    const u32x4 e = pattern16<kHbmPattern>(j, pl.seed, flip);
    const uint32_t* h = host + j * 4;
    ++r.samples;
    if (h[0] != e.x || h[1] != e.y || h[2] != e.z || h[3] != e.w) ++r.sample_bad;
  };
  if (pl.n16 <= static_cast<uint64_t>(kSamples) + 2) {
    for (uint64_t j = 0; j < pl.n16; ++j) sample(j);
  } else {
    sample(0);
    for (int k = 0; k < kSamples; ++k) sample(1 + (pl.n16 - 2) * static_cast<uint64_t>(k) / kSamples);
    sample(pl.n16 - 1);
  }
  return r;
}

}  // namespace hostlink
}  // namespace
