// Host-link (PCIe) phase of the probe, opt-in with "hostLinkBytes": the GPU writes the HBM test's
// address-dependent pattern into pinned host memory over the link (device -> host), reads it back
// over the link (host -> device) and verifies every bit, in both polarities. Included by probe.hip
// after the HBM kernels, whose pattern16<kHbmPattern>, mismatches16, umin64 and reset_pairs it shares.
//
// Shaped for the link, not for HBM: the link moves ~63 GB/s per direction (Gen5 x16) with
// microseconds of latency, a hundredth of what hbm_fill / hbm_verify are laid out for, and the phase
// runs beside the HBM and MFMA phases, whose CUs it must not take. So the grid is a handful of
// workgroups, each walking contiguous tiles of kThreads * kUnroll 16-byte chunks: one wave
// instruction covers 64 consecutive chunks = 1 KiB of contiguous link payload, and every lane keeps
// kUnroll independent 16-byte accesses in flight to cover the link's latency.
#pragma once

namespace hostlink {

constexpr int kThreads = 256;
// Grid, unroll, temporal / non-temporal access and coherent (fine-grained) / default pinned memory:
// the probe options "hostLinkGrid", "hostLinkUnroll" (4 | 8 | 16), "hostLinkNT", "hostLinkCoherent"
// select per run for the sweep of scripts/hostlink_rates.py. Measured on the MI355X at 64 MiB, alone
// on the GPU, p50 GB/s write / read (profiles/hostlink_rates.json; PCIe Gen5 x16, 63 GB/s spec):
//   * grid: the read needs 16 workgroups to fill the link — 2: 14.0, 4: 28.0, 8: 50.0, 16: 57.2,
//     32: 55.3, 64..256: 56.2-57.1 (unroll 8); the write is at 53-56 from 2 workgroups on. 16
//     workgroups are all the phase takes from the HBM and MFMA phases beside it.
//   * unroll 4 / 8 / 16 at grid 16: 55.7 / 56.1 / 56.2 write, 57.3 / 57.2 / 57.1 read: flat. 8 keeps
//     128 B per lane in flight; at grid 8 only unroll 4 still reads at 57.2 (8: 50.0, 16: 48.5).
//   * temporal stores write 56.1 vs 55.0 non-temporal (56.2 vs 53.8 in an earlier run of the same
//     sweep); loads are the same either way (57.18 vs 57.20). The opposite of the HBM kernels'
//     choice: the data leaves the device whatever the hint says.
//   * coherent (fine-grained) vs default pinned memory: 56.13 / 57.18 vs 56.07 / 57.17, no
//     difference, and no configuration exceeded the link's rate (nothing is served from a cache).
//     Coherent is kept: the host's sample and the flip hook then need no cache maintenance.
// By size at these defaults: 1 MiB 45.2 / 44.3, 4 MiB 51.0 / 53.5, 16 MiB 53.1 / 56.3, 64 MiB
// 56.1 / 57.2, 256 MiB 56.8 / 57.4; run-to-run spread under 0.2 GB/s from 8 MiB up.
constexpr int kGrid = 16;
constexpr int kUnroll = 8;
constexpr bool kNonTemporal = false;
constexpr bool kCoherent = true;
constexpr int kMaxGrid = 1024;

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

// What one run of the phase does (options of mi355x_probe_run / mi355x_probe_host_link).
struct Plan {
  uint64_t n16 = 0;
  int patterns = 2;
  uint32_t seed = 0;
  long long inject_chunk = -1;  // test hook "injectHostLinkFlipAtChunk"
  bool preload = false;         // no write pass: verify what the caller loaded, polarity 0
  int grid = kGrid, unroll = kUnroll;
  bool nt = kNonTemporal, coherent = kCoherent;
  double alloc_ms = 0;
};

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

}  // namespace hostlink
