// The probe's one device allocation, laid out once: [HBM pattern region | bf16 GEMM operands |
// counters | low-precision counters | low-precision operands]. A probe costs one hipMalloc instead
// of a dozen, and every phase takes its pointers from the same ArenaLayout, so the sizes cannot
// drift apart. Pure host code (no HIP include): native/tests/test_probe_arena.cc checks it.
#pragma once

#include <cstddef>
#include <cstdint>

#include "options.h"  // kMaxPatterns, lowp::kDtypes

namespace {

// The one rounding of every region of the arena.
inline size_t align4k(size_t x) { return (x + 4095) & ~static_cast<size_t>(4095); }

// CU identity keys (census.h): 11 bits, one bit per key in the census / GEMM maps.
constexpr int kCuKeys = 2048, kCuMapWords = kCuKeys / 64;

// device counter / pinned host result slots: 2 per HBM pattern, then the two GEMM check counters
constexpr int kSlotSmall = 2 * kMaxPatterns, kSlotAbft = kSlotSmall + 1, kSlotCensusBad = kSlotAbft + 1,
              kSlotCensusMap = kSlotCensusBad + 1, kSlotGemmMap = kSlotCensusMap + kCuMapWords,
              kResSlots = kSlotGemmMap + kCuMapWords;

namespace lowp {
// Device counters of one dtype: element mismatches, ABFT mismatches, bad census waves, census map.
constexpr int kSlotSmall = 0, kSlotAbft = 1, kSlotCensusBad = 2, kSlotCensusMap = 3, kSlots = kSlotCensusMap + kCuMapWords;
constexpr int kSmallN = 256;

// The operand / C region every asked-for dtype shares (they run one after the other on one stream),
// sized for the largest (8-bit operands); launch_phase_t (lowp.h) carves it in this order.
inline size_t region_bytes(size_t n) {
  const size_t n0 = kSmallN;
  return 2 * align4k(n0 * n0) + 2 * align4k(n0 * n0 / 32) + 2 * align4k(n0 * n0 * 4) + 2 * align4k(n * n) +
         2 * align4k(n * n / 32) + align4k(n * n * 4) + align4k(6 * n * 4);
}
}  // namespace lowp

// Byte offsets from the arena's base. Without the MFMA phase its regions are empty (all at ``cnt``);
// the low-precision counters and region follow the probe's own counters, so a probe that asks for
// no dtype has the arena it always had.
struct ArenaLayout {
  size_t hbm = 0;                        // n16 16-byte chunks of pattern
  size_t a0 = 0, b0 = 0, c0 = 0, r0 = 0;  // 256^3 check: operands, C, VALU reference
  size_t a = 0, b = 0, c = 0, v = 0;     // N^3 GEMM: operands, C, 6 ABFT vectors of N u32
  size_t cnt = 0;                        // kResSlots counters
  size_t lowp_cnt = 0;                   // lowp::kDtypes * lowp::kSlots counters
  size_t lowp_region = 0;                // lowp::region_bytes(gemm_n)
  size_t need = 0;                       // bytes of the whole arena

  static ArenaLayout make(uint64_t n16, int gemm_n, bool do_mfma, int lowp_mask) {
    const size_t n = static_cast<size_t>(gemm_n), n0 = 256;
    ArenaLayout l;
    size_t at = 0;
    auto carve = [&](size_t bytes) {
      const size_t off = at;
      at += align4k(bytes);
      return off;
    };
    l.hbm = carve(static_cast<size_t>(n16) * 16);
    auto gemm = [&](size_t bytes) { return do_mfma ? carve(bytes) : at; };
    l.a0 = gemm(n0 * n0 * 2);
    l.b0 = gemm(n0 * n0 * 2);
    l.c0 = gemm(n0 * n0 * 4);
    l.r0 = gemm(n0 * n0 * 4);
    l.a = gemm(n * n * 2);
    l.b = gemm(n * n * 2);
    l.c = gemm(n * n * 4);
    l.v = gemm(6 * n * 8);
    l.cnt = carve(kResSlots * sizeof(unsigned long long));
    l.lowp_cnt = at;
    if (lowp_mask) {
      carve(lowp::kDtypes * lowp::kSlots * sizeof(unsigned long long));
      l.lowp_region = carve(lowp::region_bytes(n));
    } else {
      l.lowp_region = at;
    }
    l.need = at;
    return l;
  }
};

}  // namespace
