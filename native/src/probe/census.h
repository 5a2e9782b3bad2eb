// CU identity and the per-CU MFMA census: which CUs ran a kernel, and whether each one's matrix
// cores compute.
#pragma once

#include <cstdint>

#include "arena.h"  // kCuKeys, kCuMapWords
#include "types.h"

namespace {

// ------------------------------------------------------------------ CU identity + MFMA census
// The hardware identity of the CU a wave runs on: XCC_ID (which XCD) and HW_ID's SE/SH/CU fields
// (CDNA3/4 ISA "HW_ID": CU_ID [11:8], SH_ID [12], SE_ID [15:13]). Both are read-only hardware
// registers (s_getreg), packed into an 11-bit key (kCuKeys): xcc[10:8] se[7:5] sh[4] cu[3:0].

__device__ __forceinline__ int cu_key() {
  unsigned hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  return static_cast<int>(((xcc & 7u) << 8) | (((hw >> 13) & 7u) << 5) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 15u));
}

// HW_ID.SIMD_ID, bits [5:4] in the same layout: which of the CU's four SIMDs the wave runs on.
__device__ __forceinline__ uint32_t simd_id() {
  unsigned hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  return (hw >> 4) & 3u;
}

__device__ __forceinline__ void mark_cu(unsigned long long* map) {
  const int k = cu_key();
  atomicOr(&map[k >> 6], 1ull << (k & 63));
}

// Every CU must prove its matrix cores: each wave chains ``iters`` v_mfma_f32_16x16x32_bf16 on
// operands A[r][k] = fa(r), B[c][k] = gb(c) (small integers from the runtime seed, so nothing folds
// at compile time) and checks every accumulator against iters * 32 * fa(r) * gb(c), exact in fp32.
// A wave whose result is exact sets its CU's bit; a wrong result counts into ``bad``. The grid is
// several waves per CU slot so the dispatcher places work on every CU of every XCD.
constexpr int kCensusThreads = 256;
__global__ __launch_bounds__(kCensusThreads) void cu_census(unsigned long long* __restrict__ map,
                                                            unsigned long long* __restrict__ bad, int iters,
                                                            uint32_t seed, int fault_xcc) {
  const int lane = threadIdx.x & 63;
  const uint32_t h = seed ^ (blockIdx.x * 0x9E3779B1u);
  const int fa = 1 + static_cast<int>((h + (lane & 15)) & 3);          // row value of this lane's A fragment
  const int gb = 1 + static_cast<int>(((h >> 8) + (lane & 15)) & 3);   // col value of this lane's B fragment
  const short a16 = static_cast<short>(__float_as_uint(static_cast<float>(fa)) >> 16);
  const short b16 = static_cast<short>(__float_as_uint(static_cast<float>(gb)) >> 16);
  bf16x8 av, bv;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    av[j] = a16;
    bv[j] = b16;
  }
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < iters; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
  if (fault_xcc >= 0 && (cu_key() >> 8) == fault_xcc) acc[0] += 1.0f;  // test hook: a "bad" XCD
  // C/D layout of 16x16x32: col = lane&15, row = 4*(lane>>4) + j; fa of row r is held by lane r
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 4 * (lane >> 4) + j;
    const int far = 1 + static_cast<int>((h + r) & 3);
    ok = ok && acc[j] == static_cast<float>(iters * 32 * far * gb);
  }
  const bool wave_ok = __all(ok);
  if (lane == 0) {
    if (wave_ok) mark_cu(map);
    else atomicAdd(bad, 1ull);
  }
}

// A CU map copied back: how many CUs set their bit, in all and per XCD.
struct CuCount {
  int total = 0;
  int per_xcc[8] = {};
};

inline CuCount count_cus(const unsigned long long* map) {
  CuCount c;
  for (int w = 0; w < kCuMapWords; ++w) {
    const int n = __builtin_popcountll(map[w]);
    c.total += n;
    c.per_xcc[(w * 64) >> 8] += n;
  }
  return c;
}

// The two CU maps of a per-CU phase (lds.h, regfile.h, atomics.h) folded: CUs tested, CUs with a
// fault, and the tested ones without, in all and per XCD.
struct CuFold {
  int tested = 0, bad = 0, verified = 0;
  int per_xcd[8] = {};  // verified
};

inline CuFold fold_cus(const unsigned long long* tested, const unsigned long long* bad) {
  unsigned long long verified[kCuMapWords];
  for (int w = 0; w < kCuMapWords; ++w) verified[w] = tested[w] & ~bad[w];
  CuFold f;
  f.tested = count_cus(tested).total;
  f.bad = count_cus(bad).total;
  const CuCount v = count_cus(verified);
  f.verified = v.total;
  for (int x = 0; x < 8; ++x) f.per_xcd[x] = v.per_xcc[x];
  return f;
}

// A dump run's kSlotDumpCu / kSlotDumpSimds (all-ones: no workgroup 0 reported) -> the CU key of the
// dumped workgroup and the SIMD each of its four waves ran on.
inline void decode_dump(unsigned long long cu, unsigned long long simds, int* dump_cu, int* dump_simds) {
  if (cu == ~0ull) return;
  *dump_cu = static_cast<int>(cu);
  for (int w = 0; w < 4; ++w) dump_simds[w] = static_cast<int>((simds >> (8 * w)) & 0xFF);
}

}  // namespace
