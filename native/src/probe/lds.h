// LDS phase of the probe, opt-in with "ldsCheck": every CU's Local Data Share (160 KiB of SRAM) is
// marched in both polarities and address-tested by a workgroup that owns all of it. Shares the HBM
// test's pattern16, mismatches16 and umin64 (hbm.h) and the census's CU identity (census.h).
//
// One kernel, one workgroup of 256 threads per CU at a time: the kernel declares the CU's whole LDS
// statically, so two of its workgroups can never share a CU and "this workgroup tested this CU's
// whole LDS" is a true statement. The grid oversubscribes the CUs ("ldsBlocksPerCU") so that the
// dispatcher visits every one, as the census does; no workgroup waits for another.
//
// What a march finds: a bit stuck at 0 or 1, a bit coupled to a neighbour written later, an address
// line that aliases two chunks (the pattern depends on the chunk index and on the workgroup, so an
// alias reads another chunk's value and the bytes a previous workgroup left are never expected).
// Every verify reads what another wave wrote, so the data crosses SIMDs and the barrier between
// write and read is load-bearing. The address pass repeats the address test at dword granularity
// through the 4-byte store path, in a strided order. What it cannot find: faults that need a
// retention time, the LDS atomics' ALU, the LDS-DMA write path, and anything outside the LDS.
#pragma once

#include <algorithm>
#include <cstdint>

#include "arena.h"    // kCuMapWords
#include "census.h"   // cu_key, fold_cus
#include "ctx.h"      // DeviceCtx, CounterSets: the phase's events, counters and pinned result
#include "hbm.h"      // pattern16, mismatches16, umin64
#include "options.h"  // lds::Plan, lds::kBytesPerCU
#include "report.h"   // LdsResult
#include "types.h"

namespace {
namespace lds {

constexpr int kThreads = 256;
constexpr uint32_t kChunksPerCU = kBytesPerCU / 16;

// One set of counters; two sets, and workgroup 0 of a run resets the OTHER set (ctx.h CounterSets).
constexpr int kSlotBadBits = 0, kSlotFirstBad = 1, kSlotWorkgroups = 2, kSlotDumpCu = 3, kSlotTested = 4,
              kSlotBad = kSlotTested + kCuMapWords, kSlots = kSlotBad + kCuMapWords;
static_assert(kSlots <= kThreads, "workgroup 0 resets a counter set with one store per thread");

__host__ __device__ constexpr unsigned long long reset_value(int slot) {
  return slot == kSlotFirstBad || slot == kSlotDumpCu ? ~0ull : 0ull;
}

struct KernelArgs {
  uint32_t n16;     // tested 16-byte chunks, 1..kChunksPerCU
  uint32_t seed;    // salted
  uint32_t stride;  // of the address pass, coprime to 4 * n16 (lds::stride_for)
  int patterns;
  uint32_t flip_byte, skip_chunk;  // test hooks, out of range: off
  int fault_xcc;                   // test hook: the flip only on this XCD (< 0: on all)
  int dump_stage;                  // 1 | 2 | 3: workgroup 0 copies its LDS to ``dump`` there
  u32x4* dump;
  unsigned long long* cnt;   // this run's counter set
  unsigned long long* next;  // the next run's, reset here
};

// The expected 16 bytes of address-pass chunk j: dword d holds the first word of its own pattern16<1>.
__device__ __forceinline__ u32x4 address_chunk(uint64_t hi, uint32_t j, uint32_t seed) {
  u32x4 e;
  e.x = pattern16<1>(hi | (4 * j), seed, 0).x;
  e.y = pattern16<1>(hi | (4 * j + 1), seed, 0).x;
  e.z = pattern16<1>(hi | (4 * j + 2), seed, 0).x;
  e.w = pattern16<1>(hi | (4 * j + 3), seed, 0).x;
  return e;
}

// Offset of the lowest differing byte of a 16-byte chunk (little-endian words); d != 0 somewhere.
__device__ __forceinline__ uint32_t first_bad_byte(u32x4 d) {
  if (d.x) return static_cast<uint32_t>(__builtin_ctz(d.x)) >> 3;
  if (d.y) return 4 + (static_cast<uint32_t>(__builtin_ctz(d.y)) >> 3);
  if (d.z) return 8 + (static_cast<uint32_t>(__builtin_ctz(d.z)) >> 3);
  return 12 + (static_cast<uint32_t>(__builtin_ctz(d.w)) >> 3);
}

__global__ __launch_bounds__(kThreads) void lds_march(const KernelArgs a) {
  __shared__ u32x4 lds[kChunksPerCU];  // all of the CU's LDS, whatever n16 is
  const uint32_t t = threadIdx.x, b = blockIdx.x, n16 = a.n16;
  if (b == 0 && t < kSlots) a.next[t] = reset_value(static_cast<int>(t));
  const int k = cu_key();  // the same for every wave of the workgroup
  const uint64_t hi = static_cast<uint64_t>(b) << 32;
  uint32_t bad = 0;
  uint64_t first = ~0ull;
  auto check = [&](u32x4 v, u32x4 e, uint32_t j) {
    const uint32_t m = mismatches16(v, e);
    if (m) {
      bad += m;
      first = umin64(first, (static_cast<uint64_t>(k) << 32) | (j * 16 + first_bad_byte(v ^ e)));
    }
  };
  // workgroup 0 copies what it holds to the caller; the barrier keeps the next step's stores out
  auto dump = [&](int stage) {
    if (a.dump_stage != stage || b != 0) return;
    for (uint32_t j = t; j < n16; j += kThreads) a.dump[j] = lds[j];
    __syncthreads();
  };
  const uint32_t up = (t + 64) & (kThreads - 1), down = (t + 128) & (kThreads - 1);

  // ---- march: per polarity, up write / up verify + complement / down verify
  for (int p = 0; p < a.patterns; ++p) {
    const uint32_t flip = (p & 1) ? 0xFFFFFFFFu : 0u;  // as PatternPass::flip_of
    for (uint32_t j = t; j < n16; j += kThreads)
      if (p != 0 || j != a.skip_chunk) lds[j] = pattern16<kHbmPattern>(hi | j, a.seed, flip);
    __syncthreads();
    if (p == 0) {
      // test hook: bit 0 of one byte, by a plain LDS store (uniform: one workgroup is on one CU)
      if (a.flip_byte < n16 * 16 && (a.fault_xcc < 0 || (k >> 8) == a.fault_xcc)) {
        if (t == 0) reinterpret_cast<unsigned char*>(lds)[a.flip_byte] ^= 1;
        __syncthreads();
      }
      dump(1);
    }
    // each thread verifies chunks the next wave wrote, then writes their complement
    for (uint32_t base = 0; base < n16; base += kThreads) {
      const uint32_t j = base + up;
      if (j < n16) {
        check(lds[j], pattern16<kHbmPattern>(hi | j, a.seed, flip), j);
        lds[j] = pattern16<kHbmPattern>(hi | j, a.seed, ~flip);
      }
    }
    __syncthreads();
    if (p == 0) dump(2);
    // ...and, from the top down, the complements a wave further on wrote
    for (uint32_t base = (n16 - 1) / kThreads * kThreads;; base -= kThreads) {
      const uint32_t j = base + down;
      if (j < n16) check(lds[j], pattern16<kHbmPattern>(hi | j, a.seed, ~flip), j);
      if (base == 0) break;
    }
    __syncthreads();
  }

  // ---- address pass: 4-byte stores in strided order, thread t's step i writes dword
  // ((t + 256 i) * S) mod N, kept incrementally; read back linearly, 16 bytes at a time
  {
    // 32-bit products: s < n <= 40960 and t < 256
    const uint32_t n = n16 * 4, s = a.stride % n, step = kThreads * s % n;
    auto* words = reinterpret_cast<uint32_t*>(lds);
    uint32_t d = t * s % n;
    for (uint32_t i = t; i < n; i += kThreads) {
      words[d] = pattern16<1>(hi | d, a.seed + 1, 0).x;
      d += step;
      if (d >= n) d -= n;
    }
    __syncthreads();
    dump(3);
    for (uint32_t j = t; j < n16; j += kThreads) check(lds[j], address_chunk(hi, j, a.seed + 1), j);
  }

  // ---- count: one atomic group per wave, and only when something is bad
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bad += __shfl_xor(bad, off, 64);
    first = umin64(first, static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(first), off, 64)));
  }
  if ((t & 63) == 0 && bad) {
    atomicAdd(&a.cnt[kSlotBadBits], static_cast<unsigned long long>(bad));
    atomicMin(&a.cnt[kSlotFirstBad], static_cast<unsigned long long>(first));
    atomicOr(&a.cnt[kSlotBad + (k >> 6)], 1ull << (k & 63));
  }
  if (t == 0) {
    atomicOr(&a.cnt[kSlotTested + (k >> 6)], 1ull << (k & 63));
    atomicAdd(&a.cnt[kSlotWorkgroups], 1ull);
    if (b == 0 && a.dump_stage) atomicMin(&a.cnt[kSlotDumpCu], static_cast<unsigned long long>(k));
  }
}

// ------------------------------------------------------------------ the phase: ensure / launch / finish
// Makes the phase's counter sets (and, for a dump stage, the device image of one LDS), and puts both
// sets at their reset values unless the last run left them so.
inline void ensure(DeviceCtx& c, const Plan& pl) {
  CounterSets& cs = c.lds.sets;
  cs.make(kSlots);
  if (!cs.clean) {  // first use, or a run that never reached finish()
    sync_streams(c);
    cs.reset<kSlots>(reset_value);
  }
  if (pl.dump_stage && !c.lds.dump) PROBE_CHECK(hipMalloc(&c.lds.dump, kBytesPerCU));
}

// Enqueues the phase on stream s: an event, the kernel, an event, the counters' copy. Settles the
// plan's salt (the context's run counter unless the caller gave one). No host synchronise.
inline void launch(DeviceCtx& c, hipStream_t s, Plan& pl) {
  if (!pl.salt_given) pl.salt = c.lds.runs;
  ++c.lds.runs;
  KernelArgs a{};
  a.n16 = pl.n16;
  a.seed = pl.seed ^ pl.salt;
  a.stride = pl.stride();
  a.patterns = pl.patterns;
  a.flip_byte = pl.flip_byte >= 0 && pl.flip_byte < static_cast<long long>(pl.n16) * 16 ? static_cast<uint32_t>(pl.flip_byte) : ~0u;
  a.skip_chunk = pl.skip_chunk >= 0 && pl.skip_chunk < static_cast<long long>(pl.n16) ? static_cast<uint32_t>(pl.skip_chunk) : ~0u;
  a.fault_xcc = pl.fault_xcc;
  a.dump_stage = c.lds.dump ? pl.dump_stage : 0;
  a.dump = static_cast<u32x4*>(c.lds.dump);
  const int grid = pl.blocks_per_cu * c.prop.multiProcessorCount;
  c.lds.sets.run(s, kSlots, [&](unsigned long long* cnt, unsigned long long* next) {
    a.cnt = cnt;
    a.next = next;
    hipLaunchKernelGGL(lds_march, dim3(grid), dim3(kThreads), 0, s, a);
  });
}

// After the stream's synchronise: the counters -> the "lds" block's result.
inline LdsResult finish(DeviceCtx& c, const Plan& pl, bool require_all) {
  LdsResult r;
  const unsigned long long* h = c.lds.sets.res;
  r.bytes_per_cu = static_cast<uint64_t>(pl.n16) * 16;
  r.patterns = pl.patterns;
  r.salt = pl.salt;
  r.expected = c.prop.multiProcessorCount;
  r.require_all = require_all;
  r.workgroups = h[kSlotWorkgroups];
  r.bad_bits = h[kSlotBadBits];
  r.first_bad = h[kSlotFirstBad];
  if (pl.dump_stage && h[kSlotDumpCu] != ~0ull) r.dump_cu = static_cast<int>(h[kSlotDumpCu]);
  const CuFold f = fold_cus(h + kSlotTested, h + kSlotBad);
  r.tested = f.tested;
  r.bad_cus = f.bad;
  r.verified = f.verified;
  for (int x = 0; x < 8; ++x) r.per_xcd[x] = f.per_xcd[x];
  r.ms = c.lds.sets.end();
  return r;
}

}  // namespace lds
}  // namespace
