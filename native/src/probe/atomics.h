// Atomic-unit phase of the probe, opt-in with "atomCheck": every CU's LDS atomic unit, the L2 atomic
// units behind every CU and the combination of device-scope atomics from all XCDs run a fixed program
// of read-modify-write instructions whose final values and returned values the host computed
// (atomics_ref.h has the ops, the layout, the operand construction and the arithmetic). Shares the
// census's CU and SIMD identity (census.h) and the HBM test's umin64 (hbm.h).
//
// atom_march, 256-thread workgroups with ordinary register counts, owns nothing. Three layers:
//   lds  a table in LDS, one row of 64 slots per contended op; the four waves (four SIMDs) contend on
//        slot = lane. The returning ops run on words private to a (wave, lane): what comes back at step t
//        is the value after step t - 1, and each lane folds it into a digest. Ticket test: all 256
//        threads do a returning add of 1 on one word and set bit ``ret`` of a 256-bit map with ds_or.
//        A second addressing, slot = lane & 15 of a row-set of its own, runs the contended ops again
//        with four lanes of every wave on one word: the conflicts inside a wave.
//        After a barrier the workgroup compares table, private words, digests, map and word with the
//        host's, which are the same for every workgroup.
//        ds_add_u32 ds_sub_u32 ds_and_b32 ds_or_b32 ds_xor_b32 ds_min_u32 ds_max_u32 ds_min_i32 ds_max_i32
//        ds_add_f32 ds_pk_add_f16 ds_pk_add_bf16 ds_add_u64 ds_max_u64 ds_xor_b64 ds_add_f64 ds_max_f64
//        ds_add_rtn_u32 ds_inc_rtn_u32 ds_dec_rtn_u32 ds_wrxchg_rtn_b32 ds_cmpst_rtn_b32
//   l2   the same program through global_atomic_* at agent scope on a region private to the workgroup;
//        digests are compared here, in registers, the final values by atom_verify.
//        global_atomic_add sub and or xor umin umax smin smax add_f32 pk_add_f16 pk_add_bf16 add_x2
//        umax_x2 xor_x2 add_f64 max_f64, returning add inc dec swap cmpswap
//   dev  the contended ops on nine row-sets: one every workgroup hits and one per XCD, hit by the
//        workgroups that run there. A wave-instruction touches 64 consecutive slots, one per lane.
//        and / or carry the workgroup's own bit and the min / max family the workgroup's own operand
//        (wave 0, step 0), so each of them has a workgroup that decides it.
// The cas is issued twice per step and never retried: first it compares with the value the program
// tracks, which must succeed, then with a wrong value, which must fail and return the current one.
// Every atomic's address depends on the lane (the ticket word's through an opaque register), so the
// compiler cannot replace a wave's atomics by a cross-lane reduction and one lane's atomic.
// No workgroup waits for another: no spin, no flag, no retry; every wave runs a fixed instruction count.
// The workgroup also writes one record {CU key, XCD} at records[b] with a plain vector store.
//
// atom_verify is the second kernel on the same stream, and the kernel boundary is the only ordering
// it relies on. One workgroup per region and one per dev row-set and op: it compares every slot with the
// expectation (a dev row's population is the records with that XCD; the table holds what every
// workgroup contributes alike and dev_combine() scales it, the workgroups' own bits and min / max
// operands are replayed over the records) and then stores each word's initial value back, so the
// next run starts clean without a memset. The allocation path runs it once in init-only mode.
//
// atom_march<true> is the test instantiation, launched only when a hook or the dump is asked for. A
// stage-1 dump copies workgroup 0's LDS tables and digests out after step 0, between two barriers,
// and the run goes on.
//
// What it cannot find: the buffer_ and flat_ forms; system-scope atomics and fine-grained memory;
// LDS-DMA; ordering and visibility (only atomicity and arithmetic are tested); defects that need
// other data, clocks or temperatures than the run's.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "arena.h"        // kCuKeys, kCuMapWords
#include "atomics_ref.h"  // layout, operands, host expectation
#include "census.h"       // cu_key, simd_id, fold_cus, decode_dump
#include "ctx.h"
#include "hbm.h"      // umin64
#include "options.h"  // atom::Plan
#include "report.h"   // AtomResult
#include "types.h"

namespace {
namespace atom {

static_assert(kPlanLayers == kLayers && kPlanOps == kAllOps && kPlanTicket == kTicket && kPlanWideFirst == kOps4 &&
                  kPlanWideEnd == kOps && kPlanLanes == kLanes && kPlanDumpWords == kDumpWords &&
                  kPlanSeedBase == kSeedBase && kMaxIters == kRefMaxIters && kMaxBlocksPerCU * 256 == kMaxWorkgroups,
              "options.h mirrors atomics_ref.h");

constexpr int kThreads = kThreadsPerWg;
constexpr int kLdsWords = kRegionWords + 16 + kRowSetWords;  // the region, the ticket word, the 8-word ticket map, the second addressing's row-set
constexpr int kLds16Off = kRegionWords + 16;
constexpr int kTicketWord = kRegionWords, kTicketMap = kRegionWords + 1;
constexpr int kBadWgWords = kMaxWorkgroups / 64;

// One set of counters; two sets, and workgroup 0 of a run resets the OTHER set (ctx.h CounterSets).
constexpr int kSlotLdsBad = 0, kSlotL2Bad = 1, kSlotDevBad = 2, kSlotBadReturns = 3, kSlotTicket = 4, kSlotFirstBad = 5,
              kSlotWorkgroups = 6, kSlotDumpCu = 7, kSlotDumpSimds = 8, kSlotWgXcd = 9 /* 8 of them */,
              kSlotTested = 17, kSlotBadCu = kSlotTested + kCuMapWords, kSlotBadWg = kSlotBadCu + kCuMapWords,
              kSlots = kSlotBadWg + kBadWgWords;

__host__ __device__ constexpr unsigned long long reset_value(int slot) {
  return slot == kSlotFirstBad || slot == kSlotDumpCu || slot == kSlotDumpSimds ? ~0ull : 0ull;
}

struct KernelArgs {
  uint32_t seed;
  int iters;
  int layers;
  const uint32_t* expect;  // atomics_ref.h kExpWords
  uint32_t* regions;       // [grid][kRegionWords]
  uint32_t* dev;           // [kDevRowSets][kRowSetWords]
  uint2* records;          // [grid] {CU key, XCD}
  // test hooks (atom_march<true> only), -1: off
  int skip_layer, skip_op, skip_step, skip_lane;
  int flip_layer, flip_op, flip_step, flip_lane, flip_bit;
  int fault_xcc, fault_wg;
  int dump_stage;
  uint32_t* dump;  // kDumpWords, or null
  unsigned long long* cnt;   // this run's counter set
  unsigned long long* next;  // the next run's, reset here
};

struct VerifyArgs {
  uint32_t seed;
  int nwg;        // regions and records in use
  int layers;
  int init_only;  // 1: store the initial values, compare nothing
  const uint32_t* expect;
  uint32_t* regions;
  uint32_t* dev;
  const uint2* records;
  uint32_t* dump;  // or null
  unsigned long long* cnt;
};

using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using i16x2 = __attribute__((ext_vector_type(2))) short;
#define ATOM_AS(N) __attribute__((address_space(N)))

// ------------------------------------------------------------------ one atomic per helper
// kLocal: the pointer is into LDS, the scope the workgroup; else global memory at agent scope.
template <int kOp, bool kLocal>
__device__ __forceinline__ void issue(uint32_t* rowset, uint32_t lane /* the slot */, uint64_t a) {
  constexpr int kScope = kLocal ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  uint32_t* p = rowset + row_word(kOp) + (wide(kOp) ? 2u * lane : lane);
  const uint32_t a32 = static_cast<uint32_t>(a);
  if constexpr (kOp == kAdd) __hip_atomic_fetch_add(p, a32, __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kSub) __hip_atomic_fetch_sub(p, a32, __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kAnd) __hip_atomic_fetch_and(p, a32, __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kOr) __hip_atomic_fetch_or(p, a32, __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kXor) __hip_atomic_fetch_xor(p, a32, __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kUmin) __hip_atomic_fetch_min(p, a32, __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kUmax) __hip_atomic_fetch_max(p, a32, __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kSmin) __hip_atomic_fetch_min(reinterpret_cast<int*>(p), static_cast<int>(a32), __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kSmax) __hip_atomic_fetch_max(reinterpret_cast<int*>(p), static_cast<int>(a32), __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kAddF32) unsafeAtomicAdd(reinterpret_cast<float*>(p), static_cast<float>(a32));
  else if constexpr (kOp == kPkF16) {
    const uint32_t bits = packed_bits(kPkF16, a32 & 1u, (a32 >> 1) & 1u);
    if constexpr (kLocal) __builtin_amdgcn_ds_atomic_fadd_v2f16((ATOM_AS(3) f16x2*)p, __builtin_bit_cast(f16x2, bits));
    else __builtin_amdgcn_global_atomic_fadd_v2f16((ATOM_AS(1) f16x2*)p, __builtin_bit_cast(f16x2, bits));
  } else if constexpr (kOp == kPkBf16) {
    const uint32_t bits = packed_bits(kPkBf16, a32 & 1u, (a32 >> 1) & 1u);
    if constexpr (kLocal) __builtin_amdgcn_ds_atomic_fadd_v2bf16((ATOM_AS(3) i16x2*)p, __builtin_bit_cast(i16x2, bits));
    else __builtin_amdgcn_global_atomic_fadd_v2bf16((ATOM_AS(1) i16x2*)p, __builtin_bit_cast(i16x2, bits));
  } else if constexpr (kOp == kAdd64) __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(a), __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kUmax64) __hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(a), __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kXor64) __hip_atomic_fetch_xor(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(a), __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kAddF64) unsafeAtomicAdd(reinterpret_cast<double*>(p), static_cast<double>(a));
  else if constexpr (kOp == kMaxF64) unsafeAtomicMax(reinterpret_cast<double*>(p), static_cast<double>(a));
}

// a returning op on a private word: the value that came back
template <int kOp, bool kLocal>
__device__ __forceinline__ uint32_t issue_rtn(uint32_t* p, uint32_t a) {
  constexpr int kScope = kLocal ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  if constexpr (kOp == kRetAdd) return __hip_atomic_fetch_add(p, a, __ATOMIC_RELAXED, kScope);
  else if constexpr (kOp == kRetInc) return atomicInc(p, a);
  else if constexpr (kOp == kRetDec) return atomicDec(p, a);
  else return __hip_atomic_exchange(p, a, __ATOMIC_RELAXED, kScope);
}
template <bool kLocal>
__device__ __forceinline__ uint32_t issue_cas(uint32_t* p, uint32_t compare, uint32_t value) {
  constexpr int kScope = kLocal ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  __hip_atomic_compare_exchange_strong(p, &compare, value, __ATOMIC_RELAXED, __ATOMIC_RELAXED, kScope);
  return compare;  // what the word held
}

// what a thread needs to build an operand and to apply the test hooks
struct Lane {
  uint32_t seed, lane, wave, b;
  bool struck;  // wave 0 of a workgroup the hooks apply to
};

template <bool kTest>
__device__ __forceinline__ bool skipped(const KernelArgs& a, const Lane& l, int layer, int op, uint32_t t) {
  if constexpr (!kTest) return false;
  return l.struck && a.skip_layer == layer && a.skip_op == op && static_cast<uint32_t>(a.skip_step) == t &&
         static_cast<uint32_t>(a.skip_lane) == l.lane;
}
template <bool kTest>
__device__ __forceinline__ uint64_t flipped(const KernelArgs& a, const Lane& l, int layer, int op, uint32_t t) {
  if constexpr (!kTest) return 0ull;
  return l.struck && a.flip_layer == layer && a.flip_op == op && static_cast<uint32_t>(a.flip_step) == t &&
                 static_cast<uint32_t>(a.flip_lane) == l.lane
             ? 1ull << (a.flip_bit & 63)
             : 0ull;
}

// one contended op of step t on ``rowset`` (and, dev, on ``rowset2`` with the same operand)
template <int kLayer, bool kTest, int kOp>
__device__ __forceinline__ void contend_one(const KernelArgs& a, const Lane& l, uint32_t t, uint32_t* rowset, uint32_t* rowset2) {
  if (!issues(kLayer, kOp, t, l.wave, l.b)) return;
  uint64_t w = kLayer == kDev && (kOp == kAnd || kOp == kOr) ? dev_bit_raw(kOp, l.b, l.lane)
               : kLayer == kDev && dev_own(kOp) && t == 0 && l.wave == 0 ? dev_own_raw(kOp, l.b, l.lane, l.seed)
                                                                         : raw(kLayer, kOp, t, l.wave, l.lane, l.seed);
  w ^= flipped<kTest>(a, l, kLayer, kOp, t);
  if (skipped<kTest>(a, l, kLayer, kOp, t)) return;
  const uint64_t v = arg(kLayer, kOp, w);
  issue<kOp, kLayer == kLds || kLayer == kLds16>(rowset, kLayer == kLds16 ? l.lane & (kSlots16 - 1) : l.lane, v);
  if constexpr (kLayer == kDev) issue<kOp, false>(rowset2, l.lane, v);
}
template <int kLayer, bool kTest, int... kOp>
__device__ __forceinline__ void contend(const KernelArgs& a, const Lane& l, uint32_t t, uint32_t* rowset, uint32_t* rowset2,
                                        std::integer_sequence<int, kOp...>) {
  (contend_one<kLayer, kTest, kOp>(a, l, t, rowset, rowset2), ...);
}

// the returning ops of step t on the lane's private words of ``region``; h is the lane's digest and
// cur what the program believes the cas word holds
template <int kLayer, bool kTest, int kOp>
__device__ __forceinline__ void return_one(const KernelArgs& a, const Lane& l, uint32_t t, uint32_t* region, uint32_t& h) {
  const uint32_t w = static_cast<uint32_t>(raw(kLayer, kOp, t, l.wave, l.lane, l.seed) ^ flipped<kTest>(a, l, kLayer, kOp, t));
  if (skipped<kTest>(a, l, kLayer, kOp, t)) return;
  h = fold(h, issue_rtn<kOp, kLayer == kLds>(region + priv_word(kOp, l.wave, l.lane), static_cast<uint32_t>(arg(kLayer, kOp, w))));
}
template <int kLayer, bool kTest>
__device__ __forceinline__ void returning(const KernelArgs& a, const Lane& l, uint32_t t, uint32_t* region, uint32_t& h, uint32_t& cur) {
  return_one<kLayer, kTest, kRetAdd>(a, l, t, region, h);
  return_one<kLayer, kTest, kRetInc>(a, l, t, region, h);
  return_one<kLayer, kTest, kRetDec>(a, l, t, region, h);
  return_one<kLayer, kTest, kRetSwap>(a, l, t, region, h);
  uint32_t* p = region + priv_word(kRetCas, l.wave, l.lane);
  const uint32_t clean = static_cast<uint32_t>(raw(kLayer, kRetCas, t, l.wave, l.lane, l.seed));
  const uint32_t value = clean ^ static_cast<uint32_t>(flipped<kTest>(a, l, kLayer, kRetCas, t));
  if (!skipped<kTest>(a, l, kLayer, kRetCas, t)) h = fold(h, issue_cas<kLayer == kLds>(p, cur, value));  // must succeed
  cur = clean;
  h = fold(h, issue_cas<kLayer == kLds>(p, ~clean, clean ^ 0x5A5A5A5Au));  // must fail and return the word
}

using ContendedOps = std::make_integer_sequence<int, kOps>;

// the 4 or 8 bytes of slot j of a region
__device__ __forceinline__ uint64_t slot_bits(const uint32_t* region, int j) {
  const int w = slot_word(j);
  return wide(slot_op(j)) ? (static_cast<uint64_t>(region[w + 1]) << 32) | region[w] : region[w];
}

template <bool kTest>
__global__ __launch_bounds__(kThreads) void atom_march(const KernelArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t b = blockIdx.x;
  if (b == 0)
    for (int i = static_cast<int>(tid); i < kSlots; i += kThreads) a.next[i] = reset_value(i);
  const int k = cu_key();
  const int xcc = (k >> 8) & 7;
  Lane l{a.seed, lane, wave, b, false};
  if constexpr (kTest)
    l.struck = wave == 0 && (a.fault_xcc < 0 || xcc == a.fault_xcc) && (a.fault_wg < 0 || static_cast<int>(b) == a.fault_wg);
  const uint32_t iters = static_cast<uint32_t>(a.iters);

  uint32_t bad_slots = 0, bad_returns = 0;
  uint64_t key = ~0ull;
  bool ticket_fault = false;
  uint32_t h_lds = 0, h_l2 = 0;

  for (int i = static_cast<int>(tid); i < kLdsWords; i += kThreads)
    lds[i] = i < kRegionWords ? init_word(i) : i < kLds16Off ? 0u : init_word(i - kLds16Off);
  __syncthreads();
  if (a.layers & 1) {
    uint32_t cur = 0;
#pragma unroll 1
    for (uint32_t t = 0; t < iters; ++t) {
      contend<kLds, kTest>(a, l, t, lds, lds, ContendedOps{});
      contend<kLds16, kTest>(a, l, t, lds + kLds16Off, lds, ContendedOps{});  // four lanes of a wave on one word
      returning<kLds, kTest>(a, l, t, lds, h_lds, cur);
      if constexpr (kTest) {
        if (t == 0 && b == 0 && a.dump && a.dump_stage == 1) {  // the state after step 0, then on with the run
          __syncthreads();
          for (int i = static_cast<int>(tid); i < kRegionWords; i += kThreads) a.dump[kDumpLds + i] = lds[i];
          for (int i = static_cast<int>(tid); i < kRowSetWords; i += kThreads) a.dump[kDumpLds16 + i] = lds[kLds16Off + i];
          a.dump[kDumpLdsDigest + tid] = h_lds;
          __syncthreads();
        }
      }
    }
    // ticket test: the word's address goes through an opaque register, so that it counts as divergent
    uint32_t tw = kTicketWord;
    asm volatile("" : "+v"(tw));
    if (!skipped<kTest>(a, l, kLds, kTicket, static_cast<uint32_t>(a.skip_step))) {
      const uint32_t r = __hip_atomic_fetch_add(&lds[tw], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_or(&lds[kTicketMap + ((r >> 5) & 7u)], 1u << (r & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    for (int j = static_cast<int>(tid); j < kRegionSlots; j += kThreads) {
      const int w = slot_word(j);
      const bool wd = wide(slot_op(j));
      if (lds[w] != a.expect[kExpLds + w] || (wd && lds[w + 1] != a.expect[kExpLds + w + 1])) {
        ++bad_slots;
        key = umin64(key, fault_key(kLds, slot_op(j), slot_index(j), xcc, k));
      }
    }
    for (int j = static_cast<int>(tid); j < kRowSetSlots; j += kThreads) {  // the second addressing; slots 16..63 untouched
      const int w = slot_word(j);
      const bool wd = wide(slot_op(j));
      if (lds[kLds16Off + w] != a.expect[kExpLds16 + w] || (wd && lds[kLds16Off + w + 1] != a.expect[kExpLds16 + w + 1])) {
        ++bad_slots;
        key = umin64(key, fault_key(kLds, slot_op(j), kLanes + slot_index(j), xcc, k));
      }
    }
    if (h_lds != a.expect[kExpLdsDigest + tid]) {
      ++bad_returns;
      key = umin64(key, fault_key(kLds, kReturns, static_cast<int>(tid), xcc, k));
    }
    if (tid < 9) {
      const bool off = tid == 0 ? lds[kTicketWord] != static_cast<uint32_t>(kThreads) : lds[kTicketMap + tid - 1] != ~0u;
      if (off) {
        ticket_fault = true;
        key = umin64(key, fault_key(kLds, kTicket, static_cast<int>(tid), xcc, k));
      }
    }
  }
  if constexpr (kTest) {
    if (b == 0 && a.dump && a.dump_stage == 2) {
      for (int i = static_cast<int>(tid); i < kRegionWords; i += kThreads) a.dump[kDumpLds + i] = lds[i];
      for (int i = static_cast<int>(tid); i < kRowSetWords; i += kThreads) a.dump[kDumpLds16 + i] = lds[kLds16Off + i];
      a.dump[kDumpLdsDigest + tid] = h_lds;
    }
  }
  if (a.layers & 2) {
    uint32_t* region = a.regions + static_cast<size_t>(b) * kRegionWords;
    uint32_t cur = 0;
#pragma unroll 1
    for (uint32_t t = 0; t < iters; ++t) {
      contend<kL2, kTest>(a, l, t, region, region, ContendedOps{});
      returning<kL2, kTest>(a, l, t, region, h_l2, cur);
      if constexpr (kTest)
        if (t == 0 && b == 0 && a.dump && a.dump_stage == 1) a.dump[kDumpL2Digest + tid] = h_l2;
    }
    if (h_l2 != a.expect[kExpL2Digest + tid]) {
      ++bad_returns;
      key = umin64(key, fault_key(kL2, kReturns, static_cast<int>(tid), xcc, k));
    }
  }
  if constexpr (kTest)
    if (b == 0 && a.dump && (a.dump_stage == 2 || !(a.layers & 2))) a.dump[kDumpL2Digest + tid] = h_l2;
  if (a.layers & 4) {
    uint32_t* own = a.dev + xcc * kRowSetWords;
    uint32_t* all = a.dev + kAllXcd * kRowSetWords;
#pragma unroll 1
    for (uint32_t t = 0; t < iters; ++t) contend<kDev, kTest>(a, l, t, own, all, ContendedOps{});
  }
  if (tid == 0) a.records[b] = make_uint2(static_cast<uint32_t>(k), static_cast<uint32_t>(xcc));

  // ---- one atomic group per wave, only when something is bad
  const unsigned long long ticket_mask = __ballot(ticket_fault);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bad_slots += __shfl_xor(bad_slots, off, 64);
    bad_returns += __shfl_xor(bad_returns, off, 64);
    key = umin64(key, static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(key), off, 64)));
  }
  if (lane == 0) {
    if (bad_slots || bad_returns || ticket_mask) {
      if (bad_slots) atomicAdd(&a.cnt[kSlotLdsBad], static_cast<unsigned long long>(bad_slots));
      if (bad_returns) atomicAdd(&a.cnt[kSlotBadReturns], static_cast<unsigned long long>(bad_returns));
      if (ticket_mask) atomicAdd(&a.cnt[kSlotTicket], 1ull);  // wave 0 holds all nine checking threads
      atomicMin(&a.cnt[kSlotFirstBad], static_cast<unsigned long long>(key));
      atomicOr(&a.cnt[kSlotBadCu + (k >> 6)], 1ull << (k & 63));
      atomicOr(&a.cnt[kSlotBadWg + (b >> 6)], 1ull << (b & 63u));
    }
    if (wave == 0) {
      atomicOr(&a.cnt[kSlotTested + (k >> 6)], 1ull << (k & 63));
      atomicAdd(&a.cnt[kSlotWgXcd + xcc], 1ull);
      atomicAdd(&a.cnt[kSlotWorkgroups], 1ull);
    }
    if constexpr (kTest) {
      if (b == 0 && a.dump) {
        atomicMin(&a.cnt[kSlotDumpCu], static_cast<unsigned long long>(k));
        // each wave of workgroup 0 clears its own byte of the all-ones word and leaves its SIMD there
        atomicAnd(&a.cnt[kSlotDumpSimds], ~(0xFFull << (8 * wave)) | (static_cast<unsigned long long>(simd_id()) << (8 * wave)));
      }
    }
  }
}

// Workgroup r < nwg: region r against the l2 table, charged to the CU in its record. Workgroup
// nwg + s * 17 + op: op's row of dev row-set s against the base table combined with its population.
// Then the initial values.
__global__ __launch_bounds__(kThreads) void atom_verify(const VerifyArgs a) {
  __shared__ uint32_t s_n, s_npk, s_bits[kLanes];
  __shared__ uint64_t s_own[kWaves][kLanes];  // the waves' partial extremes of a min / max row
  __shared__ uint16_t s_pop[kMaxWorkgroups];  // a dev row's population, in arrival order (the replay is order-free)
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const int r = static_cast<int>(blockIdx.x);
  uint32_t bad = 0;
  uint64_t key = ~0ull;
  if (r < a.nwg) {
    uint32_t* region = a.regions + static_cast<size_t>(r) * kRegionWords;
    const bool check = !a.init_only && (a.layers & 2);
    const uint2 rec = check || a.dump ? a.records[r] : make_uint2(0u, 0u);
    if (check)
      for (int j = static_cast<int>(tid); j < kRegionSlots; j += kThreads)
        if (slot_bits(region, j) != slot_bits(a.expect + kExpL2, j)) {
          ++bad;
          key = umin64(key, fault_key(kL2, slot_op(j), slot_index(j), static_cast<int>(rec.y & 7u), static_cast<int>(rec.x & 0x7FFu)));
        }
    if (r == 0 && a.dump && !a.init_only)
      for (int i = static_cast<int>(tid); i < kRegionWords; i += kThreads) a.dump[kDumpRegion + i] = region[i];
    __syncthreads();  // every compare of this workgroup is behind its loads
    for (int i = static_cast<int>(tid); i < kRegionWords; i += kThreads) region[i] = init_word(i);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      bad += __shfl_xor(bad, off, 64);
      key = umin64(key, static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(key), off, 64)));
    }
    if (lane == 0 && bad) {
      const uint32_t k = rec.x & 0x7FFu;
      atomicAdd(&a.cnt[kSlotL2Bad], static_cast<unsigned long long>(bad));
      atomicMin(&a.cnt[kSlotFirstBad], static_cast<unsigned long long>(key));
      atomicOr(&a.cnt[kSlotBadCu + (k >> 6)], 1ull << (k & 63u));
      atomicOr(&a.cnt[kSlotBadWg + (r >> 6)], 1ull << (r & 63));
    }
    return;
  }
  // one workgroup per (row-set, op): the op's 64 slots; wave w replays every fourth workgroup of the population
  const int s = (r - a.nwg) / kOps, op = (r - a.nwg) % kOps;  // s < kDevRowSets by the grid
  uint32_t* rowset = a.dev + s * kRowSetWords;
  const int w0 = row_word(op), words = wide(op) ? 2 * kLanes : kLanes;
  const bool check = !a.init_only && (a.layers & 4);
  if (check) {
    if (tid == 0) s_n = 0, s_npk = 0;
    if (tid < kLanes) s_bits[tid] = 0;
    __syncthreads();
    for (int b = static_cast<int>(tid); b < a.nwg; b += kThreads) {
      if (s == kAllXcd && op == 0 && a.dump) a.dump[kDumpRecords + b] = a.records[b].x;
      if (s != kAllXcd && static_cast<int>(a.records[b].y) != s) continue;
      s_pop[atomicAdd(&s_n, 1u)] = static_cast<uint16_t>(b);  // < nwg <= kMaxWorkgroups entries
      if (b < kPackedWorkgroups) atomicAdd(&s_npk, 1u);
      atomicOr(&s_bits[(b >> 5) & 63], 1u << (b & 31));
    }
    __syncthreads();
    const uint32_t n = s_n, npk = s_npk, part = tid >> 6;
    const int j = op * kLanes + static_cast<int>(lane);  // the slot
    const uint64_t base = slot_bits(a.expect + kExpDev, j);
    if (dev_own(op)) {  // replay the population's own operands
      uint64_t own = base;
      for (uint32_t i = part; i < n; i += kWaves) own = extreme(op, own, arg(kDev, op, dev_own_raw(op, s_pop[i], lane, a.seed)));
      s_own[part][lane] = own;
    }
    __syncthreads();
    if (part == 0) {
      uint64_t want;
      if (dev_own(op)) {
        uint64_t own = s_own[0][lane];
#pragma unroll
        for (int q = 1; q < kWaves; ++q) own = extreme(op, own, s_own[q][lane]);
        want = dev_own_combine(op, base, n, own);
      } else {
        want = dev_combine(op, base, n, npk, s_bits[lane]);
      }
      if (slot_bits(rowset, j) != want) {
        ++bad;
        key = umin64(key, fault_key(kDev, op, static_cast<int>(lane), s, 0));
      }
    }
  }
  if (a.dump && !a.init_only)
    for (int i = static_cast<int>(tid); i < words; i += kThreads) a.dump[kDumpDev + s * kRowSetWords + w0 + i] = rowset[w0 + i];
  __syncthreads();
  for (int i = static_cast<int>(tid); i < words; i += kThreads) rowset[w0 + i] = init_word(w0 + i);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bad += __shfl_xor(bad, off, 64);
    key = umin64(key, static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(key), off, 64)));
  }
  if (lane == 0 && bad) {
    atomicAdd(&a.cnt[kSlotDevBad], static_cast<unsigned long long>(bad));
    atomicMin(&a.cnt[kSlotFirstBad], static_cast<unsigned long long>(key));
  }
}

// ------------------------------------------------------------------ the phase: ensure / launch / finish
// the grid of a plan: never more workgroups than the bad-workgroup map and the dump's records hold
inline int grid_of(const DeviceCtx& c, const Plan& pl) { return std::min(kMaxWorkgroups, pl.blocks_per_cu * c.prop.multiProcessorCount); }
inline uint32_t* regions_of(DeviceCtx& c) { return c.atom.mem; }
inline uint32_t* dev_of(DeviceCtx& c) { return c.atom.mem + static_cast<size_t>(c.atom.wgs) * kRegionWords; }
inline uint2* records_of(DeviceCtx& c) { return reinterpret_cast<uint2*>(dev_of(c) + kDevRowSets * kRowSetWords); }

// Makes the phase's expectation table, counter sets and data buffers (and, for a dump stage, the
// device copy of the dump); grows the data buffers when the plan's grid is larger than the one they
// were made for and runs atom_verify in init-only mode on new ones; puts both counter sets at their
// reset values unless the last run left them so; computes and uploads the host's expectation when
// (seed, iters) is not the pair the table holds. All ahead of the probe's clock.
inline void ensure(DeviceCtx& c, const Plan& pl) {
  auto& x = c.atom;
  if (!x.ev_mid) PROBE_CHECK(hipEventCreate(&x.ev_mid));
  if (!x.exp) PROBE_CHECK(hipMalloc(reinterpret_cast<void**>(&x.exp), kExpWords * sizeof(uint32_t)));
  x.sets.make(kSlots);
  const int grid = grid_of(c, pl);
  const bool stale = x.exp_iters != pl.iters || x.exp_seed != pl.seed;
  const bool grow = grid > x.wgs;
  // first use, a run that never reached finish(), or buffers a run may still use
  if (!x.sets.clean || stale || grow) sync_streams(c);
  if (grow) {
    if (x.mem) PROBE_CHECK(hipFree(x.mem));
    x.mem = nullptr;
    x.wgs = 0;
    const size_t words = static_cast<size_t>(grid) * kRegionWords + kDevRowSets * kRowSetWords + static_cast<size_t>(grid) * 2;
    PROBE_CHECK(hipMalloc(reinterpret_cast<void**>(&x.mem), words * sizeof(uint32_t)));
    x.wgs = grid;
    x.sets.clean = false;  // a run cut short may have left any word behind: the whole buffer is initialised below
  }
  if (!x.sets.clean)
    x.sets.reset<kSlots>(reset_value, [&] {
      VerifyArgs v{};
      v.nwg = x.wgs;
      v.init_only = 1;
      v.regions = regions_of(c);
      v.dev = dev_of(c);
      v.records = records_of(c);
      v.cnt = x.sets.cnt;
      hipLaunchKernelGGL(atom_verify, dim3(x.wgs + kDevRowSets * kOps), dim3(kThreads), 0, c.stream, v);
      PROBE_CHECK(hipGetLastError());
      PROBE_CHECK(hipStreamSynchronize(c.stream));
    });
  if (stale) {
    std::vector<uint32_t> table(kExpWords);
    expected(pl.seed, pl.iters, table.data());
    x.exp_iters = 0;
    PROBE_CHECK(hipMemcpy(x.exp, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    x.exp_seed = pl.seed;
    x.exp_iters = pl.iters;
  }
  if (pl.dump_stage && !x.dump) PROBE_CHECK(hipMalloc(reinterpret_cast<void**>(&x.dump), kDumpBytes));
}

// Enqueues the phase on stream s: an event, the two kernels, an event, the counters' copy. No host synchronise.
inline void launch(DeviceCtx& c, hipStream_t s, const Plan& pl) {
  auto& x = c.atom;
  const int grid = grid_of(c, pl);  // <= x.wgs by ensure()
  KernelArgs a{};
  a.seed = pl.seed;
  a.iters = pl.iters;
  a.layers = pl.layers;
  a.expect = x.exp;
  a.regions = regions_of(c);
  a.dev = dev_of(c);
  a.records = records_of(c);
  a.skip_layer = pl.skip_layer, a.skip_op = pl.skip_op, a.skip_step = pl.skip_step, a.skip_lane = pl.skip_lane;
  a.flip_layer = pl.flip_layer, a.flip_op = pl.flip_op, a.flip_step = pl.flip_step, a.flip_lane = pl.flip_lane;
  a.flip_bit = pl.flip_bit;
  a.fault_xcc = pl.fault_xcc;
  a.fault_wg = pl.fault_wg;
  a.dump_stage = x.dump ? pl.dump_stage : 0;
  a.dump = a.dump_stage ? x.dump : nullptr;
  VerifyArgs v{};
  v.seed = pl.seed;
  v.nwg = grid;
  v.layers = pl.layers;
  v.expect = x.exp;
  v.regions = a.regions;
  v.dev = a.dev;
  v.records = a.records;
  v.dump = a.dump;
  // a dump run starts from a zeroed buffer: what a layer that does not run would have written reads 0
  if (a.dump) PROBE_CHECK(hipMemsetAsync(x.dump, 0, kDumpBytes, s));
  x.sets.run(s, kSlots, [&](unsigned long long* cnt, unsigned long long* next) {
    a.cnt = v.cnt = cnt;
    a.next = next;
    if (pl.test_kernel()) hipLaunchKernelGGL(atom_march<true>, dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(atom_march<false>, dim3(grid), dim3(kThreads), 0, s, a);
    if (pl.time_kernels) PROBE_CHECK(hipEventRecord(x.ev_mid, s));
    hipLaunchKernelGGL(atom_verify, dim3(grid + kDevRowSets * kOps), dim3(kThreads), 0, s, v);
  });
}

// After the stream's synchronise: the counters -> the "atomics" block's result.
inline AtomResult finish(DeviceCtx& c, const Plan& pl, bool require_all) {
  AtomResult r;
  CounterSets& cs = c.atom.sets;
  const unsigned long long* h = cs.res;
  r.iters = pl.iters;
  r.layers = pl.layers;
  r.expected = c.prop.multiProcessorCount;
  r.require_all = require_all;
  r.workgroups = h[kSlotWorkgroups];
  for (int x = 0; x < 8; ++x) r.wg_per_xcd[x] = h[kSlotWgXcd + x];
  r.lds_bad_slots = h[kSlotLdsBad];
  r.l2_bad_slots = h[kSlotL2Bad];
  r.dev_bad_slots = h[kSlotDevBad];
  r.bad_returns = h[kSlotBadReturns];
  r.ticket_faults = h[kSlotTicket];
  r.first_bad = h[kSlotFirstBad];
  if (pl.dump_stage) decode_dump(h[kSlotDumpCu], h[kSlotDumpSimds], &r.dump_cu, r.dump_simds);
  // a CU in the bad map counts as tested, whether or not a clean workgroup ran there too
  unsigned long long tested[kCuMapWords];
  for (int w = 0; w < kCuMapWords; ++w) tested[w] = h[kSlotTested + w] | h[kSlotBadCu + w];
  const CuFold f = fold_cus(tested, h + kSlotBadCu);
  r.cus_tested = f.tested;
  r.cus_verified = f.verified;
  r.bad_cus = f.bad;
  for (int x = 0; x < 8; ++x) r.per_xcd[x] = f.per_xcd[x];
  for (int w = 0; w < kBadWgWords; ++w) r.bad_workgroups += __builtin_popcountll(h[kSlotBadWg + w]);
  if (pl.time_kernels) {
    PROBE_CHECK(hipEventElapsedTime(&r.march_ms, cs.ev[0], c.atom.ev_mid));
    PROBE_CHECK(hipEventElapsedTime(&r.verify_ms, c.atom.ev_mid, cs.ev[1]));
  }
  r.ms = cs.end();
  return r;
}

#undef ATOM_AS
}  // namespace atom
}  // namespace
