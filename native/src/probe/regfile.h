// Register-file phase of the probe, opt-in with "regCheck": the vector register file of every SIMD
// of every CU (512 registers x 64 lanes x 4 B = 128 KiB per SIMD, 512 KiB per CU: the largest SRAM
// in a CU) is marched in both polarities by a wave that owns all of it. Shares the HBM test's
// pattern16 and umin64 (hbm.h) and the census's CU identity (census.h).
//
// On gfx950 VGPRs and AGPRs are one 512-entry-per-lane file per SIMD. The kernel's asm statements
// clobber v0..v255 and a0..a255, so its descriptor asks for all 512 registers and a SIMD holds one
// wave of it: a 256-thread workgroup puts one wave on each of the CU's four SIMDs, nothing else can
// co-reside on that CU, and "this workgroup tested this CU's whole vector register file" is a true
// statement. That is checked, not assumed: ensure() asks the runtime for the kernel's register
// count and its workgroups per CU, and the phase fails as RegisterKernelNotExclusive unless they
// are 512 and 1; each wave reads its SIMD id (HW_ID[5:4]) and a workgroup marks its CU tested only
// when its four waves sat on four different SIMDs (else it counts into simdShort).
//
// Registers are numbered u = 0..511: v0..v255 are 0..255, a0..a255 are 256..511. Register u of lane
// l of wave w of workgroup b is expected to hold E(u) = (base + u * 0x9E3779B1) ^ flip, with
// base = pattern16<1>((b << 32) | (64 w + l), seed, 0).x computed in C++ ahead of the asm. The
// multiplier is odd, so no two registers of a lane share a value and a row-decode alias reads
// another register's value; base differs per lane, wave, workgroup and run (the seed is salted),
// so what the file's previous owner left is never the expected value.
//
// March, per polarity: (1) write every register, ascending; (2) verify each, ascending, and write
// its complement, computed from E and never from what the register holds; (3) verify the
// complements, descending. AGPRs are written and read only through v_accvgpr_write_b32 /
// v_accvgpr_read_b32; there is no MFMA here (the census owns the matrix cores).
//
// The registers that hold the compiler's operands cannot be tested by the statement that uses them,
// so the march is TWO asm statements built from the same macros:
//   statement A  tests v16..v255 and a0..a255 (u = 16..511); its operands sit in v0..v15
//   statement B  tests v0..v15 (u = 0..15) and clobbers exactly those; its operands sit above them
// Every one of the 512 registers is written and verified in one of the two. Each verify counts the
// differing bits (v_bcnt_u32_b32 accumulates) and keeps the lowest u that differed per lane, inside
// the asm: nothing survives between statements but what the operands carry.
//
// rf_march<true> is the test instantiation, launched only when a hook or the dump is asked for; it
// adds, inside the asm strings, the fault hooks (flip one bit of one register of one lane after the
// first write, on every wave, on one SIMD or on one XCD; leave one register out of the first write)
// and the dump of workgroup 0's registers (vector stores through an SGPR base that SALU adds
// advance; the pair s[98:99] is named and clobbered because a 64-bit operand's halves cannot be
// named). rf_march<false>, the production instantiation, carries none of it.
//
// What it cannot find: SGPR faults, coupling between the two statements' ranges (B runs after A has
// finished with its range), faults that need a retention time, and anything outside the file.
#pragma once

#include <cstdint>

#include "arena.h"    // kCuMapWords
#include "census.h"   // cu_key, simd_id, fold_cus, decode_dump
#include "ctx.h"      // DeviceCtx, CounterSets: the phase's events, counters and pinned result
#include "hbm.h"      // pattern16, umin64
#include "options.h"  // regs::Plan
#include "report.h"   // RegsResult
#include "types.h"

namespace {
namespace regs {

constexpr int kThreads = 256;

// One set of counters; two sets, and workgroup 0 of a run resets the OTHER set (ctx.h CounterSets).
constexpr int kSlotBadBits = 0, kSlotFirstBad = 1, kSlotWorkgroups = 2, kSlotSimdShort = 3, kSlotDumpCu = 4,
              kSlotDumpSimds = 5, kSlotTested = 6, kSlotBad = kSlotTested + kCuMapWords,
              kSlots = kSlotBad + kCuMapWords;
static_assert(kSlots <= kThreads, "workgroup 0 resets a counter set with one store per thread");

__host__ __device__ constexpr unsigned long long reset_value(int slot) {
  return slot == kSlotFirstBad || slot == kSlotDumpCu || slot == kSlotDumpSimds ? ~0ull : 0ull;
}

struct KernelArgs {
  uint32_t seed;  // salted
  int patterns;
  // test hooks (rf_march<true> only), out of range: off
  uint32_t flip_u, flip_lane, flip_bit;
  int fault_simd, fault_xcc;  // the flip only on this SIMD / XCD (< 0: on all)
  uint32_t skip_u;
  int dump_stage;  // 1 | 2: workgroup 0 stores its registers to ``dump`` there
  uint32_t* dump;  // [4][512][64]
  unsigned long long* cnt;   // this run's counter set
  unsigned long long* next;  // the next run's, reset here
};

// ------------------------------------------------------------------ the asm text
// Assembler repetition: the symbol rf_i walks the register indices of a range, up or down.
#define RF_STR2(x) #x
#define RF_STR(x) RF_STR2(x)
#define RF_UP(LO, N, BODY) ".set rf_i, " RF_STR(LO) "\n.rept " RF_STR(N) "\n" BODY ".set rf_i, rf_i + 1\n.endr\n"
#define RF_DOWN(HI, N, BODY) ".set rf_i, " RF_STR(HI) "\n.rept " RF_STR(N) "\n" BODY ".set rf_i, rf_i - 1\n.endr\n"
#define RF_UV "rf_i"          // the unified index of v[rf_i]
#define RF_UA "(rf_i + 256)"  // ... of a[rf_i]
// DST = E(U) at polarity FLIP (an SGPR operand's name)
#define RF_E(DST, U, FLIP)                                               \
  "v_add_u32 " DST ", (" U " * 0x9E3779B1) & 0xffffffff, %[base]\n" \
  "v_xor_b32 " DST ", %[" FLIP "], " DST "\n"
// VAL against %[te]: differing bits into %[bad], the lowest differing U into %[first]. Two VALU
// instructions sit between the v_cmp that writes VCC and the v_cndmask that reads it: gfx950 needs
// two wait states there and nothing pads the inside of an asm string.
#define RF_CHECK(U, VAL)                       \
  "v_xor_b32 %[tx], %[te], " VAL "\n"        \
  "v_cmp_ne_u32 vcc, 0, %[tx]\n"             \
  "v_bcnt_u32_b32 %[bad], %[tx], %[bad]\n"   \
  "v_min_u32 %[tc], " U ", %[first]\n"       \
  "v_cndmask_b32 %[first], %[first], %[tc], vcc\n"

// march steps over arch registers v[rf_i] and over acc registers a[rf_i]
#define RF_WRITE_V RF_E("v[rf_i]", RF_UV, "flip")
#define RF_WRITE_A RF_E("%[te]", RF_UA, "flip") "v_accvgpr_write_b32 a[rf_i], %[te]\n"
#define RF_VERIFY1_V RF_E("%[te]", RF_UV, "flip") RF_CHECK(RF_UV, "v[rf_i]") "v_not_b32 v[rf_i], %[te]\n"
#define RF_VERIFY1_A                                                                         \
  RF_E("%[te]", RF_UA, "flip") "v_accvgpr_read_b32 %[tr], a[rf_i]\n" RF_CHECK(RF_UA, "%[tr]") \
  "v_not_b32 %[te], %[te]\n"                                                                 \
  "v_accvgpr_write_b32 a[rf_i], %[te]\n"
#define RF_VERIFY2_V RF_E("%[te]", RF_UV, "nflip") RF_CHECK(RF_UV, "v[rf_i]")
#define RF_VERIFY2_A RF_E("%[te]", RF_UA, "nflip") "v_accvgpr_read_b32 %[tr], a[rf_i]\n" RF_CHECK(RF_UA, "%[tr]")

// test instantiation: the first write leaves register %[skip_u] alone
#define RF_TWRITE_V                                 \
  RF_E("%[te]", RF_UV, "flip")                      \
  "s_cmp_eq_u32 %[skip_u], " RF_UV "\n"           \
  "s_cselect_b64 vcc, -1, 0\n"                    \
  "v_cndmask_b32 v[rf_i], %[te], v[rf_i], vcc\n"
#define RF_TWRITE_A                               \
  RF_E("%[te]", RF_UA, "flip")                    \
  "v_accvgpr_read_b32 %[tr], a[rf_i]\n"         \
  "s_cmp_eq_u32 %[skip_u], " RF_UA "\n"         \
  "s_cselect_b64 vcc, -1, 0\n"                  \
  "v_cndmask_b32 %[te], %[te], %[tr], vcc\n"    \
  "v_accvgpr_write_b32 a[rf_i], %[te]\n"
// ... then register %[flip_u] is XORed with %[fmask] (the bit in the chosen lane of the chosen waves)
#define RF_FLIP_V                           \
  "s_cmp_eq_u32 %[flip_u], " RF_UV "\n"   \
  "s_cselect_b32 %[st], -1, 0\n"          \
  "v_and_b32 %[tx], %[st], %[fmask]\n"    \
  "v_xor_b32 v[rf_i], v[rf_i], %[tx]\n"
#define RF_FLIP_A                           \
  "s_cmp_eq_u32 %[flip_u], " RF_UA "\n"   \
  "s_cselect_b32 %[st], -1, 0\n"          \
  "v_and_b32 %[tx], %[st], %[fmask]\n"    \
  "v_accvgpr_read_b32 %[tr], a[rf_i]\n"   \
  "v_xor_b32 %[tr], %[tr], %[tx]\n"       \
  "v_accvgpr_write_b32 a[rf_i], %[tr]\n"
// ... and at %[stage] == STAGE the statement's registers go to the image, 256 B per register
#define RF_STORE(VAL)                                     \
  "global_store_dword %[voff], " VAL ", s[98:99]\n"     \
  "s_add_u32 s98, s98, 256\n"                           \
  "s_addc_u32 s99, s99, 0\n"
#define RF_STORE_V RF_STORE("v[rf_i]")
#define RF_STORE_A "v_accvgpr_read_b32 %[tr], a[rf_i]\n" RF_STORE("%[tr]")
#define RF_DUMP(STAGE, STORES)                    \
  "s_cmp_lg_u32 %[stage], " RF_STR(STAGE) "\n"  \
  "s_cbranch_scc1 .Lrf_nodump" RF_STR(STAGE) "_%=\n" \
  "s_mov_b64 s[98:99], %[ptr]\n"                \
  STORES                                          \
  "s_waitcnt vmcnt(0)\n"                        \
  ".Lrf_nodump" RF_STR(STAGE) "_%=:\n"

// Statement A: v16..v255 and a0..a255. Statement B: v0..v15.
#define RF_A_LO 16
#define RF_A_N 240
#define RF_B_N 16
#define RF_MARCH_A                                                                             \
  RF_UP(RF_A_LO, RF_A_N, RF_WRITE_V) RF_UP(0, 256, RF_WRITE_A)                                 \
  RF_UP(RF_A_LO, RF_A_N, RF_VERIFY1_V) RF_UP(0, 256, RF_VERIFY1_A)                             \
  RF_DOWN(255, 256, RF_VERIFY2_A) RF_DOWN(255, RF_A_N, RF_VERIFY2_V)
#define RF_MARCH_B RF_UP(0, RF_B_N, RF_WRITE_V) RF_UP(0, RF_B_N, RF_VERIFY1_V) RF_DOWN(15, RF_B_N, RF_VERIFY2_V)
#define RF_TMARCH_A                                                                            \
  RF_UP(RF_A_LO, RF_A_N, RF_TWRITE_V) RF_UP(0, 256, RF_TWRITE_A)                               \
  RF_UP(RF_A_LO, RF_A_N, RF_FLIP_V) RF_UP(0, 256, RF_FLIP_A)                                   \
  RF_DUMP(1, RF_UP(RF_A_LO, RF_A_N, RF_STORE_V) RF_UP(0, 256, RF_STORE_A))                     \
  RF_UP(RF_A_LO, RF_A_N, RF_VERIFY1_V) RF_UP(0, 256, RF_VERIFY1_A)                             \
  RF_DUMP(2, RF_UP(RF_A_LO, RF_A_N, RF_STORE_V) RF_UP(0, 256, RF_STORE_A))                     \
  RF_DOWN(255, 256, RF_VERIFY2_A) RF_DOWN(255, RF_A_N, RF_VERIFY2_V)
#define RF_TMARCH_B                                                     \
  RF_UP(0, RF_B_N, RF_TWRITE_V) RF_UP(0, RF_B_N, RF_FLIP_V)             \
  RF_DUMP(1, RF_UP(0, RF_B_N, RF_STORE_V))                              \
  RF_UP(0, RF_B_N, RF_VERIFY1_V)                                        \
  RF_DUMP(2, RF_UP(0, RF_B_N, RF_STORE_V))                              \
  RF_DOWN(15, RF_B_N, RF_VERIFY2_V)

// clobber lists: v0..v15, v16..v255, a0..a255
#define RF_C8(P, a) P #a "0", P #a "1", P #a "2", P #a "3", P #a "4", P #a "5", P #a "6", P #a "7"
#define RF_C10(P, a) RF_C8(P, a), P #a "8", P #a "9"
#define RF_CLOB_0_15(P) P "0", P "1", P "2", P "3", P "4", P "5", P "6", P "7", P "8", P "9", P "10", P "11", P "12", P "13", P "14", P "15"
#define RF_CLOB_16_255(P)                                                                                  \
  P "16", P "17", P "18", P "19", RF_C10(P, 2), RF_C10(P, 3), RF_C10(P, 4), RF_C10(P, 5), RF_C10(P, 6),    \
  RF_C10(P, 7), RF_C10(P, 8), RF_C10(P, 9), RF_C10(P, 10), RF_C10(P, 11), RF_C10(P, 12), RF_C10(P, 13),    \
  RF_C10(P, 14), RF_C10(P, 15), RF_C10(P, 16), RF_C10(P, 17), RF_C10(P, 18), RF_C10(P, 19), RF_C10(P, 20), \
  RF_C10(P, 21), RF_C10(P, 22), RF_C10(P, 23), RF_C10(P, 24), P "250", P "251", P "252", P "253", P "254", P "255"
#define RF_CLOB_A RF_CLOB_16_255("v"), RF_CLOB_0_15("a"), RF_CLOB_16_255("a"), "vcc", "scc"
#define RF_CLOB_B RF_CLOB_0_15("v"), "vcc", "scc"

template <bool kTest>
__global__ __launch_bounds__(kThreads) void rf_march(const KernelArgs a) {
  __shared__ uint32_t simd_of[4];
  // A value that lives across both statements has no register to live in (A clobbers v16.. and every
  // AGPR, B clobbers v0..v15), so each one is a read-write operand of both and the compiler moves it.
  uint32_t tid = threadIdx.x;
  const uint32_t b = blockIdx.x;
  if (b == 0 && tid < kSlots) a.next[tid] = reset_value(static_cast<int>(tid));
  const int k = cu_key();  // the same for every wave of the workgroup
  const uint32_t simd = simd_id();
  uint32_t base = pattern16<1>((static_cast<uint64_t>(b) << 32) | tid, a.seed, 0).x;  // tid = 64 w + l
  uint32_t bad = 0, first = ~0u;  // flipped bits; the lowest u that differed in this lane
  uint32_t te, tx, tc, tr;        // the statements' working registers

  // test hooks: the bit to flip, in the chosen lane of the chosen waves; the lane's offset in an image row
  uint32_t fmask = 0, voff = (tid & 63) * 4;
  if constexpr (kTest) {
    const bool hit = (tid & 63) == a.flip_lane && (a.fault_simd < 0 || static_cast<int>(simd) == a.fault_simd) &&
                     (a.fault_xcc < 0 || (k >> 8) == a.fault_xcc);
    fmask = hit ? 1u << (a.flip_bit & 31u) : 0u;
  }

#pragma unroll 1
  for (int p = 0; p < a.patterns; ++p) {
    const uint32_t flip = (p & 1) ? 0xFFFFFFFFu : 0u, nflip = ~flip;  // as PatternPass::flip_of
    if constexpr (kTest) {
      // the hooks act on the first polarity only; out of range compares equal to no register
      const uint32_t flip_u = p == 0 ? a.flip_u : ~0u, skip_u = p == 0 ? a.skip_u : ~0u;
      const uint32_t stage = b == 0 && p == 0 ? static_cast<uint32_t>(a.dump_stage) : 0u;
      const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
      uint32_t* const img = a.dump + static_cast<size_t>(wave) * 512 * 64;
      uint32_t* ptr = img + RF_A_LO * 64;
      uint32_t st;
      asm volatile(RF_TMARCH_A
                   : [bad] "+v"(bad), [first] "+v"(first), [te] "=&v"(te), [tx] "=&v"(tx), [tc] "=&v"(tc),
                     [tr] "=&v"(tr), [st] "=&s"(st), [base] "+v"(base), [fmask] "+v"(fmask), [voff] "+v"(voff), "+v"(tid)
                   : [flip] "s"(flip), [nflip] "s"(nflip), [flip_u] "s"(flip_u), [skip_u] "s"(skip_u), [stage] "s"(stage),
                     [ptr] "s"(ptr)
                   : RF_CLOB_A, "s98", "s99", "memory");
      ptr = img;
      asm volatile(RF_TMARCH_B
                   : [bad] "+v"(bad), [first] "+v"(first), [te] "=&v"(te), [tx] "=&v"(tx), [tc] "=&v"(tc),
                     [st] "=&s"(st), [base] "+v"(base), [fmask] "+v"(fmask), [voff] "+v"(voff), "+v"(tid)
                   : [flip] "s"(flip), [nflip] "s"(nflip), [flip_u] "s"(flip_u), [skip_u] "s"(skip_u), [stage] "s"(stage),
                     [ptr] "s"(ptr)
                   : RF_CLOB_B, "s98", "s99", "memory");
    } else {
      asm volatile(RF_MARCH_A
                   : [bad] "+v"(bad), [first] "+v"(first), [te] "=&v"(te), [tx] "=&v"(tx), [tc] "=&v"(tc),
                     [tr] "=&v"(tr), [base] "+v"(base), "+v"(tid)
                   : [flip] "s"(flip), [nflip] "s"(nflip)
                   : RF_CLOB_A);
      asm volatile(RF_MARCH_B
                   : [bad] "+v"(bad), [first] "+v"(first), [te] "=&v"(te), [tx] "=&v"(tx), [tc] "=&v"(tc),
                     [base] "+v"(base), "+v"(tid)
                   : [flip] "s"(flip), [nflip] "s"(nflip)
                   : RF_CLOB_B);
    }
  }

  // ---- SIMD identity: the four waves exchange their ids; four different ones = the whole CU
  const uint32_t t = tid, lane = t & 63;
  if (lane == 0) simd_of[t >> 6] = simd;
  __syncthreads();
  const uint32_t seen = (1u << simd_of[0]) | (1u << simd_of[1]) | (1u << simd_of[2]) | (1u << simd_of[3]);

  // ---- count: one atomic group per wave, and only when something is bad
  // (CU key << 32) | SIMD << 16 | u << 6 | lane of the lowest fault
  uint64_t key = first == ~0u ? ~0ull : (static_cast<uint64_t>(k) << 32) | (simd << 16) | (first << 6) | lane;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bad += __shfl_xor(bad, off, 64);
    key = umin64(key, static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(key), off, 64)));
  }
  if (lane == 0 && bad) {
    atomicAdd(&a.cnt[kSlotBadBits], static_cast<unsigned long long>(bad));
    atomicMin(&a.cnt[kSlotFirstBad], static_cast<unsigned long long>(key));
    atomicOr(&a.cnt[kSlotBad + (k >> 6)], 1ull << (k & 63));
  }
  if (t == 0) {
    if (seen == 15u) atomicOr(&a.cnt[kSlotTested + (k >> 6)], 1ull << (k & 63));
    else atomicAdd(&a.cnt[kSlotSimdShort], 1ull);
    atomicAdd(&a.cnt[kSlotWorkgroups], 1ull);
    if constexpr (kTest) {
      if (b == 0 && a.dump_stage) {
        atomicMin(&a.cnt[kSlotDumpCu], static_cast<unsigned long long>(k));
        atomicMin(&a.cnt[kSlotDumpSimds], static_cast<unsigned long long>(simd_of[0] | (simd_of[1] << 8) |
                                                                           (simd_of[2] << 16) | (simd_of[3] << 24)));
      }
    }
  }
}

// ------------------------------------------------------------------ the phase: ensure / launch / finish
// What the runtime says of an instantiation: registers per lane and workgroups of 256 per CU. Asked
// once per context; finish() fails the phase unless they are 512 and 1.
template <bool kTest>
inline void ensure_attr(DeviceCtx& c) {
  int* at = c.regs.attr[kTest ? 1 : 0];
  if (at[0]) return;
  hipFuncAttributes fa{};
  PROBE_CHECK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&rf_march<kTest>)));
  int per_cu = 0;
  PROBE_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rf_march<kTest>, kThreads, 0));
  at[1] = per_cu;
  at[0] = fa.numRegs;
}

// Makes the phase's counter sets (and, for a dump stage, the device image of one workgroup's
// registers), and puts both sets at their reset values unless the last run left them so.
inline void ensure(DeviceCtx& c, const Plan& pl) {
  CounterSets& cs = c.regs.sets;
  cs.make(kSlots);
  if (pl.test_kernel()) ensure_attr<true>(c);
  else ensure_attr<false>(c);
  if (!cs.clean) {  // first use, or a run that never reached finish()
    sync_streams(c);
    cs.reset<kSlots>(reset_value);
  }
  if (pl.dump_stage && !c.regs.dump) PROBE_CHECK(hipMalloc(&c.regs.dump, kImageBytes));
}

// Enqueues the phase on stream s: an event, the kernel, an event, the counters' copy. Settles the
// plan's salt (the context's run counter unless the caller gave one). No host synchronise.
inline void launch(DeviceCtx& c, hipStream_t s, Plan& pl) {
  if (!pl.salt_given) pl.salt = c.regs.runs;
  ++c.regs.runs;
  KernelArgs a{};
  a.seed = pl.seed ^ pl.salt;
  a.patterns = pl.patterns;
  a.flip_u = pl.flip_u >= 0 ? static_cast<uint32_t>(pl.flip_u) : ~0u;
  a.flip_lane = pl.flip_u >= 0 ? static_cast<uint32_t>(pl.flip_lane) : ~0u;
  a.flip_bit = pl.flip_u >= 0 ? static_cast<uint32_t>(pl.flip_bit) : 0u;
  a.fault_simd = pl.fault_simd;
  a.fault_xcc = pl.fault_xcc;
  a.skip_u = pl.skip_u >= 0 ? static_cast<uint32_t>(pl.skip_u) : ~0u;
  a.dump_stage = c.regs.dump ? pl.dump_stage : 0;
  a.dump = static_cast<uint32_t*>(c.regs.dump);
  const int grid = pl.blocks_per_cu * c.prop.multiProcessorCount;
  c.regs.sets.run(s, kSlots, [&](unsigned long long* cnt, unsigned long long* next) {
    a.cnt = cnt;
    a.next = next;
    if (pl.test_kernel()) hipLaunchKernelGGL(rf_march<true>, dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(rf_march<false>, dim3(grid), dim3(kThreads), 0, s, a);
  });
}

// After the stream's synchronise: the counters -> the "regs" block's result.
inline RegsResult finish(DeviceCtx& c, const Plan& pl, bool require_all) {
  RegsResult r;
  const unsigned long long* h = c.regs.sets.res;
  const int* at = c.regs.attr[pl.test_kernel() ? 1 : 0];
  r.registers_per_lane = at[0];
  r.workgroups_per_cu = at[1];
  r.patterns = pl.patterns;
  r.salt = pl.salt;
  r.expected = c.prop.multiProcessorCount;
  r.require_all = require_all;
  r.workgroups = h[kSlotWorkgroups];
  r.simd_short = h[kSlotSimdShort];
  r.bad_bits = h[kSlotBadBits];
  r.first_bad = h[kSlotFirstBad];
  if (pl.dump_stage) decode_dump(h[kSlotDumpCu], h[kSlotDumpSimds], &r.dump_cu, r.dump_simds);
  const CuFold f = fold_cus(h + kSlotTested, h + kSlotBad);
  r.tested = f.tested;
  r.bad_cus = f.bad;
  r.verified = f.verified;
  for (int x = 0; x < 8; ++x) r.per_xcd[x] = f.per_xcd[x];
  r.ms = c.regs.sets.end();
  return r;
}

}  // namespace regs
}  // namespace
