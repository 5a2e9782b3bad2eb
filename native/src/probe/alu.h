// Vector-ALU phase of the probe, opt-in with "aluCheck": a fixed program of vector-ALU instructions
// runs on every SIMD of every CU and each lane's result digests are compared, bit for bit, with what
// the host computed (alu_ref.h); the transcendental unit, whose approximations no standard defines,
// is compared with the device-wide consensus. Shares the HBM test's pattern_word and umin64 (hbm.h),
// the census's CU and SIMD identity (census.h) and the operand construction of alu_ref.h.
//
// Six groups, each a loop of ``iters`` steps over a per-lane 32-bit digest h (alu_ref.h has the
// arithmetic of the fold and of the operand windows, and the order of every step's results):
//   int    v_mad_u64_u32 v_mul_lo_u32 v_mul_hi_u32 v_add3_u32 v_lshl_add_u32 v_alignbit_b32 v_perm_b32
//          v_bfe_u32 v_bcnt_u32_b32 v_ffbh_u32 v_add_co_u32 + v_addc_co_u32 v_dot4_i32_i8
//   f32    v_fma_f32 v_add_f32 v_mul_f32 v_pk_fma_f32 v_pk_mul_f32 v_pk_add_f32 v_min_f32 v_max_f32
//          v_cvt_i32_f32 v_cvt_f32_i32 v_ldexp_f32 v_cmp_lt_f32 + v_cndmask_b32
//   f64    v_fma_f64 v_add_f64 v_mul_f64 v_cvt_f64_f32 v_cvt_f32_f64 v_min_f64 v_max_f64
//   f16    v_pk_fma_f16 v_pk_add_f16 v_pk_mul_f16 v_cvt_f16_f32 v_cvt_pk_bf16_f32 v_dot2c_f32_f16
//          v_dot2c_f32_bf16
//   lane   v_mov_b32_dpp (row_shr:1, row_ror:3, row_bcast:15) v_permlane32_swap v_permlane16_swap
//          ds_bpermute_b32 ds_swizzle_b32 v_readlane_b32 v_writelane_b32 v_readfirstlane_b32
//   trans  v_exp_f32 v_log_f32 v_rcp_f32 v_rsq_f32 v_sqrt_f32 v_sin_f32 v_cos_f32 v_rcp_f64 v_rsq_f64
// Every operand of step t is pattern_word(index(group, t, operand, lane), seed) ^ h with h as it stood
// when the step began, and every result is folded into h: nothing folds at compile time, nothing
// hoists out of the loop, and one wrong result changes the final digest. Inputs depend on lane,
// group, step and seed only, so every wave of a run ends with the same 6 x 64 digests.
//
// Instructions come from the builtin or the C++ operator that maps to them (contraction is off in
// the floating-point steps, so a * b + c never becomes an fma behind the reference's back), or from
// a one-instruction asm helper where nothing else names the opcode. The helpers that write VCC hold
// the reader and its wait states themselves: the compiler pads nothing inside an asm string.
//
// Verdict. Exact groups: each lane compares its five digests with the host's table; a wave counts
// its bad lanes and the lowest (CU, SIMD, group, lane) is kept by a 64-bit atomicMin. trans: a wave
// folds its 64 digests into one 64-bit value and publishes it with one atomicCAS on a slot (empty
// -> mine, the winner also stores its (CU, SIMD)); a wave whose value differs from the published one
// counts into splitWaves and keeps the first differing (CU, SIMD) by atomicMin. The kernel uses
// ordinary register counts and owns nothing, so coverage is a bit map per (CU, SIMD), 2048 x 4 bits: a
// wave whose every check passed sets its bit, a wave that failed sets it in a second, "bad" map.
//
// alu_march<true> is the test instantiation, launched only when a hook or the dump is asked for: it
// XORs one bit into the last result of one step of one group in one lane (of every wave, of one
// SIMD's or one XCD's waves) and stores workgroup 0's digests after step 0 or after the last step
// (dump stages 1 and 2) or, stage 3, the trans group's raw results: per wave, step (the first
// kTraceSteps) and lane the digest as the step began and the step's eleven result words exactly as
// they were folded, the hook's XOR included. The probe judges trans by consensus only; the trace is
// what lets the test suite compare the program with a reference of the nine functions
// (gpupool/ops/alu.py trans_reference). alu_march<false>, the production instantiation, carries none
// of it.
//
// What it cannot find: a defect of the transcendental unit common to every SIMD of the device; the
// scalar ALU; opcodes outside the groups; defects that show only at other data, clocks or
// temperatures than the run's.
#pragma once

#include <cstdint>
#include <vector>

#include "alu_ref.h"  // index, operand windows, fold; the host's expectation
#include "arena.h"    // kCuKeys
#include "census.h"   // cu_key, simd_id, decode_dump
#include "ctx.h"      // DeviceCtx, CounterSets: the phase's events, counters, expectation table and pinned result
#include "hbm.h"      // pattern_word, umin64
#include "options.h"  // alu::Plan
#include "report.h"   // AluResult
#include "types.h"

namespace {
namespace alu {

constexpr int kThreads = 256;
constexpr int kMapWords = kCuKeys * 4 / 64;  // one bit per (CU key, SIMD)
static_assert(kPlanGroups == kGroups && kPlanLanes == kLanes && kPlanSeedBase == kSeedBase, "options.h mirrors alu_ref.h");

// One set of counters; two sets, and workgroup 0 of a run resets the OTHER set (ctx.h CounterSets). The
// consensus slot (0: empty) and its publisher are part of the set.
constexpr int kSlotBadWaves = 0, kSlotBadLanes = 1, kSlotFirstBad = 2, kSlotWorkgroups = 3, kSlotWaves = 4 /* 4 of them */,
              kSlotSplit = 8, kSlotFirstSplit = 9, kSlotConsensus = 10, kSlotPublisher = 11, kSlotDumpCu = 12,
              kSlotDumpSimds = 13, kSlotOkMap = 14, kSlotBadMap = kSlotOkMap + kMapWords,
              kSlots = kSlotBadMap + kMapWords;

__host__ __device__ constexpr unsigned long long reset_value(int slot) {
  return slot == kSlotFirstBad || slot == kSlotFirstSplit || slot == kSlotPublisher || slot == kSlotDumpCu ||
                 slot == kSlotDumpSimds
             ? ~0ull
             : 0ull;
}

struct KernelArgs {
  uint32_t seed;
  int iters;
  const uint32_t* expect;  // [kExactGroups][kLanes]
  // test hooks (alu_march<true> only), out of range: off
  int flip_group;
  uint32_t flip_step, flip_lane, flip_bit;
  int fault_simd, fault_xcc;  // the flip only on this SIMD / XCD (< 0: on all)
  int dump_stage;             // 1 | 2: workgroup 0 stores its digests after step 0 / after the last step; 3: the trans trace
  uint32_t* dump;             // [4][kGroups][kLanes]
  unsigned long long* cnt;    // this run's counter set
  unsigned long long* next;   // the next run's, reset here
  uint32_t* trace;            // stage 3: [4][kTraceSteps][kTraceWords][kLanes]; last, so no other argument moves
};

// ------------------------------------------------------------------ one-instruction helpers
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;

__device__ __forceinline__ uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float f32_of(uint32_t b) { return __builtin_bit_cast(float, b); }
__device__ __forceinline__ uint32_t bits(f16x2 v) { return __builtin_bit_cast(uint32_t, v); }

__device__ __forceinline__ uint64_t mad_u64_u32(uint32_t a, uint32_t b, uint64_t c) {
  uint64_t d;
  asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c) : "vcc");
  return d;
}
__device__ __forceinline__ uint32_t add3_u32(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_add3_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ uint32_t lshl_add_u32(uint32_t a, uint32_t shift, uint32_t c) {
  uint32_t d;
  asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(shift), "v"(c));
  return d;
}
// the scalar forms by name: left to the compiler, a + d and b * c pair up into v_pk_add_f32 / v_pk_mul_f32
__device__ __forceinline__ float add_f32(float a, float b) {
  float d;
  asm("v_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ float mul_f32(float a, float b) {
  float d;
  asm("v_mul_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
// the 64-bit add as the carry pair; two wait states between the VCC write and its reader
__device__ __forceinline__ uint64_t add_co_u64(uint32_t a_hi, uint32_t a_lo, uint32_t b_hi, uint32_t b_lo) {
  uint32_t lo, hi;
  asm("v_add_co_u32 %0, vcc, %2, %3\n"
      "s_nop 1\n"
      "v_addc_co_u32 %1, vcc, %4, %5, vcc"
      : "=&v"(lo), "=&v"(hi)
      : "v"(a_lo), "v"(b_lo), "v"(a_hi), "v"(b_hi)
      : "vcc");
  return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ uint32_t cvt_pk_bf16_f32(float lo, float hi) {
  uint32_t d;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(d) : "v"(lo), "v"(hi));
  return d;
}
// v_writelane_b32 reads the SGPR a v_readlane_b32 just wrote: two wait states ahead of it
__device__ __forceinline__ uint32_t writelane(uint32_t value, uint32_t old) {
  asm("s_nop 1\n"
      "v_writelane_b32 %0, %1, %2"
      : "+v"(old)
      : "s"(value), "n"(kWriteLane));
  return old;
}
// The dot products come from their builtins: a VALU that reads a dot instruction's result needs three
// wait states after it, which the compiler pads for its own instructions and not inside an asm string.
__device__ __forceinline__ float dot2c_f32_f16(uint32_t a, uint32_t b, float acc) {
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), acc, false);
}
__device__ __forceinline__ float dot2c_f32_bf16(uint32_t a, uint32_t b, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), acc, false);
}

// ------------------------------------------------------------------ the steps
// ``hs`` is the digest as the step begins, ``f`` takes each result in alu_ref.h's order; ``flip`` is
// XORed into the last one (0 in production).
#define ALU_W(G, O) (pattern_word(index(G, t, O, lane), seed) ^ hs)

template <class F>
__device__ __forceinline__ void step_int(uint32_t hs, uint32_t t, uint32_t lane, uint32_t seed, uint32_t flip, F&& f) {
  const uint32_t a = ALU_W(kInt, 0), b = ALU_W(kInt, 1), c = ALU_W(kInt, 2), d = ALU_W(kInt, 3);
  const uint64_t mad = mad_u64_u32(a, b, (static_cast<uint64_t>(c) << 32) | d);
  f(static_cast<uint32_t>(mad));
  f(static_cast<uint32_t>(mad >> 32));
  f(a * c);
  f(__umulhi(b, d));
  f(add3_u32(a, b, c));
  f(lshl_add_u32(a, d & 7u, c));
  f(__builtin_amdgcn_alignbit(a, b, c & 31u));
  f(__builtin_amdgcn_perm(a, b, d & 0x07070707u));
  f(__builtin_amdgcn_ubfe(a, b & 31u, c & 31u));
  f(static_cast<uint32_t>(__builtin_popcount(a)) + b);
  f(a ? static_cast<uint32_t>(__builtin_clz(a)) : ~0u);
  const uint64_t sum = add_co_u64(a, b, c, d);
  f(static_cast<uint32_t>(sum));
  f(static_cast<uint32_t>(sum >> 32));
  f(static_cast<uint32_t>(__builtin_amdgcn_sdot4(static_cast<int>(a), static_cast<int>(b), static_cast<int>(c & 0xFFFFFFu), false)) ^
    flip);
}

template <class F>
__device__ __forceinline__ void step_f32(uint32_t hs, uint32_t t, uint32_t lane, uint32_t seed, uint32_t flip, F&& f) {
#pragma clang fp contract(off)
  const float a = f32_of(f32_bits(ALU_W(kF32, 0))), b = f32_of(f32_bits(ALU_W(kF32, 1))),
              c = f32_of(f32_bits(ALU_W(kF32, 2))), d = f32_of(f32_bits(ALU_W(kF32, 3)));
  const uint32_t e = ALU_W(kF32, 4);
  f(bits(__builtin_fmaf(a, b, c)));
  f(bits(add_f32(a, d)));
  f(bits(mul_f32(b, c)));
  const f32x2 pf = __builtin_elementwise_fma(f32x2{a, b}, f32x2{c, d}, f32x2{b, a});
  f(bits(pf.x));
  f(bits(pf.y));
  const f32x2 pm = f32x2{a, b} * f32x2{d, d};
  f(bits(pm.x));
  f(bits(pm.y));
  const f32x2 pa = f32x2{a, c} + f32x2{b, d};
  f(bits(pa.x));
  f(bits(pa.y));
  f(bits(__builtin_fminf(a, b)));
  f(bits(__builtin_fmaxf(c, d)));
  f(static_cast<uint32_t>(static_cast<int>(__builtin_ldexpf(a, 10))));
  f(bits(static_cast<float>(static_cast<int>(e))));
  f(bits(__builtin_ldexpf(b, static_cast<int>(e & 15u) - 8)));
  f((a < b ? bits(c) : bits(d)) ^ flip);
}

template <class F>
__device__ __forceinline__ void step_f64(uint32_t hs, uint32_t t, uint32_t lane, uint32_t seed, uint32_t flip, F&& f) {
#pragma clang fp contract(off)
  const double a = __builtin_bit_cast(double, f64_bits(ALU_W(kF64, 0), ALU_W(kF64, 1))),
               b = __builtin_bit_cast(double, f64_bits(ALU_W(kF64, 2), ALU_W(kF64, 3))),
               c = __builtin_bit_cast(double, f64_bits(ALU_W(kF64, 4), ALU_W(kF64, 5)));
  const float g = f32_of(f32_bits(ALU_W(kF64, 6)));
  auto f2 = [&](double x, uint32_t fl) {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    f(static_cast<uint32_t>(u));
    f(static_cast<uint32_t>(u >> 32) ^ fl);
  };
  f2(__builtin_fma(a, b, c), 0);
  f2(a + c, 0);
  f2(b * c, 0);
  f2(static_cast<double>(g), 0);
  f(bits(static_cast<float>(a)));
  f2(__builtin_fmin(a, b), 0);
  f2(__builtin_fmax(b, c), flip);
}

template <class F>
__device__ __forceinline__ void step_f16(uint32_t hs, uint32_t t, uint32_t lane, uint32_t seed, uint32_t flip, F&& f) {
#pragma clang fp contract(off)
  const f16x2 a = __builtin_bit_cast(f16x2, f16x2_bits(ALU_W(kF16, 0))), b = __builtin_bit_cast(f16x2, f16x2_bits(ALU_W(kF16, 1))),
              c = __builtin_bit_cast(f16x2, f16x2_bits(ALU_W(kF16, 2)));
  const float g0 = f32_of(f32_bits(ALU_W(kF16, 3))), g1 = f32_of(f32_bits(ALU_W(kF16, 4)));
  const uint32_t s = ALU_W(kF16, 5);
  f(bits(__builtin_elementwise_fma(a, b, c)));
  f(bits(a + c));
  f(bits(b * c));
  f(static_cast<uint32_t>(__builtin_bit_cast(unsigned short, static_cast<_Float16>(g0))));
  f(cvt_pk_bf16_f32(g0, g1));
  // the dot products' operands: small integers, exact in f16 and bf16, so every partial sum is exact
  const float i0 = static_cast<float>(small_int(s, 0)), i1 = static_cast<float>(small_int(s, 1)),
              i2 = static_cast<float>(small_int(s, 2)), i3 = static_cast<float>(small_int(s, 3));
  const float acc = static_cast<float>(small_acc(s));
  const uint32_t ha = bits(f16x2{static_cast<_Float16>(i0), static_cast<_Float16>(i1)}),
                 hb = bits(f16x2{static_cast<_Float16>(i2), static_cast<_Float16>(i3)});
  const uint32_t ba = (bits(i0) >> 16) | (bits(i1) & 0xFFFF0000u), bb = (bits(i2) >> 16) | (bits(i3) & 0xFFFF0000u);
  f(bits(dot2c_f32_f16(ha, hb, acc)));
  f(bits(dot2c_f32_bf16(ba, bb, acc)) ^ flip);
}

template <class F>
__device__ __forceinline__ void step_lane(uint32_t hs, uint32_t t, uint32_t lane, uint32_t seed, uint32_t flip, F&& f) {
  const uint32_t x = ALU_W(kLane, 0), y = ALU_W(kLane, 1), z = ALU_W(kLane, 2);
  const int xi = static_cast<int>(x), yi = static_cast<int>(y);
  f(static_cast<uint32_t>(__builtin_amdgcn_update_dpp(yi, xi, kDppRowShr1, 0xF, 0xF, false)));
  f(static_cast<uint32_t>(__builtin_amdgcn_update_dpp(yi, xi, kDppRowRor3, 0xF, 0xF, false)));
  f(static_cast<uint32_t>(__builtin_amdgcn_update_dpp(yi, xi, kDppRowBcast15, kBcastRowMask, 0xF, false)));
  const u32x2 s32 = __builtin_amdgcn_permlane32_swap(x, y, false, false);
  f(s32.x);
  f(s32.y);
  const u32x2 s16 = __builtin_amdgcn_permlane16_swap(x, z, false, false);
  f(s16.x);
  f(s16.y);
  f(static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(static_cast<int>((z & 63u) << 2), xi)));
  f(static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(yi, kSwizzle)));
  const uint32_t s = static_cast<uint32_t>(__builtin_amdgcn_readlane(xi, static_cast<int>(read_lane(t))));
  f(writelane(s, x));
  f(s);
  f(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(yi)) ^ flip);
}

template <class F>
__device__ __forceinline__ void step_trans(uint32_t hs, uint32_t t, uint32_t lane, uint32_t seed, uint32_t flip, F&& f) {
  const float a = f32_of(f32_bits(ALU_W(kTrans, 0))), b = f32_of(f32_bits(ALU_W(kTrans, 1)));
  const double q = __builtin_bit_cast(double, f64_bits(ALU_W(kTrans, 2), ALU_W(kTrans, 3)));
  f(bits(__builtin_amdgcn_exp2f(a)));
  f(bits(__builtin_amdgcn_logf(__builtin_fabsf(b))));
  f(bits(__builtin_amdgcn_rcpf(a)));
  f(bits(__builtin_amdgcn_rsqf(__builtin_fabsf(b))));
  f(bits(__builtin_amdgcn_sqrtf(__builtin_fabsf(a))));
  f(bits(__builtin_amdgcn_sinf(a)));
  f(bits(__builtin_amdgcn_cosf(b)));
  const uint64_t r = __builtin_bit_cast(uint64_t, __builtin_amdgcn_rcp(q));
  f(static_cast<uint32_t>(r));
  f(static_cast<uint32_t>(r >> 32));
  const uint64_t rs = __builtin_bit_cast(uint64_t, __builtin_amdgcn_rsq(__builtin_fabs(q)));
  f(static_cast<uint32_t>(rs));
  f(static_cast<uint32_t>(rs >> 32) ^ flip);
}
#undef ALU_W

template <int kGroup, class F>
__device__ __forceinline__ void step(uint32_t hs, uint32_t t, uint32_t lane, uint32_t seed, uint32_t flip, F&& f) {
  if constexpr (kGroup == kInt) step_int(hs, t, lane, seed, flip, f);
  else if constexpr (kGroup == kF32) step_f32(hs, t, lane, seed, flip, f);
  else if constexpr (kGroup == kF64) step_f64(hs, t, lane, seed, flip, f);
  else if constexpr (kGroup == kF16) step_f16(hs, t, lane, seed, flip, f);
  else if constexpr (kGroup == kLane) step_lane(hs, t, lane, seed, flip, f);
  else step_trans(hs, t, lane, seed, flip, f);
}

// One group's loop: the digest after ``iters`` steps; ``first`` gets the digest after step 0. ``trace``
// (test instantiation, trans group, else null): this thread's word 0 of step 0 of its wave's trace.
template <int kGroup, bool kTest>
__device__ __forceinline__ uint32_t run_group(const KernelArgs& a, uint32_t lane, uint32_t fmask, uint32_t* first,
                                              uint32_t* trace = nullptr) {
  constexpr bool kTraced = kTest && kGroup == kTrans;
  uint32_t h = 0;
#pragma unroll 1
  for (int t = 0; t < a.iters; ++t) {
    uint32_t flip = 0;
    if constexpr (kTest) flip = a.flip_group == kGroup && static_cast<uint32_t>(t) == a.flip_step ? fmask : 0u;
    const uint32_t hs = h;
    uint32_t* row = nullptr;  // the next word of this step's [kTraceWords][kLanes]
    if constexpr (kTraced) {
      if (trace && t < kTraceSteps) {
        row = trace + static_cast<size_t>(t) * kTraceWords * kLanes;
        *row = hs;
        row += kLanes;
      }
    }
    step<kGroup>(hs, static_cast<uint32_t>(t), lane, a.seed, flip, [&](uint32_t r) {
      h = fold(h, r);
      if constexpr (kTraced) {
        if (row) {
          *row = r;
          row += kLanes;
        }
      }
    });
    if constexpr (kTest)
      if (t == 0) *first = h;
  }
  return h;
}

template <bool kTest>
__global__ __launch_bounds__(kThreads) void alu_march(const KernelArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t b = blockIdx.x;
  if (b == 0)
    for (int i = static_cast<int>(tid); i < kSlots; i += kThreads) a.next[i] = reset_value(i);
  const int k = cu_key();
  const uint32_t simd = simd_id();
  uint32_t fmask = 0;
  if constexpr (kTest) {
    const bool hit = lane == a.flip_lane && (a.fault_simd < 0 || static_cast<int>(simd) == a.fault_simd) &&
                     (a.fault_xcc < 0 || (k >> 8) == a.fault_xcc);
    fmask = hit ? 1u << (a.flip_bit & 31u) : 0u;
  }
  uint32_t h[kGroups], first[kGroups] = {};
  h[kInt] = run_group<kInt, kTest>(a, lane, fmask, &first[kInt]);
  h[kF32] = run_group<kF32, kTest>(a, lane, fmask, &first[kF32]);
  h[kF64] = run_group<kF64, kTest>(a, lane, fmask, &first[kF64]);
  h[kF16] = run_group<kF16, kTest>(a, lane, fmask, &first[kF16]);
  h[kLane] = run_group<kLane, kTest>(a, lane, fmask, &first[kLane]);
  uint32_t* trace = nullptr;
  if constexpr (kTest)
    if (b == 0 && a.dump_stage == 3) trace = a.trace + static_cast<size_t>(wave) * kTraceSteps * kTraceWords * kLanes + lane;
  h[kTrans] = run_group<kTrans, kTest>(a, lane, fmask, &first[kTrans], trace);

  // ---- exact groups against the host's table: the lowest group that differs in this lane
  uint32_t bad_group = ~0u;
#pragma unroll
  for (int g = kExactGroups - 1; g >= 0; --g)
    if (h[g] != a.expect[g * kLanes + lane]) bad_group = static_cast<uint32_t>(g);
  const bool bad = bad_group != ~0u;
  const unsigned long long bad_mask = __ballot(bad);
  // (CU key << 32) | SIMD << 16 | group << 8 | lane of the lowest mismatch
  uint64_t key = bad ? (static_cast<uint64_t>(k) << 32) | (simd << 16) | (bad_group << 8) | lane : ~0ull;
  // ---- trans: the wave's 64 digests as one 64-bit value (a sum, so the butterfly's order is free)
  uint64_t tv = wave_term(h[kTrans], lane);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    key = umin64(key, static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(key), off, 64)));
    tv += static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(tv), off, 64));
  }
  if (tv == 0) tv = 1;  // 0 is the empty slot

  if constexpr (kTest) {
    if (b == 0 && (a.dump_stage == 1 || a.dump_stage == 2)) {
#pragma unroll
      for (int g = 0; g < kGroups; ++g)
        a.dump[(wave * kGroups + g) * kLanes + lane] = a.dump_stage == 1 ? first[g] : h[g];
    }
  }

  if (lane == 0) {
    const unsigned long long wkey = (static_cast<unsigned long long>(k) << 2) | simd;
    // one atomicCAS publishes (empty -> mine); a wave that already sees a value only reads the slot
    unsigned long long seen = __hip_atomic_load(&a.cnt[kSlotConsensus], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == 0ull) seen = atomicCAS(&a.cnt[kSlotConsensus], 0ull, static_cast<unsigned long long>(tv));
    bool split = false;
    if (seen == 0ull) {
      atomicMin(&a.cnt[kSlotPublisher], wkey);  // the one winner: the slot held all-ones
    } else if (seen != tv) {
      split = true;
      atomicAdd(&a.cnt[kSlotSplit], 1ull);
      atomicMin(&a.cnt[kSlotFirstSplit], wkey);
    }
    if (bad_mask) {
      atomicAdd(&a.cnt[kSlotBadWaves], 1ull);
      atomicAdd(&a.cnt[kSlotBadLanes], static_cast<unsigned long long>(__builtin_popcountll(bad_mask)));
      atomicMin(&a.cnt[kSlotFirstBad], static_cast<unsigned long long>(key));
    }
    const int bit = k * 4 + static_cast<int>(simd);  // < kCuKeys * 4
    atomicOr(&a.cnt[(bad_mask || split ? kSlotBadMap : kSlotOkMap) + (bit >> 6)], 1ull << (bit & 63));
    atomicAdd(&a.cnt[kSlotWaves + simd], 1ull);
    if (wave == 0) atomicAdd(&a.cnt[kSlotWorkgroups], 1ull);
    if constexpr (kTest) {
      if (b == 0 && a.dump_stage) {
        atomicMin(&a.cnt[kSlotDumpCu], static_cast<unsigned long long>(k));
        // each wave of workgroup 0 clears its own byte of the all-ones word and leaves its SIMD there
        atomicAnd(&a.cnt[kSlotDumpSimds], ~(0xFFull << (8 * wave)) | (static_cast<unsigned long long>(simd) << (8 * wave)));
      }
    }
  }
}

// ------------------------------------------------------------------ the phase: ensure / launch / finish
// Makes the phase's expectation table and counter sets (and, for dump stage 1 | 2, the device copy of
// one workgroup's digests, 3, of its trans trace), puts both sets at their reset values unless the
// last run left them so, and computes and uploads the host's expectation when (seed, steps) is not
// the pair the table holds. All of it ahead of the probe's clock.
inline void ensure(DeviceCtx& c, const Plan& pl) {
  auto& x = c.alu;
  if (!x.exp) PROBE_CHECK(hipMalloc(reinterpret_cast<void**>(&x.exp), kExactGroups * kLanes * sizeof(uint32_t)));
  x.sets.make(kSlots);
  const bool stale = x.exp_iters != pl.iters || x.exp_seed != pl.seed;
  // first use, a run that never reached finish(), or a table a run may still read
  if (!x.sets.clean || stale) sync_streams(c);
  if (!x.sets.clean) x.sets.reset<kSlots>(reset_value);
  if (stale) {
    uint32_t table[kExactGroups * kLanes];
    expected(pl.seed, pl.iters, table);
    x.exp_iters = 0;
    PROBE_CHECK(hipMemcpy(x.exp, table, sizeof table, hipMemcpyHostToDevice));
    x.exp_seed = pl.seed;
    x.exp_iters = pl.iters;
  }
  if ((pl.dump_stage == 1 || pl.dump_stage == 2) && !x.dump) PROBE_CHECK(hipMalloc(&x.dump, kDumpBytes));
  if (pl.dump_stage == 3 && !x.trace) PROBE_CHECK(hipMalloc(&x.trace, kTraceBytes));
}

// Enqueues the phase on stream s: an event, the kernel, an event, the counters' copy. No host synchronise.
inline void launch(DeviceCtx& c, hipStream_t s, const Plan& pl) {
  auto& x = c.alu;
  KernelArgs a{};
  a.seed = pl.seed;
  a.iters = pl.iters;
  a.expect = x.exp;
  a.flip_group = pl.flip_group;
  a.flip_step = pl.flip_group >= 0 ? static_cast<uint32_t>(pl.flip_step) : ~0u;
  a.flip_lane = pl.flip_group >= 0 ? static_cast<uint32_t>(pl.flip_lane) : ~0u;
  a.flip_bit = pl.flip_group >= 0 ? static_cast<uint32_t>(pl.flip_bit) : 0u;
  a.fault_simd = pl.fault_simd;
  a.fault_xcc = pl.fault_xcc;
  // a stage without its buffer (a probe, which has no caller buffer) is off
  a.dump_stage = (pl.dump_stage == 3 ? x.trace : x.dump) ? pl.dump_stage : 0;
  a.dump = static_cast<uint32_t*>(x.dump);
  a.trace = static_cast<uint32_t*>(x.trace);
  const int grid = pl.blocks_per_cu * c.prop.multiProcessorCount;
  // the trace holds the first min(iters, kTraceSteps) steps; what the run does not write reads as zero
  if (a.dump_stage == 3) PROBE_CHECK(hipMemsetAsync(x.trace, 0, kTraceBytes, s));
  x.sets.run(s, kSlots, [&](unsigned long long* cnt, unsigned long long* next) {
    a.cnt = cnt;
    a.next = next;
    if (pl.test_kernel()) hipLaunchKernelGGL(alu_march<true>, dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(alu_march<false>, dim3(grid), dim3(kThreads), 0, s, a);
  });
}

// After the stream's synchronise: the counters -> the "alu" block's result.
inline AluResult finish(DeviceCtx& c, const Plan& pl, bool require_all) {
  AluResult r;
  const unsigned long long* h = c.alu.sets.res;
  r.iters = pl.iters;
  r.expected = c.prop.multiProcessorCount;
  r.require_all = require_all;
  r.workgroups = h[kSlotWorkgroups];
  for (int s = 0; s < 4; ++s) r.waves_per_simd[s] = h[kSlotWaves + s];
  r.bad_waves = h[kSlotBadWaves];
  r.bad_lanes = h[kSlotBadLanes];
  r.first_bad = h[kSlotFirstBad];
  r.split_waves = h[kSlotSplit];
  r.trans_digest = h[kSlotConsensus];
  if (r.split_waves) {  // more than half of the waves differ from the published value: the publisher is the odd one
    const unsigned long long who = 2 * r.split_waves > r.waves() ? h[kSlotPublisher] : h[kSlotFirstSplit];
    r.suspect = who == ~0ull ? -1 : static_cast<long long>(who);
  }
  if (pl.dump_stage) decode_dump(h[kSlotDumpCu], h[kSlotDumpSimds], &r.dump_cu, r.dump_simds);
  for (int w = 0; w < kMapWords; ++w) {
    const unsigned long long ok = h[kSlotOkMap + w], bad = h[kSlotBadMap + w], ver = ok & ~bad;
    r.simds_tested += __builtin_popcountll(ok | bad);
    r.simds_verified += __builtin_popcountll(ver);
    r.per_xcd[(w * 16) >> 8] += __builtin_popcountll(ver);  // 16 CU keys per word, 256 per XCD
    for (int cu = 0; cu < 16; ++cu) {
      if (((ver >> (4 * cu)) & 15ull) == 15ull) ++r.cus_verified;
      if ((bad >> (4 * cu)) & 15ull) ++r.bad_cus;
    }
  }
  r.ms = c.alu.sets.end();
  return r;
}

}  // namespace alu
}  // namespace
