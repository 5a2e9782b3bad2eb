// Host reference of the atomic-unit phase ("atomCheck", atomics.h): the layout, the operand
// construction the kernels share (ATOM_HD, so one text serves both sides) and the expected final
// values and return digests computed on the CPU. Pure host code when compiled by plain g++
// (native/tests/test_atomics_spec.cc), like alu_ref.h. gpupool/ops/atomics.py is the independent twin.
//
// Ops. 17 contended ops, every wave of a workgroup (lds, l2) or of a population of workgroups (dev)
// hitting slot = lane of the op's row, all commutative, so the final value does not depend on the
// arrival order:
//    0 add  1 sub  2 and  3 or  4 xor  5 umin  6 umax  7 smin  8 smax  9 add_f32  10 pk_add_f16
//   11 pk_add_bf16                                                        (4-byte slots)
//   12 add_x2  13 umax_x2  14 xor_x2  15 add_f64  16 max_f64              (8-byte slots)
// and 5 returning ops on words private to a (wave, lane), where the value returned at step t is
// exactly the value after step t - 1:
//   17 add_rtn  18 inc  19 dec  20 swap  21 cas
// Pseudo-ops in a fault's name: 22 ticket (the LDS ticket test), 23 returns (a lane's return digest).
//
// A row-set is one row of 64 slots per contended op: 12 x 64 + 5 x 128 = 1408 words. A region (the
// LDS table, a workgroup's private global region) is a row-set followed by the private words
// [5 ops][4 waves][64 lanes] = 1280 words: 2688 words, 2368 slots (slot numbering: slot_word()).
//
// Operands. raw(layer, op, step, wave, lane) = mix(index, seed), two words for the 8-byte ops, where
//   index = layer << 40 | op << 32 | step << 10 | part << 8 | wave << 6 | lane
// and mix is hbm.h's pattern_word. arg() turns the raw integer into the operand (a test flip is made
// in raw, before it): add sub xor umin umax smin smax add_x2 umax_x2 xor_x2 take it whole; and takes
// w | rotl(w, 13), or takes w & rotl(w, 13); the floating-point adds take small integers, so that
// every partial sum in every arrival order is exactly representable: add_f32 w & 3, add_f64 w & 7,
// max_f64 w & 0xFFFFF, the packed adds one bit per half (1.0 or 0.0). In the dev layer and / or take
// the workgroup's own bit instead (workgroup b owns bit b % 32 of slot (b / 32) % 64) and arrive once
// per workgroup (wave 0, step 0); the packed rows receive only from wave 0 at step 0 of workgroups
// b < 256 (bound: sum <= 256, exact in bf16); and in the min / max family the operand of wave 0 at step
// 0 is the workgroup's own, mix(index | (b + 1) << 44, seed), so that a slot's extreme comes from a
// workgroup the twin can name. Layer 3 (kLds16) is the lds layer's second addressing: the contended
// ops on slot = lane & 15 of a row-set of its own, its packed rows only in the first 16 steps.
// Returning ops: add_rtn adds w; inc / dec wrap at limit w & 7; swap stores w; cas first compares with
// the value the program itself tracks (stored on success: w) and then with ~w, which must fail.
// A lane's digest folds, per step, the six returns in the order add_rtn inc dec swap cas cas with
// alu_ref.h's fold, h = (rotl(h, 5) ^ r) * 0x9E3779B1.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define ATOM_HD __host__ __device__ inline
#else
#define ATOM_HD inline
#endif

namespace {
namespace atom {

constexpr int kLanes = 64, kWaves = 4, kThreadsPerWg = 256;
// kLds16 is no layer of the mask: it names the lds layer's second addressing (slot = lane & 15, four
// lanes of a wave on one word) as an operand stream and in a test hook
enum Layer { kLds = 0, kL2 = 1, kDev = 2, kLayers = 3, kLds16 = 3, kHookLayers = 4 };
constexpr int kSlots16 = 16;  // the second addressing's slots per row; a fault there is slot 64 + (lane & 15)
constexpr int kPackedSteps16 = 16;  // second addressing: only the first 16 steps add to the packed rows
constexpr const char* kLayerNames[kLayers] = {"lds", "l2", "dev"};
enum Op {
  kAdd = 0, kSub, kAnd, kOr, kXor, kUmin, kUmax, kSmin, kSmax, kAddF32, kPkF16, kPkBf16,
  kAdd64, kUmax64, kXor64, kAddF64, kMaxF64,
  kRetAdd, kRetInc, kRetDec, kRetSwap, kRetCas,
  kTicket, kReturns, kOpNames
};
constexpr int kOps4 = 12, kOps = 17, kRetOps = 5, kAllOps = 22;
constexpr const char* kOpNameTable[kOpNames] = {
    "add", "sub", "and", "or", "xor", "umin", "umax", "smin", "smax", "add_f32", "pk_add_f16", "pk_add_bf16",
    "add_x2", "umax_x2", "xor_x2", "add_f64", "max_f64", "add_rtn", "inc", "dec", "swap", "cas", "ticket", "returns"};
constexpr uint32_t kSeedBase = 0x41544D00u;  // the phase's seed is kSeedBase + HIP device ordinal
constexpr uint32_t kFoldMul = 0x9E3779B1u;

constexpr int kRowSetWords = kOps4 * kLanes + (kOps - kOps4) * 2 * kLanes;  // 1408
constexpr int kPrivWords = kRetOps * kWaves * kLanes;                        // 1280
constexpr int kRegionWords = kRowSetWords + kPrivWords;                      // 2688
constexpr int kRowSetSlots = kOps * kLanes;                                  // 1088
constexpr int kRegionSlots = kRowSetSlots + kPrivWords;                      // 2368
constexpr int kDevRowSets = 9;  // 0..7 the XCD's own, 8 the one every workgroup hits
constexpr int kAllXcd = 8;
constexpr int kDigestWords = kWaves * kLanes;
constexpr int kPackedWorkgroups = 256;  // dev: only workgroups below it add to the packed rows
constexpr int kMaxWorkgroups = 16 * 256, kRefMaxIters = 64;
// the exactness bounds: the largest partial sum of each floating-point add at the extreme plan
constexpr long long kMaxSumF32 = 3LL * kWaves * kRefMaxIters * kMaxWorkgroups;  // < 2^24
constexpr long long kMaxSumF64 = 7LL * kWaves * kRefMaxIters * kMaxWorkgroups;  // < 2^53
constexpr long long kMaxSumPacked = kWaves * kRefMaxIters;  // lds, l2: 256; dev: kPackedWorkgroups
constexpr long long kMaxSumPacked16 = 4LL * kWaves * kPackedSteps16;  // four lanes of each wave on a word: 256
static_assert(kMaxSumF32 < (1LL << 24) && kMaxSumF64 < (1LL << 53) && kMaxSumPacked <= 256 && kPackedWorkgroups <= 256 &&
                  kMaxSumPacked16 <= 256,
              "every partial sum must be exactly representable");

// the expectation table the host uploads, in words
constexpr int kExpLds = 0, kExpL2 = kRegionWords, kExpDev = 2 * kRegionWords, kExpLdsDigest = kExpDev + kRowSetWords,
              kExpL2Digest = kExpLdsDigest + kDigestWords, kExpLds16 = kExpL2Digest + kDigestWords,  // a row-set
              kExpWords = kExpLds16 + kRowSetWords;
// workgroup 0's dump (mi355x_probe_atomics), in words: its LDS region, its two digest sets, its
// private region and the nine dev row-sets as atom_verify read them, and every workgroup's CU key
constexpr int kDumpLds = 0, kDumpLdsDigest = kRegionWords, kDumpL2Digest = kDumpLdsDigest + kDigestWords,
              kDumpRegion = kDumpL2Digest + kDigestWords, kDumpDev = kDumpRegion + kRegionWords,
              kDumpRecords = kDumpDev + kDevRowSets * kRowSetWords,  // the CU key of each workgroup's record
              kDumpLds16 = kDumpRecords + kMaxWorkgroups,  // the second addressing's LDS row-set
              kDumpWords = kDumpLds16 + kRowSetWords;

// hbm.h's pattern_word, restated for the host-only build (test_atomics_spec.cc pins it)
ATOM_HD uint32_t mix(uint64_t idx, uint32_t seed) {
  uint32_t x = static_cast<uint32_t>(idx) * 0x9E3779B1u ^ static_cast<uint32_t>(idx >> 32) * 0x85EBCA77u;
  x ^= seed;
  x ^= x >> 15;
  x *= 0x2C1B3C6Du;
  x ^= x >> 12;
  return x;
}
ATOM_HD uint32_t fold(uint32_t h, uint32_t r) { return (((h << 5) | (h >> 27)) ^ r) * kFoldMul; }
ATOM_HD uint32_t rotl13(uint32_t w) { return (w << 13) | (w >> 19); }

ATOM_HD bool wide(int op) { return op >= kOps4 && op < kOps; }
// first word of a contended op's row inside a row-set
ATOM_HD int row_word(int op) { return op < kOps4 ? op * kLanes : kOps4 * kLanes + (op - kOps4) * 2 * kLanes; }
// first word of a returning op's private words inside a region
ATOM_HD int priv_word(int op, int wave, int lane) { return kRowSetWords + ((op - kOps) * kWaves + wave) * kLanes + lane; }
// slot j of a region: its first word, its op and its index inside the op (lane, or wave * 64 + lane)
ATOM_HD int slot_word(int j) {
  return j < kOps4 * kLanes ? j : j < kRowSetSlots ? kOps4 * kLanes + (j - kOps4 * kLanes) * 2 : kRowSetWords + (j - kRowSetSlots);
}
ATOM_HD int slot_op(int j) { return j < kRowSetSlots ? j / kLanes : kOps + (j - kRowSetSlots) / (kWaves * kLanes); }
ATOM_HD int slot_index(int j) { return j < kRowSetSlots ? j % kLanes : (j - kRowSetSlots) % (kWaves * kLanes); }
// the value a slot holds before a run and after atom_verify: the op's identity
ATOM_HD uint64_t identity(int op) {
  return op == kAnd || op == kUmin ? 0xFFFFFFFFull : op == kSmin ? 0x7FFFFFFFull : op == kSmax ? 0x80000000ull : 0ull;
}
ATOM_HD uint32_t init_word(int w) {  // word w of a region
  if (w >= kOps4 * kLanes) return 0u;
  return static_cast<uint32_t>(identity(w / kLanes));
}

ATOM_HD uint64_t index(int layer, int op, uint32_t step, int part, uint32_t wave, uint32_t lane) {
  return (static_cast<uint64_t>(layer) << 40) | (static_cast<uint64_t>(op) << 32) | (static_cast<uint64_t>(step) << 10) |
         (static_cast<uint64_t>(part) << 8) | (static_cast<uint64_t>(wave) << 6) | lane;
}
ATOM_HD uint64_t raw(int layer, int op, uint32_t step, uint32_t wave, uint32_t lane, uint32_t seed) {
  const uint64_t lo = mix(index(layer, op, step, 0, wave, lane), seed);
  return wide(op) ? (static_cast<uint64_t>(mix(index(layer, op, step, 1, wave, lane), seed)) << 32) | lo : lo;
}
// dev layer, and / or: workgroup b's own bit
ATOM_HD uint64_t dev_bit_raw(int op, uint32_t b, uint32_t lane) {
  const uint32_t bit = lane == ((b >> 5) & 63u) ? 1u << (b & 31u) : 0u;
  return op == kAnd ? ~bit : bit;
}
// dev layer, the min / max family: the operand wave 0 sends at step 0 is the workgroup's own
ATOM_HD bool dev_own(int op) { return op == kUmin || op == kUmax || op == kSmin || op == kSmax || op == kUmax64 || op == kMaxF64; }
ATOM_HD uint64_t dev_own_raw(int op, uint32_t b, uint32_t lane, uint32_t seed) {
  const uint64_t who = static_cast<uint64_t>(b + 1u) << 44;
  const uint64_t lo = mix(index(kDev, op, 0, 0, 0, lane) | who, seed);
  return wide(op) ? (static_cast<uint64_t>(mix(index(kDev, op, 0, 1, 0, lane) | who, seed)) << 32) | lo : lo;
}
// the min / max family on integers (max_f64's operands are non-negative integers until the end)
ATOM_HD uint64_t extreme(int op, uint64_t x, uint64_t y) {
  switch (op) {
    case kUmin: return x < y ? x : y;
    case kSmin: return static_cast<int32_t>(x) < static_cast<int32_t>(y) ? x : y;
    case kSmax: return static_cast<int32_t>(x) > static_cast<int32_t>(y) ? x : y;
    default: return x > y ? x : y;
  }
}
// raw integer -> operand (for the floating-point ops the small integer, for the packed ones bit 0 /
// bit 1 = the low / high half's 1.0)
ATOM_HD uint64_t arg(int layer, int op, uint64_t w) {
  const uint32_t w32 = static_cast<uint32_t>(w);
  switch (op) {
    case kAnd: return layer == kDev ? w32 : (w32 | rotl13(w32));
    case kOr: return layer == kDev ? w32 : (w32 & rotl13(w32));
    case kAddF32: return w32 & 3u;
    case kPkF16:
    case kPkBf16: return w32 & 3u;
    case kAddF64: return w & 7ull;
    case kMaxF64: return w & 0xFFFFFull;
    case kRetInc:
    case kRetDec: return w32 & 7u;
    default: return wide(op) ? w : w32;
  }
}
// does (wave, step, workgroup) issue this contended op in this layer?
ATOM_HD bool issues(int layer, int op, uint32_t step, uint32_t wave, uint32_t b) {
  const bool packed = op == kPkF16 || op == kPkBf16;
  if (layer == kDev && (packed || op == kAnd || op == kOr))  // one arrival per workgroup: its own bit, or its one packed add
    return wave == 0 && step == 0 && (!packed || b < static_cast<uint32_t>(kPackedWorkgroups));
  if (layer == kLds16 && packed) return step < static_cast<uint32_t>(kPackedSteps16);
  return true;
}
// a non-negative integer n <= 2^(mant + 1) as a binary floating-point number of ``mant`` mantissa bits
ATOM_HD uint32_t int_to_fp(uint32_t n, int mant, int bias) {
  if (n == 0) return 0;
  int e = 31;
  while (!((n >> e) & 1u)) --e;
  const uint32_t m = e <= mant ? n << (mant - e) : n >> (e - mant);
  return (static_cast<uint32_t>(e + bias) << mant) | (m & ((1u << mant) - 1u));
}
ATOM_HD uint32_t packed_bits(int op, uint32_t lo, uint32_t hi) {
  return op == kPkF16 ? int_to_fp(lo, 10, 15) | (int_to_fp(hi, 10, 15) << 16) : int_to_fp(lo, 7, 127) | (int_to_fp(hi, 7, 127) << 16);
}
// one returning op as the hardware defines it: the new value of ``v`` (the old one is returned)
ATOM_HD uint32_t ret_apply(int op, uint32_t v, uint32_t a) {
  switch (op) {
    case kRetAdd: return v + a;
    case kRetInc: return v >= a ? 0u : v + 1u;
    case kRetDec: return (v == 0u || v > a) ? a : v - 1u;
    default: return a;  // swap
  }
}
// the lowest fault's key: layer, op, slot index, row (XCD 0..7, 8 = the all-XCD row; lds / l2: the CU's XCD), CU key
ATOM_HD uint64_t fault_key(int layer, int op, int slot, int xcc, int cu) {
  return (static_cast<uint64_t>(layer) << 60) | (static_cast<uint64_t>(op) << 52) | (static_cast<uint64_t>(slot) << 36) |
         (static_cast<uint64_t>(xcc) << 32) | static_cast<uint32_t>(cu);
}

// ------------------------------------------------------------------ host side

// a test hook as the kernel applies it: on wave 0 of the struck workgroups (-1: off)
struct Hook {
  int skip_layer = -1, skip_op = -1, skip_step = -1, skip_lane = -1;
  int flip_layer = -1, flip_op = -1, flip_step = -1, flip_lane = -1, flip_bit = 0;
  bool skips(int layer, int op, int step, int wave, int lane) const {
    return wave == 0 && layer == skip_layer && op == skip_op && (step == skip_step || op == kTicket) && lane == skip_lane;
  }
  uint64_t flips(int layer, int op, int step, int wave, int lane) const {
    return wave == 0 && layer == flip_layer && op == flip_op && step == flip_step && lane == flip_lane ? 1ull << flip_bit : 0ull;
  }
};

// accumulator of one contended slot in exact integers
struct Acc {
  uint64_t v = 0;
  uint64_t lo = 0, hi = 0;  // the packed halves
  void start(int op) { v = identity(op), lo = hi = 0; }
  void apply(int op, uint64_t a) {
    switch (op) {
      case kAdd: v = static_cast<uint32_t>(v + a); break;
      case kSub: v = static_cast<uint32_t>(v - a); break;
      case kAnd: v &= a; break;
      case kOr: v |= a; break;
      case kXor: case kXor64: v ^= a; break;
      case kUmin: v = std::min(v, a); break;
      case kUmax: case kUmax64: case kMaxF64: v = std::max(v, a); break;
      case kSmin: v = static_cast<uint32_t>(std::min(static_cast<int32_t>(v), static_cast<int32_t>(a))); break;
      case kSmax: v = static_cast<uint32_t>(std::max(static_cast<int32_t>(v), static_cast<int32_t>(a))); break;
      case kPkF16: case kPkBf16: lo += a & 1u, hi += (a >> 1) & 1u; break;
      default: v += a; break;  // add_f32, add_x2, add_f64: integer sums
    }
  }
};
inline uint64_t f64_bits_of(uint64_t n) {
  const double d = static_cast<double>(n);
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}
inline uint32_t f32_bits_of(uint32_t n) {
  const float f = static_cast<float>(n);
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}
// the slot's final contents out of its accumulator
inline uint64_t acc_bits(int op, const Acc& a) {
  switch (op) {
    case kAddF32: return f32_bits_of(static_cast<uint32_t>(a.v));
    case kAddF64: case kMaxF64: return f64_bits_of(a.v);
    case kPkF16: case kPkBf16: return packed_bits(op, static_cast<uint32_t>(a.lo), static_cast<uint32_t>(a.hi));
    default: return a.v;
  }
}
inline void put_slot(uint32_t* region, int op, int lane, uint64_t bits) {
  uint32_t* p = region + row_word(op) + (wide(op) ? 2 * lane : lane);
  p[0] = static_cast<uint32_t>(bits);
  if (wide(op)) p[1] = static_cast<uint32_t>(bits >> 32);
}

// One workgroup's region (layer lds or l2) after ``iters`` steps and its lanes' return digests
// [wave][lane], with ``hook`` applied when given.
inline void region_expected(int layer, uint32_t seed, int iters, uint32_t* region, uint32_t* digest, const Hook* hook = nullptr) {
  const Hook none;
  const Hook& hk = hook ? *hook : none;
  for (int op = 0; op < kOps; ++op)
    for (int lane = 0; lane < kLanes; ++lane) {
      Acc a;
      a.start(op);
      for (int t = 0; t < iters; ++t)
        for (int w = 0; w < kWaves; ++w) {
          if (hk.skips(layer, op, t, w, lane)) continue;
          a.apply(op, arg(layer, op, raw(layer, op, t, w, lane, seed) ^ hk.flips(layer, op, t, w, lane)));
        }
      put_slot(region, op, lane, acc_bits(op, a));
    }
  for (int w = 0; w < kWaves; ++w)
    for (int lane = 0; lane < kLanes; ++lane) {
      uint32_t v[kRetOps] = {}, h = 0;
      uint32_t cur = 0;  // what the program believes the cas word holds
      for (int t = 0; t < iters; ++t)
        for (int op = kRetAdd; op <= kRetCas; ++op) {
          uint32_t& m = v[op - kRetAdd];
          const uint32_t a = static_cast<uint32_t>(arg(layer, op, raw(layer, op, t, w, lane, seed) ^ hk.flips(layer, op, t, w, lane)));
          const bool skip = hk.skips(layer, op, t, w, lane);
          if (op != kRetCas) {
            if (skip) continue;  // nothing issued, nothing folded
            h = fold(h, m);
            m = ret_apply(op, m, a);
            continue;
          }
          const uint32_t clean = static_cast<uint32_t>(raw(layer, op, t, w, lane, seed));
          if (!skip) {  // the skip drops the first cas only
            h = fold(h, m);
            if (m == cur) m = a;
          }
          cur = clean;
          h = fold(h, m);  // compare ~clean against the word: fails while the word holds clean
          if (m == ~clean) m = clean ^ 0x5A5A5A5Au;
        }
      digest[w * kLanes + lane] = h;
      for (int op = kRetAdd; op <= kRetCas; ++op) region[priv_word(op, w, lane)] = v[op - kRetAdd];
    }
}

// The lds layer's second addressing: a row-set of which slots 0..15 of every row receive the four
// lanes j, j + 16, j + 32, j + 48 of every wave; the other slots keep their initial value.
inline void lds16_expected(uint32_t seed, int iters, uint32_t* rowset, const Hook* hook = nullptr) {
  const Hook none;
  const Hook& hk = hook ? *hook : none;
  for (int i = 0; i < kRowSetWords; ++i) rowset[i] = init_word(i);
  for (int op = 0; op < kOps; ++op)
    for (int j = 0; j < kSlots16; ++j) {
      Acc a;
      a.start(op);
      for (int t = 0; t < iters; ++t)
        for (int w = 0; w < kWaves; ++w)
          for (int lane = j; lane < kLanes; lane += kSlots16) {
            if (!issues(kLds16, op, t, w, 0) || hk.skips(kLds16, op, t, w, lane)) continue;
            a.apply(op, arg(kLds16, op, raw(kLds16, op, t, w, lane, seed) ^ hk.flips(kLds16, op, t, w, lane)));
          }
      put_slot(rowset, op, j, acc_bits(op, a));
    }
}

// The dev layer's base table, a row-set: per slot what ONE workgroup contributes over all its waves
// and steps (add sub add_x2: the sum; xor: the xor; min / max: the extreme, max_f64 as double bits;
// add_f32 add_f64: the integer sum; packed: bit 0 / 1 = the halves wave 0 adds at step 0; and / or:
// unused, they come from the records). atom_verify combines it with the population's size.
inline void dev_base(uint32_t seed, int iters, uint32_t* rowset) {
  for (int op = 0; op < kOps; ++op)
    for (int lane = 0; lane < kLanes; ++lane) {
      Acc a;
      const int as = op == kSub ? kAdd : op;  // sub: the sum, which dev_combine subtracts n times
      a.start(as);
      if (op != kAnd && op != kOr)
        for (int t = 0; t < iters; ++t)
          for (int w = 0; w < kWaves; ++w)
            if (issues(kDev, op, t, w, 0) && !(dev_own(op) && t == 0 && w == 0))  // that one is the workgroup's own
              a.apply(as, arg(kDev, op, raw(kDev, op, t, w, lane, seed)));
      uint64_t bits = a.v;  // max_f64: the integer, dev_own_combine converts
      if (op == kPkF16 || op == kPkBf16) bits = a.lo | (a.hi << 1);
      put_slot(rowset, op, lane, bits);
    }
}

// The min / max family of the dev layer: the base table's extreme of the operands every workgroup
// shares, folded with ``own``, the extreme of the population's own operands (both integers).
ATOM_HD uint64_t dev_own_combine(int op, uint64_t base, uint32_t n, uint64_t own) {
  if (!n) return identity(op);
  const uint64_t v = extreme(op, base, own);
  if (op != kMaxF64) return v;
  const double d = static_cast<double>(v);
  return __builtin_bit_cast(uint64_t, d);
}

// What a dev slot must hold once ``n`` workgroups of its population have run (``npk`` of them below
// kPackedWorkgroups, ``bits`` the OR of their own bits in this slot), given the base table's entry.
ATOM_HD uint64_t dev_combine(int op, uint64_t base, uint32_t n, uint32_t npk, uint32_t bits) {
  switch (op) {
    case kAdd: return static_cast<uint32_t>(static_cast<uint32_t>(base) * n);
    case kSub: return static_cast<uint32_t>(identity(kSub) - static_cast<uint32_t>(base) * n);
    case kAnd: return static_cast<uint32_t>(~bits);
    case kOr: return bits;
    case kXor: case kXor64: return (n & 1u) ? base : 0ull;
    case kAdd64: return base * n;
    case kPkF16: case kPkBf16: return packed_bits(op, static_cast<uint32_t>(base & 1u) * npk, static_cast<uint32_t>((base >> 1) & 1u) * npk);
    case kAddF32: {
      const float f = static_cast<float>(static_cast<uint32_t>(base) * n);
      return __builtin_bit_cast(uint32_t, f);
    }
    case kAddF64: {
      const double d = static_cast<double>(base * n);
      return __builtin_bit_cast(uint64_t, d);
    }
    default: return n ? base : identity(op);  // the min / max family
  }
}

// The nine dev row-sets after a run whose workgroup b ran on XCD xcc[b], as atom_verify computes them.
inline void dev_expected(uint32_t seed, int iters, const int* xcc, int nwg, uint32_t* rows) {
  std::vector<uint32_t> base(kRowSetWords);
  dev_base(seed, iters, base.data());
  for (int s = 0; s < kDevRowSets; ++s) {
    uint32_t n = 0, npk = 0, bits[kLanes] = {};
    for (int b = 0; b < nwg; ++b) {
      if (s != kAllXcd && xcc[b] != s) continue;
      ++n;
      if (b < kPackedWorkgroups) ++npk;
      bits[(b >> 5) & 63] |= 1u << (b & 31);
    }
    for (int op = 0; op < kOps; ++op)
      for (int lane = 0; lane < kLanes; ++lane) {
        const uint32_t* p = base.data() + row_word(op) + (wide(op) ? 2 * lane : lane);
        const uint64_t base1 = wide(op) ? (static_cast<uint64_t>(p[1]) << 32) | p[0] : p[0];
        if (dev_own(op)) {
          uint64_t own = base1;
          for (int b = 0; b < nwg; ++b)
            if (s == kAllXcd || xcc[b] == s) own = extreme(op, own, arg(kDev, op, dev_own_raw(op, static_cast<uint32_t>(b), lane, seed)));
          put_slot(rows + s * kRowSetWords, op, lane, dev_own_combine(op, base1, n, own));
        } else {
          put_slot(rows + s * kRowSetWords, op, lane, dev_combine(op, base1, n, npk, bits[lane]));
        }
      }
  }
}

// the whole table the library uploads (kExpWords)
inline void expected(uint32_t seed, int iters, uint32_t* table) {
  region_expected(kLds, seed, iters, table + kExpLds, table + kExpLdsDigest);
  region_expected(kL2, seed, iters, table + kExpL2, table + kExpL2Digest);
  dev_base(seed, iters, table + kExpDev);
  lds16_expected(seed, iters, table + kExpLds16);
}

// 32-bit digest of a word array, for the table the tests pin
inline uint32_t digest_of(const uint32_t* w, int n) {
  uint32_t h = 0;
  for (int i = 0; i < n; ++i) h = fold(h, w[i]);
  return h;
}

}  // namespace atom
}  // namespace
