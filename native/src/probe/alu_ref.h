// Host reference of the vector-ALU phase ("aluCheck", alu.h): the operand construction the kernel
// shares (index, operand windows, digest fold: ALU_HD, so one text serves both sides) and, for the
// five exact groups, every result computed on the CPU. Pure host code when compiled by plain g++
// (native/tests/test_alu_spec.cc), like arena.h.
//
// A lane keeps a 32-bit digest h per group. Step t of group g builds every operand from
//   word(g, t, o, lane) = mix(index(g, t, o, lane), seed) ^ h      h as it stood when the step began
// (mix is hbm.h's pattern_word) and folds every result r, as bits, h = (rotl(h, 5) ^ r) * 0x9E3779B1,
// in the order the step lists them. Inputs depend on lane, group, step and seed only.
//
// Floating-point operands take sign and mantissa from the word and confine the biased exponent to
// a window at the bias (f32 2^-4..2^4, f64 the same, f16 2^-2..2^2): every result is finite, no
// result is an operand, f32 and f64 never reach the subnormal range; only a cancelling v_pk_fma_f16
// does. f32 and f64 results come from std::fmaf / std::fma and from double arithmetic rounded once
// (exact for + and * of floats); f16 and bf16 are computed in double, where every intermediate of
// the window is exact, and rounded once by round_to(). The dot products get small integers, so
// every partial sum is exact whatever the order. The transcendental group has no host
// expectation in the probe: the device checks it by consensus (wave_value is that value's host side),
// and the test suite compares the kernel's trace of it (alu.h, dump stage 3) with a reference of the
// nine functions (gpupool/ops/alu.py trans_reference).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define ALU_HD __host__ __device__ inline
#else
#define ALU_HD inline
#endif

namespace {
namespace alu {

constexpr int kGroups = 6;       // int, f32, f64, f16, lane, trans
constexpr int kExactGroups = 5;  // the ones with a host expectation
constexpr int kLanes = 64;
constexpr int kMaxResults = 16;  // per step and group
enum Group { kInt = 0, kF32 = 1, kF64 = 2, kF16 = 3, kLane = 4, kTrans = 5 };
constexpr const char* kGroupNames[kGroups] = {"int", "f32", "f64", "f16", "lane", "trans"};
constexpr uint32_t kSeedBase = 0x414C5500u;  // the phase's seed is kSeedBase + HIP device ordinal
constexpr uint32_t kFoldMul = 0x9E3779B1u;
// lane-group constants: the DPP controls, the swizzle pattern (bit mode, xor 0x15), the lane written
constexpr int kDppRowShr1 = 0x111, kDppRowRor3 = 0x123, kDppRowBcast15 = 0x142, kBcastRowMask = 0xA;
constexpr int kSwizzle = 0x541F;
constexpr int kWriteLane = 5;

// hbm.h's pattern_word, restated for the host-only build (test_alu_spec.cc pins both to one table)
ALU_HD uint32_t mix(uint64_t idx, uint32_t seed) {
  uint32_t x = static_cast<uint32_t>(idx) * 0x9E3779B1u ^ static_cast<uint32_t>(idx >> 32) * 0x85EBCA77u;
  x ^= seed;
  x ^= x >> 15;
  x *= 0x2C1B3C6Du;
  x ^= x >> 12;
  return x;
}

ALU_HD uint64_t index(int group, uint32_t step, int operand, uint32_t lane) {
  return (static_cast<uint64_t>(group) << 32) | (static_cast<uint64_t>(step) << 12) |
         (static_cast<uint64_t>(operand) << 6) | lane;
}

ALU_HD uint32_t word(int group, uint32_t step, int operand, uint32_t lane, uint32_t seed, uint32_t h) {
  return mix(index(group, step, operand, lane), seed) ^ h;
}

ALU_HD uint32_t fold(uint32_t h, uint32_t r) { return (((h << 5) | (h >> 27)) ^ r) * kFoldMul; }

// operand windows: sign and mantissa of the word, biased exponent bias-4 .. bias+3 (f16: bias-2 .. bias+1)
ALU_HD uint32_t f32_bits(uint32_t w) { return (w & 0x807FFFFFu) | ((123u + ((w >> 23) & 7u)) << 23); }
ALU_HD uint64_t f64_bits(uint32_t hi, uint32_t lo) {
  return (static_cast<uint64_t>((hi & 0x800FFFFFu) | ((1019u + ((hi >> 20) & 7u)) << 20)) << 32) | lo;
}
ALU_HD uint32_t f16_bits(uint32_t w16) { return (w16 & 0x83FFu) | ((13u + ((w16 >> 10) & 3u)) << 10); }
ALU_HD uint32_t f16x2_bits(uint32_t w) { return f16_bits(w & 0xFFFFu) | (f16_bits(w >> 16) << 16); }
// dot-product operands out of one word: four integers in [-8, 7] and an accumulator in [256, 511]
ALU_HD int small_int(uint32_t w, int i) { return static_cast<int>((w >> (4 * i)) & 15u) - 8; }
ALU_HD int small_acc(uint32_t w) { return 256 + static_cast<int>((w >> 16) & 255u); }
// the lane v_readlane reads in step t
ALU_HD uint32_t read_lane(uint32_t step) { return (7u * step + 37u) & 63u; }
// A wave's 64 trans digests as the one 64-bit value the consensus compares: the sum over lanes of
// these terms mod 2^64 (a sum, so the order is free), 0 (the empty slot) mapped to 1.
ALU_HD uint64_t wave_term(uint32_t h, uint32_t lane) { return static_cast<uint64_t>(h) * (0x9E3779B97F4A7C15ull + 2ull * lane); }

// ------------------------------------------------------------------ host side

inline float as_f32(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
inline uint32_t bits_f32(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}
inline double as_f64(uint64_t b) {
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}
inline uint64_t bits_f64(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

// x, exactly representable in double, rounded once to nearest-even in the binary format of
// ``eb`` exponent and ``mb`` mantissa bits, subnormals included; finite results only. The scaling
// by a power of two is exact and nearbyint rounds in the default (nearest-even) mode.
inline uint64_t round_to(double x, int eb, int mb) {
  const uint64_t sign = std::signbit(x) ? 1ull << (eb + mb) : 0ull;
  const double a = std::fabs(x);
  if (a == 0) return sign;
  const int bias = (1 << (eb - 1)) - 1;
  int e;
  std::frexp(a, &e);  // a = m * 2^e, m in [0.5, 1)
  const int q = std::max(e - 1, 1 - bias) - mb;  // the exponent of one unit in the last place
  const uint64_t m = static_cast<uint64_t>(std::nearbyint(std::ldexp(a, -q)));  // <= 2^(mb+1)
  // a normal m carries its hidden bit into the exponent field; so does a mantissa that rounded up
  return sign | ((static_cast<uint64_t>(q + mb + bias - 1) << mb) + m);
}

// an f16 encoding (normal or subnormal) as a double
inline double f16_value(uint32_t b) {
  const int e = static_cast<int>((b >> 10) & 31u);
  const double m = static_cast<double>(b & 0x3FFu);
  const double v = e ? std::ldexp(1024.0 + m, e - 25) : std::ldexp(m, -24);
  return (b & 0x8000u) ? -v : v;
}
inline uint32_t f16_of(double x) { return static_cast<uint32_t>(round_to(x, 5, 10)); }
inline uint32_t bf16_of(double x) { return static_cast<uint32_t>(round_to(x, 8, 7)); }
// float + and * through double: 53 bits hold the exact sum or product's rounding unambiguously,
// and no compiler can contract what it sees into an fma
inline float add32(float a, float b) { return static_cast<float>(static_cast<double>(a) + static_cast<double>(b)); }
inline float mul32(float a, float b) { return static_cast<float>(static_cast<double>(a) * static_cast<double>(b)); }

// A step's results go through one of these: folded into h and, with a trace, stored at
// trace[result index][lane] (what a test or a diagnostic compares per instruction).
struct Sink {
  uint32_t h;
  uint32_t* trace;  // [kMaxResults][kLanes] or null
  uint32_t lane;
  int n = 0;
  void operator()(uint32_t r) {
    h = fold(h, r);
    if (trace) trace[n * kLanes + lane] = r;
    ++n;
  }
};

inline uint32_t step_int(uint32_t h, uint32_t t, uint32_t lane, uint32_t seed, uint32_t* trace = nullptr) {
  const uint32_t a = word(kInt, t, 0, lane, seed, h), b = word(kInt, t, 1, lane, seed, h),
                 c = word(kInt, t, 2, lane, seed, h), d = word(kInt, t, 3, lane, seed, h);
  Sink f{h, trace, lane};
  const uint64_t cd = (static_cast<uint64_t>(c) << 32) | d, ab = (static_cast<uint64_t>(a) << 32) | b;
  const uint64_t mad = static_cast<uint64_t>(a) * b + cd;  // v_mad_u64_u32
  f(static_cast<uint32_t>(mad));
  f(static_cast<uint32_t>(mad >> 32));
  f(a * c);                                                      // v_mul_lo_u32
  f(static_cast<uint32_t>((static_cast<uint64_t>(b) * d) >> 32));  // v_mul_hi_u32
  f(a + b + c);                                                  // v_add3_u32
  f((a << (d & 7u)) + c);                                        // v_lshl_add_u32
  f(static_cast<uint32_t>(ab >> (c & 31u)));                     // v_alignbit_b32: {a, b} >> c[4:0]
  uint32_t perm = 0;                                             // v_perm_b32: bytes of {a, b}, selectors 0..7
  for (int i = 0; i < 4; ++i) perm |= static_cast<uint32_t>((ab >> (8 * ((d >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
  f(perm);
  f((a >> (b & 31u)) & ((1u << (c & 31u)) - 1u));                // v_bfe_u32
  f(static_cast<uint32_t>(__builtin_popcount(a)) + b);           // v_bcnt_u32_b32
  f(a ? static_cast<uint32_t>(__builtin_clz(a)) : ~0u);          // v_ffbh_u32
  const uint64_t sum = ab + cd;                                  // v_add_co_u32, v_addc_co_u32
  f(static_cast<uint32_t>(sum));
  f(static_cast<uint32_t>(sum >> 32));
  int32_t dot = static_cast<int32_t>(c & 0xFFFFFFu);             // v_dot4_i32_i8
  for (int i = 0; i < 4; ++i) dot += static_cast<int8_t>(a >> (8 * i)) * static_cast<int8_t>(b >> (8 * i));
  f(static_cast<uint32_t>(dot));
  return f.h;
}

inline uint32_t step_f32(uint32_t h, uint32_t t, uint32_t lane, uint32_t seed, uint32_t* trace = nullptr) {
  const float a = as_f32(f32_bits(word(kF32, t, 0, lane, seed, h))), b = as_f32(f32_bits(word(kF32, t, 1, lane, seed, h))),
              c = as_f32(f32_bits(word(kF32, t, 2, lane, seed, h))), d = as_f32(f32_bits(word(kF32, t, 3, lane, seed, h)));
  const uint32_t e = word(kF32, t, 4, lane, seed, h);
  Sink f{h, trace, lane};
  f(bits_f32(std::fmaf(a, b, c)));  // v_fma_f32
  f(bits_f32(add32(a, d)));         // v_add_f32
  f(bits_f32(mul32(b, c)));         // v_mul_f32
  f(bits_f32(std::fmaf(a, c, b)));  // v_pk_fma_f32 (a, b) * (c, d) + (b, a)
  f(bits_f32(std::fmaf(b, d, a)));
  f(bits_f32(mul32(a, d)));         // v_pk_mul_f32 (a, b) * (d, d)
  f(bits_f32(mul32(b, d)));
  f(bits_f32(add32(a, b)));         // v_pk_add_f32 (a, c) + (b, d)
  f(bits_f32(add32(c, d)));
  f(bits_f32(std::fmin(a, b)));     // v_min_f32
  f(bits_f32(std::fmax(c, d)));     // v_max_f32
  f(static_cast<uint32_t>(static_cast<int32_t>(std::ldexp(a, 10))));            // v_ldexp_f32, v_cvt_i32_f32 (truncates)
  f(bits_f32(static_cast<float>(static_cast<int32_t>(e))));                      // v_cvt_f32_i32 (nearest-even)
  f(bits_f32(std::ldexp(b, static_cast<int>(e & 15u) - 8)));                     // v_ldexp_f32
  f(a < b ? bits_f32(c) : bits_f32(d));                                          // v_cmp_lt_f32, v_cndmask_b32
  return f.h;
}

inline uint32_t step_f64(uint32_t h, uint32_t t, uint32_t lane, uint32_t seed, uint32_t* trace = nullptr) {
  auto w = [&](int o) { return word(kF64, t, o, lane, seed, h); };
  const double a = as_f64(f64_bits(w(0), w(1))), b = as_f64(f64_bits(w(2), w(3))), c = as_f64(f64_bits(w(4), w(5)));
  const float g = as_f32(f32_bits(w(6)));
  Sink f{h, trace, lane};
  auto f2 = [&](double x) {
    f(static_cast<uint32_t>(bits_f64(x)));
    f(static_cast<uint32_t>(bits_f64(x) >> 32));
  };
  f2(std::fma(a, b, c));                  // v_fma_f64
  volatile double s = a + c, p = b * c;   // v_add_f64, v_mul_f64; volatile: no contraction across them
  f2(s);
  f2(p);
  f2(static_cast<double>(g));             // v_cvt_f64_f32
  f(bits_f32(static_cast<float>(a)));     // v_cvt_f32_f64
  f2(std::fmin(a, b));                    // v_min_f64
  f2(std::fmax(b, c));                    // v_max_f64
  return f.h;
}

inline uint32_t step_f16(uint32_t h, uint32_t t, uint32_t lane, uint32_t seed, uint32_t* trace = nullptr) {
  auto w = [&](int o) { return word(kF16, t, o, lane, seed, h); };
  const uint32_t a = f16x2_bits(w(0)), b = f16x2_bits(w(1)), c = f16x2_bits(w(2));
  const float g0 = as_f32(f32_bits(w(3))), g1 = as_f32(f32_bits(w(4)));
  const uint32_t s = w(5);
  Sink f{h, trace, lane};
  auto pk = [&](auto op) {
    const uint32_t lo = f16_of(op(f16_value(a & 0xFFFFu), f16_value(b & 0xFFFFu), f16_value(c & 0xFFFFu)));
    const uint32_t hi = f16_of(op(f16_value(a >> 16), f16_value(b >> 16), f16_value(c >> 16)));
    f(lo | (hi << 16));
  };
  pk([](double x, double y, double z) { return x * y + z; });  // v_pk_fma_f16: exact in double, rounded once
  pk([](double x, double, double z) { return x + z; });        // v_pk_add_f16
  pk([](double, double y, double z) { return y * z; });        // v_pk_mul_f16
  f(f16_of(g0));                                               // v_cvt_f16_f32
  f(bf16_of(g0) | (bf16_of(g1) << 16));                        // v_cvt_pk_bf16_f32
  const int dot = small_acc(s) + small_int(s, 0) * small_int(s, 2) + small_int(s, 1) * small_int(s, 3);
  f(bits_f32(static_cast<float>(dot)));                        // v_dot2c_f32_f16
  f(bits_f32(static_cast<float>(dot)));                        // v_dot2c_f32_bf16
  return f.h;
}

// The lane group works on a wave: h[64] in, h[64] out. trace as above.
inline void step_lane(uint32_t* h, uint32_t t, uint32_t seed, uint32_t* trace = nullptr) {
  uint32_t x[kLanes], y[kLanes], z[kLanes];
  for (uint32_t l = 0; l < kLanes; ++l) {
    x[l] = word(kLane, t, 0, l, seed, h[l]);
    y[l] = word(kLane, t, 1, l, seed, h[l]);
    z[l] = word(kLane, t, 2, l, seed, h[l]);
  }
  const uint32_t s = x[read_lane(t)];
  for (uint32_t l = 0; l < kLanes; ++l) {
    Sink f{h[l], trace, l};
    const uint32_t row = l & ~15u, in = l & 15u;
    f(in ? x[l - 1] : y[l]);                          // v_mov_b32_dpp row_shr:1, the row's lane 0 keeps old = y
    f(x[row | ((in + 13u) & 15u)]);                   // v_mov_b32_dpp row_ror:3
    f(((l >> 4) & 1u) ? x[row - 1] : y[l]);           // v_mov_b32_dpp row_bcast:15 row_mask:0xa, old = y
    f(l < 32 ? x[l] : y[l - 32]);                     // v_permlane32_swap (x, y): x's upper half <-> y's lower half
    f(l < 32 ? x[l + 32] : y[l]);
    f(((l >> 4) & 1u) ? z[l - 16] : x[l]);            // v_permlane16_swap (x, z): x's odd rows <-> z's even rows
    f(((l >> 4) & 1u) ? z[l] : x[l + 16]);
    f(x[z[l] & 63u]);                                 // ds_bpermute_b32
    f(y[l ^ 0x15u]);                                  // ds_swizzle_b32, bit mode: and 0x1f, or 0, xor 0x15
    f(l == kWriteLane ? s : x[l]);                    // v_readlane_b32 + v_writelane_b32
    f(s);
    f(y[0]);                                          // v_readfirstlane_b32
    h[l] = f.h;
  }
}

// the consensus value of a wave whose lanes hold the trans digests h[0..63] (alu.h sums in a butterfly)
inline uint64_t wave_value(const uint32_t* h) {
  uint64_t v = 0;
  for (uint32_t l = 0; l < kLanes; ++l) v += wave_term(h[l], l);
  return v ? v : 1;
}

// expect[g][lane], g < kExactGroups: the digests after ``steps`` steps (the kernel's dump stage 1
// is steps = 1, stage 2 and the verdict steps = iters).
inline void expected(uint32_t seed, int steps, uint32_t* expect) {
  for (uint32_t l = 0; l < kLanes; ++l) {
    uint32_t hi = 0, hf = 0, hd = 0, hh = 0;
    for (int t = 0; t < steps; ++t) {
      hi = step_int(hi, t, l, seed);
      hf = step_f32(hf, t, l, seed);
      hd = step_f64(hd, t, l, seed);
      hh = step_f16(hh, t, l, seed);
    }
    expect[kInt * kLanes + l] = hi;
    expect[kF32 * kLanes + l] = hf;
    expect[kF64 * kLanes + l] = hd;
    expect[kF16 * kLanes + l] = hh;
  }
  uint32_t* hl = expect + kLane * kLanes;
  for (uint32_t l = 0; l < kLanes; ++l) hl[l] = 0;
  for (int t = 0; t < steps; ++t) step_lane(hl, t, seed);
}

}  // namespace alu
}  // namespace
