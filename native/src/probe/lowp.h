// Low-precision matrix-core checks of the probe: OCP FP8 on the unscaled MFMA and MXFP8 / MXFP4 on
// the block-scaled one (E8M0 scale per 32 K-elements). Opt-in ("mfmaLowPrecision"): none of this
// is launched, and no memory is reserved for it, unless a probe asks for a dtype.
//
// Uses the probe's f32x4 / u32x4 / lds_void_t types, pattern_word (hbm.h), cu_key / mark_cu /
// kCensusThreads (census.h), xcd_remap (tile_order.h) and abft.h's fp32 instantiations of
// colsum_partial / rowdot, count_diff and count_ne_u32.
//
// Per dtype: a per-CU census on that dtype's instruction, a 256^3 GEMM checked element by element
// against a VALU reference that decodes the formats with integer bit arithmetic, and the N^3 GEMM
// with exact ABFT checksums over the decoded operands.
//
// Operand lane maps (pinned by the encodings test, tests/gpu/test_probe_lowp_gpu.py):
//   v_mfma_f32_16x16x32_fp8_fp8        lane l holds 8 bytes: row l&15, k = 8(l>>4) + j
//   v_mfma_scale_f32_16x16x128_f8f6f4  lane l holds row l&15 and supplies, in byte 0 of its scale
//                                      register (opsel 0), the E8M0 scale of K-block g = l>>4 (k =
//                                      32g .. 32g+31). Its operand registers hold
//                         e2m1 (16 B)  that block: k = 32g + 2j, 32g + 2j + 1 in the low and high
//                                      nibble of byte j;
//                         e4m3 (32 B)  NOT that block: registers 0-3 are k = 16g .. 16g+15 and
//                                      registers 4-7 k = 64 + 16g .. 64 + 16g + 15, so a lane's
//                                      bytes fall under the scales of two other lane groups. Found
//                                      on MI355X with per-block scales: 32 consecutive bytes per
//                                      lane is right for 1 element in 4 only.
// C/D: col = lane&15, row = 4(lane>>4) + j, as for bf16.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "abft.h"
#include "arena.h"  // align4k, lowp::region_bytes, the counter slots
#include "census.h"
#include "hbm.h"
#include "options.h"  // lowp::Dtype, kNames
#include "report.h"   // LowpResult
#include "tile_order.h"
#include "types.h"

namespace {
namespace lowp {

using i32x8 = __attribute__((ext_vector_type(8))) int;

// What the GEMM template needs to know about a dtype: element bits, the register image of one
// lane's operand for one MFMA, the K of that MFMA, the format code and the builtin.
struct Fp8 {
  static constexpr int kBits = 8, kMfmaK = 32, kFmt = 0;
  static constexpr bool kScaled = false;
  using frag = long;  // 8 e4m3 bytes
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c, int, int) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
  }
};
struct MxFp8 {
  static constexpr int kBits = 8, kMfmaK = 128, kFmt = 0;
  static constexpr bool kScaled = true;
  using frag = i32x8;  // 32 e4m3 bytes: two 16-element halves, 64 elements apart
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, kFmt, kFmt, 0, sa, 0, sb);
  }
};
struct MxFp4 {
  static constexpr int kBits = 4, kMfmaK = 128, kFmt = 4;
  static constexpr bool kScaled = true;
  using frag = i32x8;  // 16 bytes of e2m1 pairs in the low half, the high half unused
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, kFmt, kFmt, 0, sa, 0, sb);
  }
};

constexpr int bits_of(int dtype) { return dtype == kMxFp4 ? 4 : 8; }
constexpr bool scaled(int dtype) { return dtype != kFp8; }

// ------------------------------------------------------------------ decode: integer bit arithmetic only
__device__ __forceinline__ float e4m3_to_f32(uint32_t b) {  // OCP e4m3fn: bias 7, no inf, S.1111.111 = NaN
  const uint32_t s = (b & 0x80u) << 24, e = (b >> 3) & 15u, m = b & 7u;
  if (e == 15u && m == 7u) return __uint_as_float(s | 0x7fc00000u);
  if (e) return __uint_as_float(s | ((e + 120u) << 23) | (m << 20));
  if (!m) return __uint_as_float(s);
  const uint32_t p = 31u - static_cast<uint32_t>(__builtin_clz(m));  // subnormal m * 2^-9 = 1.x * 2^(p-9)
  return __uint_as_float(s | ((p + 118u) << 23) | ((m << (23u - p)) & 0x7fffffu));
}
__device__ __forceinline__ float e2m1_to_f32(uint32_t b) {  // bias 1: 0 .5 1 1.5 2 3 4 6
  const uint32_t s = (b & 8u) << 28, e = (b >> 1) & 3u, m = b & 1u;
  if (e) return __uint_as_float(s | ((e + 126u) << 23) | (m << 22));
  return __uint_as_float(s | (m ? 0x3f000000u : 0u));
}
__device__ __forceinline__ float e8m0_to_f32(uint32_t b) {  // 2^(b-127); 255 = NaN
  if (b == 255u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float(b ? b << 23 : 0x00400000u);
}
// element j of a 32-bit word of packed operand bytes (4 e4m3 or 8 e2m1, low bits first)
template <class T>
__device__ __forceinline__ float elem(uint32_t word, int j) {
  if constexpr (T::kBits == 8) return e4m3_to_f32((word >> (8 * j)) & 0xffu);
  else return e2m1_to_f32((word >> (4 * j)) & 0xfu);
}
// encodings of small integers (operand generation, census)
__device__ __forceinline__ uint32_t e4m3_of_int(int v) {  // |v| <= 15
  const uint32_t a = static_cast<uint32_t>(v < 0 ? -v : v);
  if (!a) return 0u;
  const uint32_t p = 31u - static_cast<uint32_t>(__builtin_clz(a));
  return (v < 0 ? 0x80u : 0u) | ((p + 7u) << 3) | ((a << (3u - p)) & 7u);
}
__device__ __forceinline__ uint32_t e2m1_of_1to4(int v) { return v == 1 ? 2u : v == 2 ? 4u : v == 3 ? 5u : 6u; }

// ------------------------------------------------------------------ in-probe operands
// fp8 / mxfp8: integers in [-8, 8]; mxfp4: all 16 e2m1 encodings. Scales (scaled dtypes) are
// 2^scale_lo or 2^(scale_lo+1) per (row, 32-block): mxfp8 {2^0, 2^1}, mxfp4 {2^1, 2^2}, so every
// scaled operand is an integer of magnitude <= 24 and |C| <= 576 K: exact in fp32 in any order
// for K <= 29127.
template <class T>
__global__ void gen_operand(uint32_t* __restrict__ out, uint64_t nwords, uint8_t* __restrict__ scales, uint64_t nscales,
                            uint32_t seed, int scale_lo) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nwords; i += stride) {
    uint32_t w = 0;
    if constexpr (T::kBits == 8) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w |= e4m3_of_int(static_cast<int>(pattern_word(i * 4 + j, seed) % 17u) - 8) << (8 * j);
    } else {
      w = pattern_word(i, seed);
    }
    out[i] = w;
  }
  if constexpr (T::kScaled)
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nscales; i += stride)
      scales[i] = static_cast<uint8_t>(127 + scale_lo + ((pattern_word(i, seed ^ 0x5CA1Eu) >> 7) & 1u));
}

// ------------------------------------------------------------------ census
// As cu_census, on the dtype's instruction: A[r][k] = fa(r), B[c][k] = gb(c) in 1..4. Scaled
// dtypes: K-blocks 0, 1 (lanes 0-31) carry scale 2^1 and blocks 2, 3 scale 2^2 on both operands, so
// one MFMA adds 32 * (2 * 4 + 2 * 16) * fa * gb = 1280 fa gb and a scale path that is dead, or
// takes another lane's byte, changes the sum. Unscaled: 32 fa gb. iters <= 128: below 2^24, exact.
template <class T>
__global__ __launch_bounds__(kCensusThreads) void census(unsigned long long* __restrict__ map,
                                                         unsigned long long* __restrict__ bad, int iters, uint32_t seed,
                                                         int fault_xcc) {
  const int lane = threadIdx.x & 63;
  const uint32_t h = seed ^ (blockIdx.x * 0x9E3779B1u);
  const int fa = 1 + static_cast<int>((h + (lane & 15)) & 3);
  const int gb = 1 + static_cast<int>(((h >> 8) + (lane & 15)) & 3);
  uint32_t aw, bw;
  if constexpr (T::kBits == 8) {
    aw = e4m3_of_int(fa) * 0x01010101u;
    bw = e4m3_of_int(gb) * 0x01010101u;
  } else {
    aw = e2m1_of_1to4(fa) * 0x11111111u;
    bw = e2m1_of_1to4(gb) * 0x11111111u;
  }
  typename T::frag av, bv;
  if constexpr (!T::kScaled) {
    av = static_cast<long>((static_cast<unsigned long long>(aw) << 32) | aw);
    bv = static_cast<long>((static_cast<unsigned long long>(bw) << 32) | bw);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool used = T::kBits == 8 || j < 4;
      av[j] = used ? static_cast<int>(aw) : 0;
      bv[j] = used ? static_cast<int>(bw) : 0;
    }
  }
  const int sc = lane < 32 ? 128 : 129;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < iters; ++i) acc = T::mma(av, bv, acc, sc, sc);
  if (fault_xcc >= 0 && (cu_key() >> 8) == fault_xcc) acc[0] += 1.0f;  // test hook: a "bad" XCD
  const int per = T::kScaled ? 1280 : 32;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 4 * (lane >> 4) + j;
    const int far = 1 + static_cast<int>((h + r) & 3);
    ok = ok && acc[j] == static_cast<float>(iters * per * far * gb);
  }
  const bool wave_ok = __all(ok);
  if (lane == 0) {
    if (wave_ok) mark_cu(map);
    else atomicAdd(bad, 1ull);
  }
}

// ------------------------------------------------------------------ tiled GEMM  C = A * Bt^T
// A: [M][K], Bt: [N][K] elements of T, K-contiguous (e2m1: two per byte); sA / sB: [rows][K/32] E8M0
// bytes (scaled dtypes); C: [M][N] fp32. 128x128 block tile, BK = 128 elements, 4 waves as 2x2 with
// 4x4 16x16 MFMA tiles each. Operands go HBM -> LDS by 16-byte global_load_lds into two stages; the
// plain double-buffered loop of gemm_bf16_mfma_256 (next tile's DMA under this tile's MFMAs, one
// vmcnt(0) + barrier per K-step). LDS rows are 128 B (8-bit) or 64 B (4-bit); 16-B chunk c of row r
// sits in slot c ^ swz(r), so the 16 rows a lane group reads at one chunk fall in distinct banks.
// M, N, K multiples of 128.
constexpr int kBM = 128, kBN = 128, kBK = 128, kGemmThreads = 256;

// One 16-byte global_load_lds: the lane's 16 bytes at ``src`` land at LDS address ``dst`` (wave-
// uniform) + 16 * lane. Not a template: in a type-dependent context the host pass of hipcc drops a
// kernel that calls the builtin without a word, and its launch stub with it.
__device__ __forceinline__ void glds16(const uint8_t* src, uint8_t* dst) {
  __builtin_amdgcn_global_load_lds(src, (lds_void_t*)dst, 16, 0, 0);
}

template <class T>
struct Tile {
  static constexpr int kRowBytes = kBK * T::kBits / 8;       // 128 | 64
  static constexpr int kChunks = kRowBytes / 16;             // 16-B chunks per row: 8 | 4
  static constexpr int kRowsPer256 = 256 / kRowBytes;        // rows per 256 B of LDS: 2 | 4
  static constexpr int kOperandBytes = kBM * kRowBytes;      // one operand tile: 16 | 8 KiB
  static constexpr int kLoads = kBM * kChunks / kGemmThreads;  // glds per thread per operand: 4 | 2
  static __device__ __forceinline__ int swz(int r) { return (r / kRowsPer256) & (kChunks - 1); }
  static __device__ __forceinline__ int at(int r, int c) { return r * kRowBytes + ((c ^ swz(r)) << 4); }
};

template <class T>
__device__ __forceinline__ typename T::frag read_frag(const uint8_t* tile, int r, int ks, int fq) {
  using L = Tile<T>;
  if constexpr (!T::kScaled) {
    // MFMA ks covers k = 32 ks .. 32 ks + 31: this lane's 8 bytes start at k = 32 ks + 8 fq
    return *reinterpret_cast<const long*>(tile + L::at(r, ks * 2 + (fq >> 1)) + (fq & 1) * 8);
  } else if constexpr (T::kBits == 8) {
    // two 16-element halves: k = 16 fq .. and k = 64 + 16 fq ..
    const u32x4 lo = *reinterpret_cast<const u32x4*>(tile + L::at(r, fq));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(tile + L::at(r, 4 + fq));
    return i32x8{static_cast<int>(lo.x), static_cast<int>(lo.y), static_cast<int>(lo.z), static_cast<int>(lo.w),
                 static_cast<int>(hi.x), static_cast<int>(hi.y), static_cast<int>(hi.z), static_cast<int>(hi.w)};
  } else {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(tile + L::at(r, fq));
    return i32x8{static_cast<int>(lo.x), static_cast<int>(lo.y), static_cast<int>(lo.z), static_cast<int>(lo.w), 0, 0, 0, 0};
  }
}

// a lane's scale bytes of K-step kt for its four 16-row tiles (sa, sb point at its first tile's row
// and K-block)
template <class T>
__device__ __forceinline__ void load_scales(const uint8_t* sa, const uint8_t* sb, int64_t srow, int kt, int (&a)[4],
                                            int (&b)[4]) {
  if constexpr (T::kScaled) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = sa[i * 16 * srow + kt * 4];
      b[i] = sb[i * 16 * srow + kt * 4];
    }
  }
}

template <class T>
__global__ __launch_bounds__(kGemmThreads) void gemm(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bt,
                                                     const uint8_t* __restrict__ sA, const uint8_t* __restrict__ sB,
                                                     float* __restrict__ C, int M, int N, int K) {
  using L = Tile<T>;
  __shared__ __attribute__((aligned(16))) uint8_t smem[4 * L::kOperandBytes];  // 2 stages of A then B
  const int tiles_n = N / kBN;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = wg / tiles_n, tile_n = wg % tiles_n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;  // 2x2 waves, each 64x64
  const int64_t row_bytes = static_cast<int64_t>(K) * T::kBits / 8;

  // glds: chunk q = i*256 + tid of a 128-row operand tile lands at LDS byte q*16 (lane-linear per
  // wave): LDS row q / kChunks, slot q % kChunks, which holds logical chunk slot ^ swz(row)
  const uint8_t* a_src[L::kLoads];
  const uint8_t* b_src[L::kLoads];
#pragma unroll
  for (int i = 0; i < L::kLoads; ++i) {
    const int q = i * kGemmThreads + tid, row = q / L::kChunks, slot = q % L::kChunks;
    const int chunk = slot ^ L::swz(row);
    a_src[i] = A + static_cast<int64_t>(tile_m * kBM + row) * row_bytes + chunk * 16;
    b_src[i] = Bt + static_cast<int64_t>(tile_n * kBN + row) * row_bytes + chunk * 16;
  }
  auto stage = [&](int buf, int kt) {
    uint8_t* base = smem + buf * 2 * L::kOperandBytes;
    const int64_t k0 = static_cast<int64_t>(kt) * L::kRowBytes;
#pragma unroll
    for (int i = 0; i < L::kLoads; ++i) {
      const int off = (i * kGemmThreads + wave * 64) * 16;  // wave-uniform LDS destination (M0)
      glds16(a_src[i] + k0, base + off);
      glds16(b_src[i] + k0, base + L::kOperandBytes + off);
    }
  };

  const int fr = lane & 15, fq = lane >> 4;  // fragment row and K-block
  // scaled dtypes: this lane's scale byte (row of its fragment, K-block fq of the K-step) per
  // 16-row tile, read straight from global one K-step ahead
  const int64_t srow = K / 32;
  int sa[4] = {}, sb[4] = {}, sa_next[4] = {}, sb_next[4] = {};
  const uint8_t* sa_row = sA;
  const uint8_t* sb_row = sB;
  if constexpr (T::kScaled) {
    sa_row += static_cast<int64_t>(tile_m * kBM + wr * 64 + fr) * srow + fq;
    sb_row += static_cast<int64_t>(tile_n * kBN + wc * 64 + fr) * srow + fq;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ksteps = K / kBK;
  stage(0, 0);
  load_scales<T>(sa_row, sb_row, srow, 0, sa, sb);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < ksteps; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < ksteps) {  // next tile's DMA and scales under this tile's MFMAs
      stage(cur ^ 1, kt + 1);
      load_scales<T>(sa_row, sb_row, srow, kt + 1, sa_next, sb_next);
    }
    const uint8_t* as = smem + cur * 2 * L::kOperandBytes;
    const uint8_t* bs = as + L::kOperandBytes;
#pragma unroll
    for (int ks = 0; ks < kBK / T::kMfmaK; ++ks) {
      typename T::frag bfr[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) bfr[n] = read_frag<T>(bs, wc * 64 + n * 16 + fr, ks, fq);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const typename T::frag af = read_frag<T>(as, wr * 64 + m * 16 + fr, ks, fq);
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = T::mma(af, bfr[n], acc[m][n], sa[m], sb[n]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of tile kt+1 has landed
    __syncthreads();                                   // ...and every other wave's; reads of kt done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa[i] = sa_next[i];
      sb[i] = sb_next[i];
    }
  }
  // C/D layout of 16x16: col = lane&15, row = 4*(lane>>4) + j
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int col = tile_n * kBN + wc * 64 + n * 16 + fr;
      const int row0 = tile_m * kBM + wr * 64 + m * 16 + 4 * fq;
#pragma unroll
      for (int j = 0; j < 4; ++j) C[static_cast<int64_t>(row0 + j) * N + col] = acc[m][n][j];
    }
}

inline bool gemm_args_ok(int dtype, int m, int n, int k) {
  return dtype >= 0 && dtype < kDtypes && m > 0 && n > 0 && k > 0 && m % kBM == 0 && n % kBN == 0 && k % kBK == 0;
}

template <class T>
void launch_gemm_t(hipStream_t s, const uint8_t* A, const uint8_t* Bt, const uint8_t* sA, const uint8_t* sB, float* C, int M,
                   int N, int K) {
  hipLaunchKernelGGL(gemm<T>, dim3((M / kBM) * (N / kBN)), dim3(kGemmThreads), 0, s, A, Bt, sA, sB, C, M, N, K);
}

inline void launch_gemm(hipStream_t s, int dtype, const uint8_t* A, const uint8_t* Bt, const uint8_t* sA,
                        const uint8_t* sB, float* C, int M, int N, int K) {
  if (dtype == kFp8) launch_gemm_t<Fp8>(s, A, Bt, sA, sB, C, M, N, K);
  else if (dtype == kMxFp8) launch_gemm_t<MxFp8>(s, A, Bt, sA, sB, C, M, N, K);
  else launch_gemm_t<MxFp4>(s, A, Bt, sA, sB, C, M, N, K);
}

// ------------------------------------------------------------------ VALU reference + ABFT over decoded operands
// One thread per output, no matrix cores: per 32-block an fp32 fma chain of the decoded elements,
// times the two block scales. Exact on the in-probe operands (small integers).
template <class T>
__global__ void gemm_ref(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bt, const uint8_t* __restrict__ sA,
                         const uint8_t* __restrict__ sB, float* __restrict__ C, int M, int N, int K) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
  if (n >= N || m >= M) return;
  constexpr int E = 32 / T::kBits, W = 32 / E;  // elements per word, words per 32-block
  const int64_t row_words = static_cast<int64_t>(K) / E, srow = K / 32;
  const uint32_t* a = reinterpret_cast<const uint32_t*>(A) + m * row_words;
  const uint32_t* b = reinterpret_cast<const uint32_t*>(Bt) + n * row_words;
  float s = 0.f;
  for (int blk = 0; blk < K / 32; ++blk) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint32_t aw = a[blk * W + w], bw = b[blk * W + w];
#pragma unroll
      for (int j = 0; j < E; ++j) t = fmaf(elem<T>(aw, j), elem<T>(bw, j), t);
    }
    if constexpr (T::kScaled) t *= e8m0_to_f32(sA[m * srow + blk]) * e8m0_to_f32(sB[n * srow + blk]);
    s += t;
  }
  C[static_cast<int64_t>(m) * N + n] = s;
}

__device__ __forceinline__ uint32_t int_u32(float v) { return static_cast<uint32_t>(static_cast<int>(v)); }

// out[k] += sum over a slab of rows of the decoded, scaled X[r][k] (an integer), mod 2^32. A thread
// owns one 32-bit word of each row (4 or 8 adjacent columns).
constexpr int kColSlab = 64;
template <class T>
__global__ __launch_bounds__(256) void colsum(const uint8_t* __restrict__ X, const uint8_t* __restrict__ S, int rows, int K,
                                              uint32_t* __restrict__ out) {
  constexpr int E = 32 / T::kBits;
  const int w = blockIdx.x * 256 + threadIdx.x, k0 = w * E;
  if (k0 >= K) return;
  const int64_t row_words = K / E, srow = K / 32;
  const int r0 = blockIdx.y * kColSlab, r1 = min(rows, r0 + kColSlab);
  uint32_t acc[E] = {};
  for (int r = r0; r < r1; ++r) {
    const uint32_t x = reinterpret_cast<const uint32_t*>(X)[r * row_words + w];
    float sc = 1.f;
    if constexpr (T::kScaled) sc = e8m0_to_f32(S[r * srow + k0 / 32]);
#pragma unroll
    for (int j = 0; j < E; ++j) acc[j] += int_u32(elem<T>(x, j) * sc);
  }
#pragma unroll
  for (int j = 0; j < E; ++j) atomicAdd(&out[k0 + j], acc[j]);
}

// out[r] = sum_k X[r][k] * w[k] mod 2^32 over the decoded, scaled operand; one wave per row.
template <class T>
__global__ __launch_bounds__(256) void rowdot(const uint8_t* __restrict__ X, const uint8_t* __restrict__ S, int rows, int K,
                                              const uint32_t* __restrict__ w, uint32_t* __restrict__ out) {
  constexpr int E = 32 / T::kBits;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int64_t row_words = K / E, srow = K / 32;
  const uint32_t* x = reinterpret_cast<const uint32_t*>(X) + row * row_words;
  uint32_t s = 0;
  for (int d = lane; d < row_words; d += 64) {
    const uint32_t xw = x[d];
    const int k0 = d * E;
    float sc = 1.f;
    if constexpr (T::kScaled) sc = e8m0_to_f32(S[row * srow + k0 / 32]);
#pragma unroll
    for (int j = 0; j < E; ++j) s += int_u32(elem<T>(xw, j) * sc) * w[k0 + j];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) out[row] = s;
}

__global__ void inject_fault(float* __restrict__ c, int64_t idx) { c[idx] += 1.0f; }  // test hook

// The element check's reference launch, as the probe and the host-buffer test surface share it
// (k % 32 == 0); its count_diff is abft.h's launch_count_diff.
template <class T>
void launch_gemm_ref(hipStream_t s, const uint8_t* a, const uint8_t* bt, const uint8_t* sa, const uint8_t* sb, float* r, int m,
                     int n, int k) {
  hipLaunchKernelGGL(gemm_ref<T>, dim3((n + 255) / 256, m), dim3(256), 0, s, a, bt, sa, sb, r, m, n, k);
}

// The low-precision checker sequence on stream s (no host sync), abft.h's enqueue_abft over the
// decoded, scaled operands: A [m][k], Bt [n][k] elements of T with their scales (null: unscaled),
// C [m][n] fp32; k % 32 == 0, n % 4 == 0. The caller zeroes the first three vectors on s first.
template <class T>
void enqueue_abft(hipStream_t s, const uint8_t* a, const uint8_t* bt, const uint8_t* sa, const uint8_t* sb, const float* c,
                  int m, int n, int k, float bound, const AbftVectors& v, const AbftCounters& cnt) {
  constexpr int E = 32 / T::kBits;
  const int xblocks = (k / E + 255) / 256;
  hipLaunchKernelGGL(colsum<T>, dim3(xblocks, (m + kColSlab - 1) / kColSlab), dim3(256), 0, s, a, sa, m, k, v.acol);
  hipLaunchKernelGGL(colsum<T>, dim3(xblocks, (n + kColSlab - 1) / kColSlab), dim3(256), 0, s, bt, sb, n, k, v.bcol);
  enqueue_abft_c_colsum(s, c, m, n, bound, v, cnt);
  hipLaunchKernelGGL(rowdot<T>, dim3((n + 3) / 4), dim3(256), 0, s, bt, sb, n, k, static_cast<const uint32_t*>(v.acol),
                     v.exp_col);
  enqueue_abft_c_rowsum(s, c, m, n, v);
  hipLaunchKernelGGL(rowdot<T>, dim3((m + 3) / 4), dim3(256), 0, s, a, sa, m, k, static_cast<const uint32_t*>(v.bcol),
                     v.exp_row);
  enqueue_abft_compare(s, m, n, v, cnt);
}

// ------------------------------------------------------------------ host side: one dtype's phase
// The dtype's counters (kSlot*) and the size of the region carved below (region_bytes): arena.h.
constexpr int kCensusIters = 128;

// Enqueues one dtype's checks on s (no host sync): the 256^3 GEMM against the VALU reference, the
// timed N^3 GEMM (events e0, e1) with ABFT, the census. cnt: the dtype's kSlots counters, zeroed by
// the caller on s. gemm_n: a multiple of 128.
template <class T>
void launch_phase_t(hipStream_t s, int dtype, char* region, int gemm_n, int cus, unsigned long long* cnt,
                         hipEvent_t e0, hipEvent_t e1, int64_t inject_at, int census_fault_xcc, bool poison_c) {
  const size_t n = static_cast<size_t>(gemm_n), n0 = kSmallN;
  char* p = region;
  auto carve = [&](size_t bytes) {
    char* q = p;
    p += align4k(bytes);
    return reinterpret_cast<uint8_t*>(q);
  };
  uint8_t *a0 = carve(n0 * n0), *b0 = carve(n0 * n0), *sa0 = carve(n0 * n0 / 32), *sb0 = carve(n0 * n0 / 32);
  auto* c0 = reinterpret_cast<float*>(carve(n0 * n0 * 4));
  auto* r0 = reinterpret_cast<float*>(carve(n0 * n0 * 4));
  uint8_t *a = carve(n * n), *b = carve(n * n), *sa = carve(n * n / 32), *sb = carve(n * n / 32);
  auto* c = reinterpret_cast<float*>(carve(n * n * 4));
  auto* v32 = reinterpret_cast<uint32_t*>(carve(6 * n * 4));
  if (static_cast<size_t>(p - region) != region_bytes(n)) throw ProbeError("lowp region and its size disagree");
  uint32_t *vacol = v32, *vbcol = v32 + n, *vcolC = v32 + 2 * n, *vexpC = v32 + 3 * n, *vrowC = v32 + 4 * n,
           *vexpR = v32 + 5 * n;
  const int scale_lo = dtype == kMxFp4 ? 1 : 0;
  const uint32_t seed = 0x10F0u + 0x101u * static_cast<uint32_t>(dtype);
  // |C| <= K * (largest scaled operand)^2: 8, 16, 24
  const float span = dtype == kFp8 ? 8.f : dtype == kMxFp8 ? 16.f : 24.f;
  const float bound = static_cast<float>(gemm_n) * span * span;
  PROBE_CHECK(hipMemsetAsync(v32, 0, 3 * n * sizeof(uint32_t), s));
  if (poison_c) PROBE_CHECK(hipMemsetAsync(c, 0xFF, n * n * sizeof(float), s));
  {
    const int in0 = static_cast<int>(n0);
    const uint64_t w0 = n0 * n0 * T::kBits / 32, w = n * n * T::kBits / 32;
    // (a) 256^3, every element against the VALU reference
    hipLaunchKernelGGL(gen_operand<T>, dim3(64), dim3(256), 0, s, reinterpret_cast<uint32_t*>(a0), w0, sa0,
                       static_cast<uint64_t>(n0 * n0 / 32), seed, scale_lo);
    hipLaunchKernelGGL(gen_operand<T>, dim3(64), dim3(256), 0, s, reinterpret_cast<uint32_t*>(b0), w0, sb0,
                       static_cast<uint64_t>(n0 * n0 / 32), seed ^ 0xBEEFu, scale_lo);
    launch_gemm(s, dtype, a0, b0, sa0, sb0, c0, in0, in0, in0);
    launch_gemm_ref<T>(s, a0, b0, sa0, sb0, r0, in0, in0, in0);
    launch_count_diff(s, c0, r0, static_cast<uint64_t>(n0 * n0), cnt + kSlotSmall);
    // (b) N^3, timed, exact ABFT
    hipLaunchKernelGGL(gen_operand<T>, dim3(2048), dim3(256), 0, s, reinterpret_cast<uint32_t*>(a), w, sa,
                       static_cast<uint64_t>(n * n / 32), seed ^ 0x51u, scale_lo);
    hipLaunchKernelGGL(gen_operand<T>, dim3(2048), dim3(256), 0, s, reinterpret_cast<uint32_t*>(b), w, sb,
                       static_cast<uint64_t>(n * n / 32), seed ^ 0x77u, scale_lo);
    PROBE_CHECK(hipEventRecord(e0, s));
    launch_gemm(s, dtype, a, b, sa, sb, c, gemm_n, gemm_n, gemm_n);
    PROBE_CHECK(hipEventRecord(e1, s));
    if (inject_at >= 0) hipLaunchKernelGGL(inject_fault, dim3(1), dim3(1), 0, s, c, inject_at);
    unsigned long long* bad = cnt + kSlotAbft;
    enqueue_abft<T>(s, a, b, sa, sb, c, gemm_n, gemm_n, gemm_n, bound, AbftVectors{vacol, vbcol, vcolC, vexpC, vrowC, vexpR},
                    AbftCounters{bad, bad, bad});
    // (c) every CU on this dtype's instruction
    hipLaunchKernelGGL(census<T>, dim3(8 * cus), dim3(kCensusThreads), 0, s, cnt + kSlotCensusMap, cnt + kSlotCensusBad,
                       kCensusIters, 0xC0FFEEu ^ static_cast<uint32_t>(gemm_n) ^ (static_cast<uint32_t>(dtype) << 20),
                       census_fault_xcc);
  }
}

inline void launch_phase(hipStream_t s, int dtype, char* region, int gemm_n, int cus, unsigned long long* cnt,
                         hipEvent_t e0, hipEvent_t e1, int64_t inject_at, int census_fault_xcc, bool poison_c) {
  if (dtype == kFp8) launch_phase_t<Fp8>(s, dtype, region, gemm_n, cus, cnt, e0, e1, inject_at, census_fault_xcc, poison_c);
  else if (dtype == kMxFp8) launch_phase_t<MxFp8>(s, dtype, region, gemm_n, cus, cnt, e0, e1, inject_at, census_fault_xcc, poison_c);
  else launch_phase_t<MxFp4>(s, dtype, region, gemm_n, cus, cnt, e0, e1, inject_at, census_fault_xcc, poison_c);
}

// What the phase needs of a probe: where its memory and events are, and the options.
struct Phase {
  int mask = 0;                         // dtypes asked for; 0: nothing is enqueued
  char* region = nullptr;               // region_bytes(gemm_n), shared by the dtypes
  unsigned long long* cnt = nullptr;    // kDtypes * kSlots device counters
  unsigned long long* host = nullptr;   // their pinned copy
  hipEvent_t (*ev)[2] = nullptr;        // per dtype: around the timed GEMM
  int gemm_n = 0, cus = 0;
  int inject_mask = 0, census_fault_xcc = -1;  // test hooks
  int64_t inject_at = -1;                      // the element inject_mask's dtypes corrupt; -1: none
  bool poison_c = false;
};

// Follows the bf16 MFMA phase on its stream: one dtype after the other through the shared region,
// their counters copied back together. No host sync.
inline void launch(hipStream_t s, const Phase& ph) {
  if (!ph.mask) return;
  PROBE_CHECK(hipMemsetAsync(ph.cnt, 0, kDtypes * kSlots * sizeof(unsigned long long), s));
  for (int d = 0; d < kDtypes; ++d)
    if (ph.mask >> d & 1)
      launch_phase(s, d, ph.region, ph.gemm_n, ph.cus, ph.cnt + d * kSlots, ph.ev[d][0], ph.ev[d][1],
                   (ph.inject_mask >> d & 1) ? ph.inject_at : -1, ph.census_fault_xcc, ph.poison_c);
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipMemcpyAsync(ph.host, ph.cnt, kDtypes * kSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
}

// After the stream's synchronise: each dtype's report entry; any failure fails the probe.
inline std::vector<LowpResult> finish(const Phase& ph, bool require_all_cus) {
  std::vector<LowpResult> out;
  for (int d = 0; d < kDtypes; ++d) {
    if (!(ph.mask >> d & 1)) continue;
    const unsigned long long* r = ph.host + d * kSlots;
    LowpResult res;
    res.name = kNames[d];
    res.n = ph.gemm_n;
    PROBE_CHECK(hipEventElapsedTime(&res.ms, ph.ev[d][0], ph.ev[d][1]));
    res.small_bad = r[kSlotSmall];
    res.abft_bad = r[kSlotAbft];
    res.bad_waves = r[kSlotCensusBad];
    res.verified = count_cus(r + kSlotCensusMap).total;
    res.ok = res.small_bad == 0 && res.abft_bad == 0 && res.bad_waves == 0 && (!require_all_cus || res.verified >= ph.cus);
    out.push_back(res);
  }
  return out;
}

}  // namespace lowp
}  // namespace
