// The probe's bf16 GEMM, C = A * Bt^T on the matrix cores: the kernel every claim runs
// (gemm_bf16_mfma_256p<true, 0, 1>) and nothing else. Its A/B siblings are in gemm_bf16_lab.h.
//
// A: [M][K] bf16 row-major, Bt: [N][K] bf16 row-major (the "NT" layout: both operands are read
// along K, so every MFMA fragment is one contiguous 16-byte LDS read), C: [M][N] fp32.
//   * 256x256x64 block tile, 8 waves, v_mfma_f32_16x16x32_bf16;
//   * operands staged HBM -> LDS by global_load_lds_dwordx4 (no VGPR round trip), two 64 KiB LDS
//     stages;
//   * st_16x32-style XOR swizzle so each 16-lane ds_read_b128 group hits 16 distinct 16-B bank
//     slots: glds writes LDS lane-linearly, so the permutation is applied to the per-lane GLOBAL
//     source address and the same involution on the read (rule 21);
//   * one block per CU at N=4096 (256 tiles), XCD-aware bijective remap (T1), tile rows in groups
//     (tile_order.h).
#pragma once

#include <cstdint>
#include <type_traits>

#include "census.h"      // mark_cu
#include "options.h"     // kGemmPipe, kGemmGroupM and the measurements that chose them
#include "tile_order.h"  // xcd_remap, grouped_tile
#include "types.h"

namespace {

constexpr int G2_BM = 256, G2_BN = 256, G2_BK = 64;
constexpr int kGemm2Threads = 512;
constexpr int G2_STAGE_SHORTS = (G2_BM + G2_BN) * G2_BK;  // one stage: A then B, 64 KiB

// byte offset, inside a [rows][64] bf16 tile (128-B rows), of logical 16-B chunk c of row r
__device__ __forceinline__ int g2_swz(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

// ------------------------------------------------------------------ MFMA GEMM, 256x256, half-tile pipeline
// The K-loop does not drain its DMA at every K-step (cdna_hip_programming.md §5 "Pipelining across barriers", T3+T4):
//   * a K-tile is four half-tiles (A rows 0-127 "A0", B rows 0-127 "B0", "B1", "A1"), each 16 KiB,
//     two global_load_lds per thread; K-tile t+1's half h is issued in phase h of K-tile t;
//   * each wave owns a 64x32 sub-block in each of the block tile's four 128x128 quadrants, so
//     phase 0 needs only A0+B0, phase 1 B1, phase 2 A1 (phase 3 computes from registers): the
//     wait before a phase retires just the halves it reads — counted vmcnt(4), i.e. two halves
//     stay in flight across every barrier — and a raw s_barrier (no __syncthreads: its fence
//     would drain the DMA) publishes them to every wave;
//   * WAR: half h of K-tile t+1 lands in K-tile t-1's buffer, whose half h was last read in a
//     phase <= h of K-tile t-1, at least one barrier earlier;
//   * s_setprio(1) around each 16-MFMA quadrant keeps hipcc from moving the cluster across the
//     barriers (T5).
// All LDS is the one __shared__ array (a second LDS object makes hipcc wait vmcnt(0) before ds_reads).
// kStagger: waves 4-7 run one phase (one barrier) behind waves 0-3, so on each SIMD one wave reads
// LDS while the other runs its MFMAs. Every wave then retires a half one phase BEFORE the phase that
// reads it (a reader one barrier behind the writer needs one barrier more: §5 "Read a staged buffer
// one phase AFTER the wait that retires it"), every phase has a barrier, and both groups execute
// the same number of barriers (group 1 one extra before the loop, group 0 one extra after it).
// kAblate (timing experiments only, wrong C): 1 = no DMA inside the K-loop, 2 = no MFMAs.
// kPrio: 0 s_setprio(1) around every quadrant's MFMAs, 1 one static s_setprio(1) for waves 4-7 and
// no flips (MI355X_MICROARCH.md §Two waves per SIMD item 4), 2 none.
template <bool kStagger, int kAblate = 0, int kPrio = 0>
__global__ __launch_bounds__(kGemm2Threads, 1) void gemm_bf16_mfma_256p(const short* __restrict__ A,
                                                                        const short* __restrict__ Bt,
                                                                        float* __restrict__ C, int M,
                                                                        int N, int K,
                                                                        unsigned long long* __restrict__ cu_map,
                                                                        int group_m) {
  __shared__ __attribute__((aligned(16))) short smem[2 * G2_STAGE_SHORTS];  // 128 KiB
  if (cu_map && threadIdx.x == 0) mark_cu(cu_map);
  const int tiles_n = N / G2_BN, tiles_m = M / G2_BM;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  int tile_m, tile_n;
  grouped_tile(wg, tiles_m, tiles_n, group_m, &tile_m, &tile_n);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;

  // half-tile h (0 A0, 1 B0, 2 B1, 3 A1): operand and row half
  // chunk q = i*512 + tid (i = 0, 1) of a 128x8-chunk half lands at byte q*16 of the half's LDS
  // image: row q>>3, slot q&7 holding logical chunk slot ^ ((row>>1)&7) (the full-tile row has
  // the same bits 1..3, so the swizzle matches g2_swz on the 256-row image)
  const short* src[4][2];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const bool is_a = (h == 0 || h == 3);
    const int half = (h == 0 || h == 1) ? 0 : 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = i * kGemm2Threads + tid, row = q >> 3, slot = q & 7;
      const int chunk = slot ^ ((row >> 1) & 7);
      const int grow = (is_a ? tile_m * G2_BM : tile_n * G2_BN) + half * 128 + row;
      src[h][i] = (is_a ? A : Bt) + static_cast<int64_t>(grow) * K + chunk * 8;
    }
  }
  auto stage_half = [&](int buf, int h, int k0) {
    if (kAblate == 1 && k0 > 0) return;
    const bool is_a = (h == 0 || h == 3);
    const int half = (h == 0 || h == 1) ? 0 : 1;
    char* base = reinterpret_cast<char*>(smem) + buf * G2_STAGE_SHORTS * 2 + (is_a ? 0 : G2_BM * 128) +
                 half * 128 * 128;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds(src[h][i] + k0, (lds_void_t*)(base + (i * kGemm2Threads + wave * 64) * 16),
                                       16, 0, 0);
  };

  f32x4 acc[4][4][2];  // [quadrant i*2+j][m][n]
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[q][m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  const int ksteps = K / G2_BK;
  bf16x8 af[2][4], b0f[2][2], b1f[2][2];  // [k-sub][m|n]
  auto read_a = [&](const char* as, int half) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int m = 0; m < 4; ++m)
        af[ks][m] = *reinterpret_cast<const bf16x8*>(as + g2_swz(half * 128 + wr * 64 + m * 16 + fr, ks * 4 + fq));
  };
  auto read_b = [&](const char* bs, int half, bf16x8 (&bf)[2][2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int n = 0; n < 2; ++n)
        bf[ks][n] = *reinterpret_cast<const bf16x8*>(bs + g2_swz(half * 128 + wc * 32 + n * 16 + fr, ks * 4 + fq));
  };
  auto quadrant = [&](f32x4 (&c)[4][2], const bf16x8 (&bf)[2][2]) {
    if constexpr (kAblate == 2) {  // keep the fragment reads alive without the matrix work
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int m = 0; m < 4; ++m) asm volatile("" ::"v"(af[ks][m]));
#pragma unroll
        for (int n = 0; n < 2; ++n) asm volatile("" ::"v"(bf[ks][n]));
      }
      return;
    }
    if constexpr (kPrio == 0) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          c[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][m], bf[ks][n], c[m][n], 0, 0, 0);
    if constexpr (kPrio == 0) __builtin_amdgcn_s_setprio(0);
  };
  auto sync = [&]() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");  // no LDS read moves above the barrier
  };

#pragma unroll
  for (int h = 0; h < 4; ++h) stage_half(0, h, 0);
  // group 1 = waves 4-7; readfirstlane makes the branch scalar (a divergent-looking `if` would
  // run the s_barrier for every wave: balanced, but no stagger)
  const bool group1 = __builtin_amdgcn_readfirstlane(wave) >= 4;
  if constexpr (kPrio == 1) {
    if (group1) __builtin_amdgcn_s_setprio(1);
  }
  if constexpr (kStagger) {
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // A0, B0 of tile 0
    sync();
    if (group1) sync();
  }
  // one K-tile: kLast drops the prefetch and retires the tail with smaller counts
  auto ktile = [&](int t, auto last_tag) {
    constexpr bool kLast = decltype(last_tag)::value;
    const int cur = t & 1, k1 = (t + 1) * G2_BK;
    const char* as = reinterpret_cast<const char*>(smem) + cur * G2_STAGE_SHORTS * 2;
    const char* bs = as + G2_BM * 128;
    if constexpr (kStagger) {
      // waits retire what the NEXT phase reads: outstanding before phase 0 = B1, A1 of this tile
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");  // B1 (read in phase 1)
      sync();
      if constexpr (!kLast) stage_half(cur ^ 1, 0, k1);
      read_a(as, 0);
      read_b(bs, 0, b0f);
      quadrant(acc[0], b0f);
      if constexpr (kLast) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");  // A1 (read in phase 2); A0' in flight
      sync();
      if constexpr (!kLast) stage_half(cur ^ 1, 1, k1);
      read_b(bs, 1, b1f);
      quadrant(acc[1], b1f);
      sync();
      if constexpr (!kLast) stage_half(cur ^ 1, 2, k1);
      read_a(as, 1);
      quadrant(acc[3], b1f);
      if constexpr (!kLast) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");  // A0', B0' (next tile's phase 0)
      sync();
      if constexpr (!kLast) stage_half(cur ^ 1, 3, k1);
      quadrant(acc[2], b0f);
    } else {
      // phase 0: A0 + B0 of this tile (A1, B1 may still be in flight)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      sync();
      if constexpr (!kLast) stage_half(cur ^ 1, 0, k1);
      read_a(as, 0);
      read_b(bs, 0, b0f);
      quadrant(acc[0], b0f);
      // phase 1: B1
      if constexpr (kLast) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      sync();
      if constexpr (!kLast) stage_half(cur ^ 1, 1, k1);
      read_b(bs, 1, b1f);
      quadrant(acc[1], b1f);
      // phase 2: A1
      if constexpr (kLast) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      sync();
      if constexpr (!kLast) stage_half(cur ^ 1, 2, k1);
      read_a(as, 1);
      quadrant(acc[3], b1f);
      // phase 3: registers only (A1 x B0); A1 of the next tile goes out
      if constexpr (!kLast) stage_half(cur ^ 1, 3, k1);
      quadrant(acc[2], b0f);
    }
  };
  for (int t = 0; t + 1 < ksteps; ++t) ktile(t, std::false_type{});
  ktile(ksteps - 1, std::true_type{});
  if constexpr (kStagger) {
    if (!group1) sync();  // balance group 1's extra barrier: every wave ran 4*ksteps + 2
  }

  // C/D layout of 16x16x32: col = lane&15, row = 4*(lane>>4) + j; quadrant q = i*2 + j
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int col = tile_n * G2_BN + (q & 1) * 128 + wc * 32 + n * 16 + fr;
        const int row0 = tile_m * G2_BM + (q >> 1) * 128 + wr * 64 + m * 16 + 4 * fq;
#pragma unroll
        for (int j = 0; j < 4; ++j) C[static_cast<int64_t>(row0 + j) * N + col] = acc[q][m][n][j];
      }
}

// The claim path's kernel: staggered wave groups, one static s_setprio ("gemmPipe" kGemmPipe).
// M, N multiples of 256, K of 64; cu_map (may be null): the CUs that ran tiles.
inline void launch_gemm_production(hipStream_t s, const short* A, const short* Bt, float* C, int M, int N, int K,
                                   unsigned long long* cu_map, int group_m) {
  static_assert(kGemmPipe == 2, "the default pipe is the kernel launched here");
  hipLaunchKernelGGL((gemm_bf16_mfma_256p<true, 0, 1>), dim3((M / G2_BM) * (N / G2_BN)), dim3(kGemm2Threads), 0, s, A,
                     Bt, C, M, N, K, cu_map, group_m);
}

}  // namespace
