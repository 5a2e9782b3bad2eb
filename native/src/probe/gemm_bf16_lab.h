// The bf16 GEMM's experiment kernels, selectable per probe for in-process A/B comparisons against
// the production kernel (gemm_bf16.h): the older 128x128 register-staged kernel ("gemmTile":128),
// the 2-phase loop of the 256x256 tile ("gemmPipe":0, with "gemmPrio" / "gemmVecC"), the 32x32x16
// fragment ring (3), the other instantiations of the half-tile pipeline (1, 21, 22) and its
// timing-only ablations (11, 12). launch_gemm_lab() is every branch of the dispatch but the default.
#pragma once

#include <cstdint>

#include "gemm_bf16.h"

namespace {

// ------------------------------------------------------------------ MFMA GEMM, 128x128 tile
// A: [M][K] bf16 row-major, Bt: [N][K] bf16 row-major (the "NT" layout: both operands are read
// along K, so every MFMA fragment is one contiguous 16-byte LDS read), C: [M][N] fp32.
constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDS_STRIDE = BK + 8;  // +16 B pad per row: 80-B rows spread ds_read_b128 lane groups
constexpr int kGemmThreads = 256;

__global__ __launch_bounds__(kGemmThreads, 2) void gemm_bf16_mfma_nt(const short* __restrict__ A,
                                                                      const short* __restrict__ Bt,
                                                                      float* __restrict__ C, int M,
                                                                      int N, int K) {
  __shared__ __attribute__((aligned(16))) short smem[2 * (BM + BN) * LDS_STRIDE];
  short* As = smem;
  short* Bs = smem + BM * LDS_STRIDE;

  const int tiles_n = N / BN;
  const int nwg = gridDim.x;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int tile_m = wg / tiles_n, tile_n = wg % tiles_n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;  // 2x2 waves, each 64x64

  // global->register staging: 128 rows x 32 bf16 = 512 x 16 B per operand, 2 per thread
  const int ld_row = tid >> 2, ld_col = (tid & 3) * 8;
  const short* a_src = A + static_cast<int64_t>(tile_m * BM + ld_row) * K + ld_col;
  const short* b_src = Bt + static_cast<int64_t>(tile_n * BN + ld_row) * K + ld_col;
  const int64_t row64 = static_cast<int64_t>(64) * K;

  bf16x8 ra0, ra1, rb0, rb1;
  auto gload = [&](int k0) {
    ra0 = *reinterpret_cast<const bf16x8*>(a_src + k0);
    ra1 = *reinterpret_cast<const bf16x8*>(a_src + row64 + k0);
    rb0 = *reinterpret_cast<const bf16x8*>(b_src + k0);
    rb1 = *reinterpret_cast<const bf16x8*>(b_src + row64 + k0);
  };
  auto swrite = [&](int buf) {
    short* as = As + buf * (BM + BN) * LDS_STRIDE;
    short* bs = as + BM * LDS_STRIDE;
    *reinterpret_cast<bf16x8*>(as + ld_row * LDS_STRIDE + ld_col) = ra0;
    *reinterpret_cast<bf16x8*>(as + (ld_row + 64) * LDS_STRIDE + ld_col) = ra1;
    *reinterpret_cast<bf16x8*>(bs + ld_row * LDS_STRIDE + ld_col) = rb0;
    *reinterpret_cast<bf16x8*>(bs + (ld_row + 64) * LDS_STRIDE + ld_col) = rb1;
  };
  (void)Bs;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;  // fragment row/col and k-half
  gload(0);
  swrite(0);
  __syncthreads();
  const int ksteps = K / BK;
  for (int kt = 0; kt < ksteps; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < ksteps) gload((kt + 1) * BK);  // next tile in flight under this tile's MFMAs
    const short* as = As + buf * (BM + BN) * LDS_STRIDE;
    const short* bs = as + BM * LDS_STRIDE;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      bf16x8 af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(as + (wr * 64 + i * 32 + fr) * LDS_STRIDE + ks * 16 + fh * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        bfr[j] = *reinterpret_cast<const bf16x8*>(bs + (wc * 64 + j * 32 + fr) * LDS_STRIDE + ks * 16 + fh * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < ksteps) swrite(buf ^ 1);  // other buffer: last read one iteration ago
    __syncthreads();
  }
  // C/D layout of 32x32x16: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = tile_n * BN + wc * 64 + j * 32 + fr;
      const int row0 = tile_m * BM + wr * 64 + i * 32 + 4 * fh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + (r & 3) + 8 * (r >> 2);
        C[static_cast<int64_t>(row) * N + col] = acc[i][j][r];
      }
    }
}

// ------------------------------------------------------------------ MFMA GEMM, 256x256 tile, 2-phase loop
// The production kernel's tile, LDS image and swizzle (gemm_bf16.h) with the "minimum 2-phase" loop
// (cdna_hip_programming.md §5 "glds, 2 LDS buffers, BK=64" row, T3/T4), "gemmPipe":0:
//   * 256x256x64 block tile, 8 waves as 2(M) x 4(N), each wave 128x64 = 8x4 tiles of
//     v_mfma_f32_16x16x32_bf16 (64 MFMAs per wave per K-step, 128 accumulator registers);
//   * operands staged HBM -> LDS by global_load_lds_dwordx4 (no VGPR round trip, 8 per thread per
//     K-step), two 64 KiB LDS stages: the next K-tile's DMA is issued before this tile's
//     ds_reads + MFMAs and retired by one vmcnt(0) + barrier per K-step;
//   * st_16x32-style XOR swizzle so each 16-lane ds_read_b128 group hits 16 distinct 16-B bank
//     slots: glds writes LDS lane-linearly, so the permutation is applied to the per-lane GLOBAL
//     source address and the same involution on the read (rule 21);
//   * one block per CU at N=4096 (256 tiles), XCD-aware bijective remap (T1).
// kPrio: s_setprio(1) around each K-step's MFMA block (cdna_hip_programming.md T5). Measured null on
// this 2-phase loop (4096^3 1246 vs 1236, 8192^3 1315 vs 1312 TFLOP/s, profiles/
// r4u_gemm_setprio_ab_rejected.json): off by default, selectable for A/B ("gemmPrio").
// kVecC: the MFMA computes each 16x16 tile transposed (B fragment as the first operand), so a lane
// holds 4 consecutive columns of one C row and the epilogue writes them as one 16-byte store
// instead of four 4-byte ones (same MFMAs, same C). Measured no faster (4096^3 1322 vs 1322, 2048^3
// 315 vs 337 TFLOP/s, profiles/r4v_gemm_vecc_ab_rejected.json): off, selectable ("gemmVecC").
template <bool kPrio = false, bool kVecC = false>
__global__ __launch_bounds__(kGemm2Threads, 1) void gemm_bf16_mfma_256(const short* __restrict__ A,
                                                                       const short* __restrict__ Bt,
                                                                       float* __restrict__ C, int M,
                                                                       int N, int K,
                                                                       unsigned long long* __restrict__ cu_map,
                                                                       int group_m) {
  __shared__ __attribute__((aligned(16))) short smem[2 * G2_STAGE_SHORTS];  // 128 KiB, the only LDS object
  if (cu_map && threadIdx.x == 0) mark_cu(cu_map);  // which CUs ran GEMM tiles (probe report)
  const int tiles_n = N / G2_BN, tiles_m = M / G2_BM;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  // tile order inside each XCD's contiguous range of wg: tile_order.h
  int tile_m, tile_n;
  grouped_tile(wg, tiles_m, tiles_n, group_m, &tile_m, &tile_n);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;

  // glds source addresses. Chunk q = i*512 + tid (i = 0..3) of a 256x8-chunk operand tile lands at
  // LDS byte q*16 (lane-linear per wave: q = i*512 + wave*64 + lane): LDS row q>>3, slot q&7. The
  // slot holds logical chunk (slot ^ swz(row)), so that is the chunk we fetch.
  const short* a_src[4];
  const short* b_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = i * kGemm2Threads + tid, row = q >> 3, slot = q & 7;
    const int chunk = slot ^ ((row >> 1) & 7);
    a_src[i] = A + static_cast<int64_t>(tile_m * G2_BM + row) * K + chunk * 8;
    b_src[i] = Bt + static_cast<int64_t>(tile_n * G2_BN + row) * K + chunk * 8;
  }
  // wave-uniform LDS destinations (M0) for instruction i of this wave: byte (i*512 + wave*64)*16
  auto stage = [&](int buf, int k0) {
    char* base = reinterpret_cast<char*>(smem) + buf * G2_STAGE_SHORTS * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = (i * kGemm2Threads + wave * 64) * 16;
      __builtin_amdgcn_global_load_lds(a_src[i] + k0, (lds_void_t*)(base + off), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(b_src[i] + k0, (lds_void_t*)(base + G2_BM * 128 + off), 16,
                                       0, 0);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;  // fragment row and k-quarter (8 elements)
  const int ksteps = K / G2_BK;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < ksteps; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < ksteps) stage(cur ^ 1, (kt + 1) * G2_BK);  // next tile's DMA under this tile's MFMAs
    const char* as = reinterpret_cast<const char*>(smem) + cur * G2_STAGE_SHORTS * 2;
    const char* bs = as + G2_BM * 128;
#pragma unroll
    for (int ks = 0; ks < G2_BK / 32; ++ks) {
      const int c = ks * 4 + fq;
      bf16x8 af[8], bfr[4];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        bfr[n] = *reinterpret_cast<const bf16x8*>(bs + g2_swz(wc * 64 + n * 16 + fr, c));
#pragma unroll
      for (int m = 0; m < 8; ++m)
        af[m] = *reinterpret_cast<const bf16x8*>(as + g2_swz(wr * 128 + m * 16 + fr, c));
      if constexpr (kPrio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          if constexpr (kVecC)
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[n], af[m], acc[m][n], 0, 0, 0);
          else
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], bfr[n], acc[m][n], 0, 0, 0);
        }
      if constexpr (kPrio) __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of tile kt+1 has landed
    __syncthreads();                                   // ...and every other wave's; reads of kt done
  }
  if constexpr (kVecC) {
    // transposed tile: lane holds C[m*16 + (lane&15)][n*16 + 4*(lane>>4) + j], j = 0..3
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int row = tile_m * G2_BM + wr * 128 + m * 16 + fr;
        const int col0 = tile_n * G2_BN + wc * 64 + n * 16 + 4 * fq;
        *reinterpret_cast<f32x4*>(C + static_cast<int64_t>(row) * N + col0) = acc[m][n];
      }
  } else {
    // C/D layout of 16x16x32: col = lane&15, row = 4*(lane>>4) + j
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int col = tile_n * G2_BN + wc * 64 + n * 16 + fr;
        const int row0 = tile_m * G2_BM + wr * 128 + m * 16 + 4 * fq;
#pragma unroll
        for (int j = 0; j < 4; ++j) C[static_cast<int64_t>(row0 + j) * N + col] = acc[m][n][j];
      }
  }
}

// ------------------------------------------------------------------ MFMA GEMM, 256x256, 32x32x16 + fragment ring
// The same tile, LDS image and DMA as gemm_bf16_mfma_256 (one 64 KiB K-tile per stage, two stages,
// one barrier per K-tile), with the fragment reads pipelined instead of issued in a burst:
//   * v_mfma_f32_32x32x16_bf16: a wave's 128x64 is 4x2 tiles of 32x32, a K-tile 4 k-steps of 16,
//     8 MFMAs (256 matrix cycles) per k-step;
//   * two fragment register sets (A 4 x 16 B, B 2 x 16 B each): while k-step s runs its MFMAs from
//     one set, the 6 ds_read_b128 of k-step s+1 fill the other — the reads sit in the MFMA gaps
//     (2 per 32-cycle gap cost ~nothing, MI355X_MICROARCH.md §LDS) instead of in front of them;
//   * k-step 0 of the next K-tile is read during k-step 3 of this one, so the K-tile's barrier sits
//     between k-steps 2 and 3: vmcnt(0) (this wave's DMA of the next tile, issued a K-tile ago) +
//     lgkmcnt(0) (its reads of this tile's last k-step, so the stage can be overwritten) + barrier,
//     then the DMA of the tile after next goes into this tile's stage.
// 32x32x16 operand map: lane l holds A[row l&31][k 8*(l>>5) + j], B likewise; C: col = l&31,
// row = (reg&3) + 8*(reg>>2) + 4*(l>>5).
__global__ __launch_bounds__(kGemm2Threads, 1) void gemm_bf16_mfma_256x(const short* __restrict__ A,
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
  const short* a_src[4];
  const short* b_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = i * kGemm2Threads + tid, row = q >> 3, slot = q & 7;
    const int chunk = slot ^ ((row >> 1) & 7);
    a_src[i] = A + static_cast<int64_t>(tile_m * G2_BM + row) * K + chunk * 8;
    b_src[i] = Bt + static_cast<int64_t>(tile_n * G2_BN + row) * K + chunk * 8;
  }
  auto stage = [&](int buf, int k0) {
    char* base = reinterpret_cast<char*>(smem) + buf * G2_STAGE_SHORTS * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = (i * kGemm2Threads + wave * 64) * 16;
      __builtin_amdgcn_global_load_lds(a_src[i] + k0, (lds_void_t*)(base + off), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(b_src[i] + k0, (lds_void_t*)(base + G2_BM * 128 + off), 16, 0, 0);
    }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[m][n][j] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;
  bf16x8 ra0[4], rb0[2], ra1[4], rb1[2];  // the two fragment sets
  // Fragment reads are inline-asm ds_read_b128 with hand-counted lgkmcnt: hipcc waits lgkmcnt(0)
  // for its own reads before every MFMA group here, which serialises the ring. hipcc neither
  // tracks nor waits for these, so every use sits behind an explicit wait + sched_barrier
  // (cdna_hip_programming.md §5.4 rule 18).
  typedef __attribute__((address_space(3))) char lds_char_t;
  const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_char_t*)smem));
  // per-lane byte offset of k-step s inside a stage, A rows (wr*128 + fr) and B rows (wc*64 + fr);
  // the m / n tiles add 32 rows = 4096 B (the swizzle depends on row bits 1..3 only)
  uint32_t a_off[4], b_off[4];
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    a_off[st] = lds0 + g2_swz(wr * 128 + fr, 2 * st + fh);
    b_off[st] = lds0 + G2_BM * 128 + g2_swz(wc * 64 + fr, 2 * st + fh);
  }
  auto ds16 = [](uint32_t addr) {
    bf16x8 r;
    asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(addr));
    return r;
  };
  auto read = [&](int buf, int st, bf16x8 (&ra)[4], bf16x8 (&rb)[2]) {
    const uint32_t bo = static_cast<uint32_t>(buf) * (G2_STAGE_SHORTS * 2);
#pragma unroll
    for (int n = 0; n < 2; ++n) rb[n] = ds16(b_off[st] + bo + n * 4096);
#pragma unroll
    for (int m = 0; m < 4; ++m) ra[m] = ds16(a_off[st] + bo + m * 4096);
  };
  auto wait_lgkm6 = [] {
    asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto wait_lgkm0 = [] {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto mfma = [&](const bf16x8 (&ra)[4], const bf16x8 (&rb)[2]) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[m], rb[n], acc[m][n], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };

  const int ksteps = K / G2_BK;
  stage(0, 0);
  if (ksteps > 1) stage(1, G2_BK);
  if (ksteps > 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // stage 0 (stage 1 in flight)
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  read(0, 0, ra0, rb0);
  for (int t = 0; t < ksteps; ++t) {
    const int cur = t & 1;
    read(cur, 1, ra1, rb1);
    wait_lgkm6();  // k-step 0's six reads are in, k-step 1's six may be in flight
    mfma(ra0, rb0);
    read(cur, 2, ra0, rb0);
    wait_lgkm6();
    mfma(ra1, rb1);
    read(cur, 3, ra1, rb1);
    wait_lgkm6();
    mfma(ra0, rb0);
    if (t + 1 < ksteps) {
      // the next tile's stage has landed (this wave's part; the barrier makes it everyone's) and
      // this wave's reads of this stage are done, so the tile after next may overwrite it
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (t + 2 < ksteps) stage(cur, (t + 2) * G2_BK);
      __builtin_amdgcn_sched_barrier(0);
      read(cur ^ 1, 0, ra0, rb0);
      __builtin_amdgcn_sched_barrier(0);
    } else {
      wait_lgkm0();
    }
    mfma(ra1, rb1);
  }

#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = tile_n * G2_BN + wc * 64 + n * 32 + fr;
      const int rbase = tile_m * G2_BM + wr * 128 + m * 32 + 4 * fh;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        C[static_cast<int64_t>(rbase + (j & 3) + 8 * (j >> 2)) * N + col] = acc[m][n][j];
    }
}

// Every variant but the default (tile 256, pipe kGemmPipe: launch_gemm never comes here with it).
// Pipes 11 / 12 are the timing-only ablations (wrong C); any other unknown pipe runs the 2-phase
// loop. The 128x128 kernel has no tile order option and marks no CUs.
inline void launch_gemm_lab(hipStream_t s, const GemmVariant& v, const short* A, const short* Bt, float* C, int M, int N,
                            int K, unsigned long long* cu_map, int group_m) {
  if (v.tile != 256) {
    hipLaunchKernelGGL(gemm_bf16_mfma_nt, dim3((M / BM) * (N / BN)), dim3(kGemmThreads), 0, s, A, Bt, C, M, N, K);
    return;
  }
  const dim3 grid((M / G2_BM) * (N / G2_BN)), block(kGemm2Threads);
  if (v.pipe == 1)
    hipLaunchKernelGGL((gemm_bf16_mfma_256p<false>), grid, block, 0, s, A, Bt, C, M, N, K, cu_map, group_m);
  else if (v.pipe == 3)
    hipLaunchKernelGGL(gemm_bf16_mfma_256x, grid, block, 0, s, A, Bt, C, M, N, K, cu_map, group_m);
  else if (v.pipe == 21)
    hipLaunchKernelGGL((gemm_bf16_mfma_256p<true, 0, 0>), grid, block, 0, s, A, Bt, C, M, N, K, cu_map, group_m);
  else if (v.pipe == 22)
    hipLaunchKernelGGL((gemm_bf16_mfma_256p<true, 0, 2>), grid, block, 0, s, A, Bt, C, M, N, K, cu_map, group_m);
  else if (v.pipe == 11)  // ablations (timing only; the checks fail)
    hipLaunchKernelGGL((gemm_bf16_mfma_256p<true, 1, 1>), grid, block, 0, s, A, Bt, C, M, N, K, cu_map, group_m);
  else if (v.pipe == 12)
    hipLaunchKernelGGL((gemm_bf16_mfma_256p<true, 2, 1>), grid, block, 0, s, A, Bt, C, M, N, K, cu_map, group_m);
  else if (v.prio)
    hipLaunchKernelGGL((gemm_bf16_mfma_256<true, false>), grid, block, 0, s, A, Bt, C, M, N, K, cu_map, group_m);
  else if (v.vec_c)
    hipLaunchKernelGGL((gemm_bf16_mfma_256<false, true>), grid, block, 0, s, A, Bt, C, M, N, K, cu_map, group_m);
  else
    hipLaunchKernelGGL((gemm_bf16_mfma_256<false, false>), grid, block, 0, s, A, Bt, C, M, N, K, cu_map, group_m);
}

}  // namespace
