// What checks a GEMM's result without trusting the matrix cores: small-integer operands (every
// partial sum exact in fp32), a VALU reference for the element-by-element check, and exact ABFT
// row / column checksums mod 2^32. Shared by the bf16 phase and the low-precision phase (lowp.h).
#pragma once

#include <cstdint>

#include "hbm.h"  // pattern_word
#include "types.h"

namespace {

// ------------------------------------------------------------------ operand generation
__device__ __forceinline__ short small_int_bf16(uint32_t h, int span) {
  // Integer in [-span, span] encoded as bf16 (exact).
  float v = static_cast<float>(static_cast<int>(h % static_cast<uint32_t>(2 * span + 1)) - span);
  return static_cast<short>(__float_as_uint(v) >> 16);
}

// ``zero``/``nzero``: the grid also zeroes nzero words (the MFMA phase's result slots, its ABFT
// accumulators), so that phase's stream needs no memsets and no hand-off from the HBM stream.
__global__ void gen_operand(short* __restrict__ out, uint64_t n, uint32_t seed, int span,
                            uint32_t* __restrict__ zero, uint64_t nzero) {
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < nzero;
       j += static_cast<uint64_t>(gridDim.x) * blockDim.x)
    zero[j] = 0u;
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  for (; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
    out[i] = small_int_bf16(pattern_word(i, seed), span);
}

__device__ __forceinline__ float bf16_to_f32(short s) {
  return __uint_as_float(static_cast<uint32_t>(static_cast<uint16_t>(s)) << 16);
}
// Full VALU reference (independent of the matrix cores), fp32, k-ordered.
// One thread per output; both operand rows read with 16-byte loads (K % 8 == 0).
__global__ void gemm_ref_valu(const short* __restrict__ A, const short* __restrict__ Bt,
                              float* __restrict__ C, int M, int N, int K) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  int m = blockIdx.y;
  if (n >= N || m >= M) return;
  const bf16x8* a = reinterpret_cast<const bf16x8*>(A + static_cast<int64_t>(m) * K);
  const bf16x8* b = reinterpret_cast<const bf16x8*>(Bt + static_cast<int64_t>(n) * K);
  float s = 0.f;
  for (int k8 = 0; k8 < K / 8; ++k8) {
    const bf16x8 av = a[k8], bv = b[k8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s = fmaf(bf16_to_f32(av[j]), bf16_to_f32(bv[j]), s);
  }
  C[static_cast<int64_t>(m) * N + n] = s;
}

// Bit-exact: the words are compared, so a zero of the other sign differs and a NaN equals the NaN
// of the same bits.
__global__ void count_diff(const float* __restrict__ x, const float* __restrict__ y, uint64_t n,
                           unsigned long long* __restrict__ bad) {
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  uint32_t b = 0;
  for (; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x) b += __float_as_uint(x[i]) != __float_as_uint(y[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) b += __shfl_xor(b, off, 64);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(bad, static_cast<unsigned long long>(b));
}

// The element check's two launches, as the probe and the host-buffer test surfaces share them: the
// reference of C[m][n] = A[m][k] * Bt[n][k]^T (k % 8 == 0), and count_diff with its one grid.
inline void launch_gemm_ref(hipStream_t s, const short* a, const short* bt, float* r, int m, int n, int k) {
  hipLaunchKernelGGL(gemm_ref_valu, dim3((n + 255) / 256, m), dim3(256), 0, s, a, bt, r, m, n, k);
}
inline void launch_count_diff(hipStream_t s, const float* x, const float* y, uint64_t count, unsigned long long* bad) {
  hipLaunchKernelGGL(count_diff, dim3(64), dim3(256), 0, s, x, y, count, bad);
}

// ABFT (algorithm-based fault tolerance) checks. Every operand is a small integer, so with
// C = A * Bt^T these identities hold over the integers, and therefore modulo 2^32:
//   column checksum  sum_m C[m][n] == sum_k (sum_m A[m][k]) * Bt[n][k]
//   row checksum     sum_n C[m][n] == sum_k A[m][k] * (sum_n Bt[n][k])
// All arithmetic is unsigned 32-bit (wraps exactly; a corrupted element changes a sum by a
// non-multiple of 2^32). Two memory-bound primitives with 16-byte loads per lane and four loads in
// flight (profiles/r1q: the former 2-byte-load / int64 versions took ~0.5 ms per probe, 4-5x the
// GEMM they check).
__device__ __forceinline__ uint32_t to_u32(short v) { return static_cast<uint32_t>(static_cast<int>(bf16_to_f32(v))); }
__device__ __forceinline__ uint32_t to_u32(float v) {
  // clamp first: an out-of-range float-to-int conversion is undefined (colsum_partial flags it).
  // Rounded down, not towards zero: an element that gained a fraction keeps its integer part
  // whatever its sign, so it is the integrality flag alone that reports it.
  return static_cast<uint32_t>(static_cast<int>(floorf(fminf(fmaxf(v, -2.0e9f), 2.0e9f))));
}

constexpr int kColRows = 64;  // rows per colsum_partial block (4 waves x 16 interleaved rows)
constexpr int kUnroll = 4;    // independent 16-byte loads in flight per lane

// Column sums: a lane owns V = 16/sizeof(T) adjacent columns (one 16-byte load per row); the
// block's 4 waves take interleaved rows of a kColRows chunk, combine through LDS, and add one
// 32-bit atomic per column. cols % V == 0.
// For the fp32 product C the same pass also flags any element that is not an exact integer, is
// not finite, or exceeds ``bound`` (= K * span^2): a corrupted element that keeps its integer part
// (a low-mantissa flip) or wraps the int cast would otherwise leave the mod-2^32 sums intact.
template <class T>
__global__ __launch_bounds__(256) void colsum_partial(const T* __restrict__ X, int rows, int cols,
                                                      uint32_t* __restrict__ out, float bound,
                                                      unsigned long long* __restrict__ bad) {
  constexpr int V = 16 / sizeof(T);
  using vec = __attribute__((ext_vector_type(V))) T;
  __shared__ uint32_t part[4][64 * V];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cb = blockIdx.x * 64 * V;
  const int c0 = cb + lane * V;
  const int r0 = blockIdx.y * kColRows;
  const int r1 = min(rows, r0 + kColRows);
  uint32_t acc[V] = {};
  uint32_t odd = 0;
  if (c0 < cols) {
    for (int r = r0 + wave; r < r1; r += 4 * kUnroll) {
      vec v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
        if (r + 4 * u < r1) v[u] = *reinterpret_cast<const vec*>(X + static_cast<int64_t>(r + 4 * u) * cols + c0);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
        if (r + 4 * u < r1) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T x = static_cast<T>(v[u][j]);
            if constexpr (sizeof(T) == 4) odd += !(x == rintf(x) && fabsf(x) <= bound);  // NaN fails both
            acc[j] += to_u32(x);
          }
        }
    }
  }
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) odd += __shfl_xor(odd, off, 64);
    if (lane == 0 && odd && bad) atomicAdd(bad, static_cast<unsigned long long>(odd));
  }
#pragma unroll
  for (int j = 0; j < V; ++j) part[wave][lane * V + j] = acc[j];
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * V && cb + i < cols; i += 256)
    atomicAdd(&out[cb + i], part[0][i] + part[1][i] + part[2][i] + part[3][i]);
}

// out[r] = sum_k X[r][k] * w[k] mod 2^32 (w = nullptr: plain row sums); one wave64 per row, 4 rows
// per block. The 32-bit weights (colsum_partial's output) are read with 16-byte loads and stay in
// L1/L2 (K * 4 bytes). K % V == 0.
template <class T>
__global__ __launch_bounds__(256) void rowdot(const T* __restrict__ X, int rows, int K, const uint32_t* __restrict__ w,
                                              uint32_t* __restrict__ out) {
  constexpr int V = 16 / sizeof(T);
  using vec = __attribute__((ext_vector_type(V))) T;
  using wvec = __attribute__((ext_vector_type(V))) uint32_t;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const T* x = X + static_cast<int64_t>(row) * K;
  uint32_t s = 0;
  for (int k0 = lane * V; k0 < K; k0 += 64 * V * kUnroll) {
    vec v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (k0 + u * 64 * V < K) v[u] = *reinterpret_cast<const vec*>(x + k0 + u * 64 * V);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int k = k0 + u * 64 * V;
      if (k >= K) break;
      if (w) {
        const wvec wv = *reinterpret_cast<const wvec*>(w + k);
#pragma unroll
        for (int j = 0; j < V; ++j) s += to_u32(static_cast<T>(v[u][j])) * wv[j];
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) s += to_u32(static_cast<T>(v[u][j]));
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) out[row] = s;
}

// ---- fault injection (test hook: proves the checkers catch corruption on real hardware)
// mode 1: +1.0 (an integer error: caught by the mod-2^32 checksums); mode 2: +0.25 (the integer
// part survives: caught only by the integrality check); mode 3: NaN.
__global__ void inject_gemm_fault(float* __restrict__ c, int64_t idx, int mode) {
  if (mode == 1) c[idx] += 1.0f;
  else if (mode == 2) c[idx] += 0.25f;
  else c[idx] = __int_as_float(0x7fc00000);
}

// test surface (mi355x_probe_abft_check): one element of C set to a value the host chose
__global__ void poke_f32(float* __restrict__ c, int64_t idx, float v) { c[idx] = v; }

__global__ void count_ne_u32(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, int n,
                             unsigned long long* __restrict__ bad) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t d = (i < n && a[i] != b[i]) ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
  if ((threadIdx.x & 63) == 0 && d) atomicAdd(bad, static_cast<unsigned long long>(d));
}

// The six checksum vectors of one C[m][n] = A[m][k] * Bt[n][k]^T, of K, K, N, N, M and M words:
// column sums of A and of Bt, column sums of C and what they must be, row sums of C and what they
// must be. Each at least 32-byte aligned (rowdot<short> loads eight weights at once). The first
// three accumulate atomically: the caller zeroes them on the stream first.
struct AbftVectors {
  uint32_t *acol, *bcol, *col_c, *exp_col, *row_c, *exp_row;
};
// Where the checks count: elements of C that are no integer, not finite or beyond the bound; column
// checksums that differ; row checksums that differ. A probe points all three at its one ABFT slot.
struct AbftCounters {
  unsigned long long *odd, *col, *row;
};

// The checks on C that read no operand, shared by the bf16 and the low-precision sequence: the
// column sums with the integrality / range flag, and the row sums.
inline void enqueue_abft_c_colsum(hipStream_t s, const float* c, int m, int n, float bound, const AbftVectors& v,
                                  const AbftCounters& cnt) {
  const dim3 grid((n + 255) / 256, (m + kColRows - 1) / kColRows);
  hipLaunchKernelGGL(colsum_partial<float>, grid, dim3(256), 0, s, c, m, n, v.col_c, bound, cnt.odd);
}
inline void enqueue_abft_c_rowsum(hipStream_t s, const float* c, int m, int n, const AbftVectors& v) {
  hipLaunchKernelGGL(rowdot<float>, dim3((m + 3) / 4), dim3(256), 0, s, c, m, n, static_cast<const uint32_t*>(nullptr),
                     v.row_c);
}
inline void enqueue_abft_compare(hipStream_t s, int m, int n, const AbftVectors& v, const AbftCounters& cnt) {
  hipLaunchKernelGGL(count_ne_u32, dim3((n + 255) / 256), dim3(256), 0, s, static_cast<const uint32_t*>(v.col_c),
                     static_cast<const uint32_t*>(v.exp_col), n, cnt.col);
  hipLaunchKernelGGL(count_ne_u32, dim3((m + 255) / 256), dim3(256), 0, s, static_cast<const uint32_t*>(v.row_c),
                     static_cast<const uint32_t*>(v.exp_row), m, cnt.row);
}

// The bf16 checker sequence on stream s (no host sync): A [m][k], Bt [n][k] bf16 small integers,
// C [m][n] fp32; k % 8 == 0, n % 4 == 0. bound: the largest |C| the operands allow.
inline void enqueue_abft(hipStream_t s, const short* a, const short* bt, const float* c, int m, int n, int k, float bound,
                         const AbftVectors& v, const AbftCounters& cnt) {
  const dim3 agrid((k + 511) / 512, (m + kColRows - 1) / kColRows), bgrid((k + 511) / 512, (n + kColRows - 1) / kColRows);
  hipLaunchKernelGGL(colsum_partial<short>, agrid, dim3(256), 0, s, a, m, k, v.acol, 0.f,
                     static_cast<unsigned long long*>(nullptr));
  hipLaunchKernelGGL(colsum_partial<short>, bgrid, dim3(256), 0, s, bt, n, k, v.bcol, 0.f,
                     static_cast<unsigned long long*>(nullptr));
  enqueue_abft_c_colsum(s, c, m, n, bound, v, cnt);
  hipLaunchKernelGGL(rowdot<short>, dim3((n + 3) / 4), dim3(256), 0, s, bt, n, k, static_cast<const uint32_t*>(v.acol),
                     v.exp_col);
  enqueue_abft_c_rowsum(s, c, m, n, v);
  hipLaunchKernelGGL(rowdot<short>, dim3((m + 3) / 4), dim3(256), 0, s, a, m, k, static_cast<const uint32_t*>(v.bcol),
                     v.exp_row);
  enqueue_abft_compare(s, m, n, v, cnt);
}

}  // namespace
