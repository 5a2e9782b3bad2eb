// The bf16 MFMA phase of a probe: the one GEMM dispatch, and the phase as launch / finish.
#pragma once

#include <cstdint>

#include "abft.h"
#include "arena.h"
#include "census.h"
#include "ctx.h"
#include "gemm_bf16.h"
#include "gemm_bf16_lab.h"  // the A/B variants: without it launch_gemm is launch_gemm_production alone
#include "options.h"
#include "report.h"

namespace {

constexpr int kCensusIters = 128;

// A variant that computes C (not a timing-only ablation) and the shape its tile divides.
inline bool gemm_args_ok(const GemmVariant& v, int m, int n, int k) {
  if (v.tile != 256 && v.tile != 128) return false;
  if (v.pipe != 0 && v.pipe != 1 && v.pipe != 2 && v.pipe != 3 && v.pipe != 21 && v.pipe != 22)
    return false;
  const int bm = v.tile == 256 ? G2_BM : BM, bn = v.tile == 256 ? G2_BN : BN, bk = v.tile == 256 ? G2_BK : BK;
  return m > 0 && n > 0 && k > 0 && m % bm == 0 && n % bn == 0 && k % bk == 0;
}

// The one kernel dispatch: the probe's MFMA phase and the host-buffer entry points both launch
// through it. The default variant is the production kernel; every other one is in the lab.
inline void launch_gemm(hipStream_t s, const GemmVariant& v, const short* A, const short* Bt, float* C, int M, int N, int K,
                        unsigned long long* cu_map, int group_m) {
  if (v.tile == 256 && v.pipe == kGemmPipe) launch_gemm_production(s, A, Bt, C, M, N, K, cu_map, group_m);
  else launch_gemm_lab(s, v, A, Bt, C, M, N, K, cu_map, group_m);
}

// The three parts of the phase share one view of it: the arena, the options, the stream, and the
// phase's counters. zero_in_kernel: the operand kernels zero those counters and the ABFT
// accumulators themselves.
struct MfmaPhase {
  char* base;
  const ArenaLayout& lay;
  const ProbeOptions& o;
  hipStream_t s;
  unsigned long long* cnt() const { return reinterpret_cast<unsigned long long*>(base + lay.cnt); }
  template <class T>
  T* at(size_t off) const {
    return reinterpret_cast<T*>(base + off);
  }
  void gemm(const short* a, const short* b, float* c, int nn, unsigned long long* cu_map) const {
    launch_gemm(s, o.gemm.variant, a, b, c, nn, nn, nn, cu_map, o.gemm.group_m);
  }
};

// (a) 256^3 full-element check vs the VALU reference; asymmetric operands
inline void enqueue_element_check(const MfmaPhase& ph) {
  const size_t n0 = 256;
  const bool zero_mfma = ph.o.zero_in_kernel;
  hipStream_t s = ph.s;
  unsigned long long* cnt = ph.cnt();
  auto *a0 = ph.at<short>(ph.lay.a0), *b0 = ph.at<short>(ph.lay.b0);
  auto *c0 = ph.at<float>(ph.lay.c0), *r0 = ph.at<float>(ph.lay.r0);
  const uint64_t e0 = static_cast<uint64_t>(n0) * n0;
  hipLaunchKernelGGL(gen_operand, dim3(256), dim3(256), 0, s, a0, e0, 0x1234u, 3,
                     zero_mfma ? reinterpret_cast<uint32_t*>(cnt + kSlotSmall) : nullptr,
                     zero_mfma ? static_cast<uint64_t>(kResSlots - kSlotSmall) * 2 : 0);
  hipLaunchKernelGGL(gen_operand, dim3(256), dim3(256), 0, s, b0, e0, 0xBEEFu, 3, static_cast<uint32_t*>(nullptr), 0);
  ph.gemm(a0, b0, c0, static_cast<int>(n0), nullptr);
  launch_gemm_ref(s, a0, b0, r0, static_cast<int>(n0), static_cast<int>(n0), static_cast<int>(n0));
  launch_count_diff(s, c0, r0, e0, cnt + kSlotSmall);
  PROBE_CHECK(hipGetLastError());
}

// (b) the N^3 GEMM, timed between e0 and e1, on fresh small-integer operands
inline void enqueue_timed_gemm(const MfmaPhase& ph, hipEvent_t ev0, hipEvent_t ev1) {
  const ProbeOptions& o = ph.o;
  const int gemm_n = o.gemm_n;
  const size_t n = static_cast<size_t>(gemm_n);
  const bool zero_mfma = o.zero_in_kernel;
  hipStream_t s = ph.s;
  unsigned long long* cnt = ph.cnt();
  auto *a = ph.at<short>(ph.lay.a), *b = ph.at<short>(ph.lay.b);
  auto* c = ph.at<float>(ph.lay.c);
  const uint64_t e = static_cast<uint64_t>(n) * n;
  // ABFT checksums: 6 uint32 vectors [acol | bcol | colsumC | expCol | rowsumC | expRow]; the first
  // three accumulate atomically and start from zero (zeroed by the operand kernel, or a memset)
  uint32_t* v32 = ph.at<uint32_t>(ph.lay.v);
  hipLaunchKernelGGL(gen_operand, dim3(2048), dim3(256), 0, s, a, e, 0x51u, 2, zero_mfma ? v32 : nullptr,
                     zero_mfma ? 3 * n : 0);
  hipLaunchKernelGGL(gen_operand, dim3(2048), dim3(256), 0, s, b, e, 0x77u, 2, static_cast<uint32_t*>(nullptr), 0);
  // test hook: C starts as all-ones words (NaN) so a tile the GEMM never writes fails the checks
  // instead of passing on the previous run's identical result (the arena is reused)
  if (o.gemm.poison_c) PROBE_CHECK(hipMemsetAsync(c, 0xFF, n * n * sizeof(float), s));
  // the 256^3 check above already ran this kernel's code object: time the first launch
  PROBE_CHECK(hipEventRecord(ev0, s));
  for (int rep = 0; rep < o.reps; ++rep) ph.gemm(a, b, c, gemm_n, cnt + kSlotGemmMap);  // reps 0: test hook
  PROBE_CHECK(hipEventRecord(ev1, s));
  PROBE_CHECK(hipGetLastError());
  const int64_t at = o.inject_gemm_at.index(gemm_n);
  if (o.inject_gemm && at >= 0) hipLaunchKernelGGL(inject_gemm_fault, dim3(1), dim3(1), 0, s, c, at, o.inject_gemm);
}

// ...and its exact u32 (mod 2^32) ABFT row / column checksums
inline void enqueue_abft(const MfmaPhase& ph) {
  const int gemm_n = ph.o.gemm_n;
  const size_t n = static_cast<size_t>(gemm_n);
  const bool zero_mfma = ph.o.zero_in_kernel;
  hipStream_t s = ph.s;
  unsigned long long* cnt = ph.cnt();
  auto *a = ph.at<short>(ph.lay.a), *b = ph.at<short>(ph.lay.b);
  auto* c = ph.at<float>(ph.lay.c);
  uint32_t* v32 = ph.at<uint32_t>(ph.lay.v);
  uint32_t *vacol = v32, *vbcol = v32 + n, *vcolC = v32 + 2 * n, *vexpC = v32 + 3 * n, *vrowC = v32 + 4 * n,
           *vexpR = v32 + 5 * n;
  if (!zero_mfma) PROBE_CHECK(hipMemsetAsync(v32, 0, 3 * n * sizeof(uint32_t), s));
  const float bound = static_cast<float>(gemm_n) * 4.0f;  // |C| <= K * span^2, span 2
  unsigned long long* bad = cnt + kSlotAbft;
  enqueue_abft(s, a, b, c, gemm_n, gemm_n, gemm_n, bound, AbftVectors{vacol, vbcol, vcolC, vexpC, vrowC, vexpR},
               AbftCounters{bad, bad, bad});
}

// Enqueues the whole MFMA phase on stream s (no host sync): (a) a 256^3 GEMM checked element by
// element against the VALU reference, (b) the timed N^3 GEMM (events ctx.gev[0..1]) with its ABFT
// checksums, (c) the census; then copies the phase's counters to
// ctx.host_res[kSlotSmall..kResSlots). Operands at ``lay`` in the arena ``base``.
inline void launch_mfma_phase(char* base, const ArenaLayout& lay, const ProbeOptions& o, DeviceCtx& ctx, hipStream_t s) {
  const MfmaPhase ph{base, lay, o, s};
  unsigned long long* cnt = ph.cnt();
  enqueue_element_check(ph);
  enqueue_timed_gemm(ph, ctx.gev[0], ctx.gev[1]);
  enqueue_abft(ph);
  // (c) every CU's matrix cores: the census (the GEMM above marked the CUs that ran its tiles)
  hipLaunchKernelGGL(cu_census, dim3(8 * ctx.prop.multiProcessorCount), dim3(kCensusThreads), 0, s, cnt + kSlotCensusMap,
                     cnt + kSlotCensusBad, kCensusIters, 0xC0FFEEu ^ static_cast<uint32_t>(o.gemm_n), o.census_fault_xcc);
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipMemcpyAsync(ctx.host_res + kSlotSmall, cnt + kSlotSmall,
                             (kResSlots - kSlotSmall) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
}

// After the stream's synchronise: the timed GEMM's rate, the counters and the two CU maps -> the
// "mfma" and "cus" blocks. Every CU the runtime reports must have proven its matrix cores
// (requireAllCUs, default on).
inline void finish_mfma(const ProbeOptions& o, DeviceCtx& ctx, MfmaResult* m, CusResult* cu) {
  const unsigned long long* hres = ctx.host_res;
  float ms;
  PROBE_CHECK(hipEventElapsedTime(&ms, ctx.gev[0], ctx.gev[1]));
  m->ms = o.reps > 0 ? ms / o.reps : 0.0;
  m->tflops = gemm_tflops(o.gemm_n, m->ms);
  m->small_bad = hres[kSlotSmall];
  m->abft_bad = hres[kSlotAbft];
  const CuCount census = count_cus(hres + kSlotCensusMap);
  cu->expected = ctx.prop.multiProcessorCount;
  cu->verified = census.total;
  for (int x = 0; x < 8; ++x) cu->per_xcd[x] = census.per_xcc[x];
  cu->gemm_tiles = count_cus(hres + kSlotGemmMap).total;
  cu->bad_waves = hres[kSlotCensusBad];
  cu->want_keys = o.cu_keys;
  if (o.cu_keys)  // the (xcc, se, sh, cu) key of every CU that proved its MFMA (isolation tests)
    for (int k = 0; k < kCuKeys; ++k)
      if (hres[kSlotCensusMap + k / 64] >> (k % 64) & 1ull) cu->keys.push_back(k);
  const bool cus_ok = !o.require_all_cus || cu->verified >= cu->expected;
  m->ok = m->small_bad == 0 && m->abft_bad == 0 && cu->bad_waves == 0 && cus_ok;
}

}  // namespace
