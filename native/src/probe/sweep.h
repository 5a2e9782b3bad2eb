// The rotating HBM sweep (mi355x_probe_hbm_sweep and the sweep buffer's alloc / release): the
// claim-time probe always tests the same ~1 GiB arena; this walks the rest of the 288 GB.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>

#include "ctx.h"
#include "hbm.h"
#include "options.h"
#include "report.h"
#include "sweep_window.h"  // kSweepChunk and how a window splits over the chunks

namespace {

// All free HBM minus ``reserve``, 2 MiB granular, as kSweepChunk pieces. Measured on MI355X
// (profiles/r2h_sweep_claim_diag.txt): ~0.2 s to allocate ~282 GiB of fresh VRAM, ~6 s once the
// driver must clear previously used VRAM; neither runs under the device lock a probe takes.
// Claim-time probes running per device (mi355x_probe_run). Mapping or unmapping the sweep buffer
// stalls a probe that runs beside it — up to the whole 6 s allocation when the driver is still
// clearing the previous buffer, 5-211 ms per chunk otherwise (profiles/r4p_probe_during_sweep_free.json)
// — so the lock-free sweep alloc / free paths wait between chunks while a probe runs: a probe then
// shares the device with at most one chunk operation (the scrubber avoids the pending clear).
// Counted over all devices: the HIP runtime serialises parts of an allocation process-wide, so a
// chunk mapped on one GPU can hold up a probe launching on another (an 8-GPU node scrubs idle GPUs
// while claims probe the others).
std::atomic<int> g_probes_active{0};

struct ProbeActive {
  ProbeActive() { g_probes_active.fetch_add(1); }
  ~ProbeActive() { g_probes_active.fetch_sub(1); }
};

// Wait until no claim-time probe runs in this process; dev -1: never wait (callers holding a
// device lock). Bounded twice: at most 2 s before one chunk, and at most ``budget`` (what is left of
// the whole alloc / free call's 3 s) over all its chunks — ~282 chunks under steady claim traffic
// must not turn a free into minutes while the pod's Allocate waits for it. In the agent's probe
// helpers a process holds one GPU, so only probes of that GPU are waited for. Returns the seconds
// spent waiting (the sweep trace reports them).
inline double yield_to_probes(int dev, double* budget) {
  static const bool off = std::getenv("GPUPOOL_SWEEP_NO_YIELD") != nullptr;  // in-process A/B only
  if (dev < 0 || off || !budget || *budget <= 0) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  const auto deadline = t0 + std::chrono::duration<double>(std::min(2.0, *budget));
  while (g_probes_active.load() > 0 && std::chrono::steady_clock::now() < deadline)
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *budget -= waited;
  return waited;
}

constexpr double kYieldBudgetS = 3.0;  // per sweep-buffer alloc / free call, over all its chunks

inline SweepBuf sweep_alloc_raw(uint64_t reserve, int yield_dev = -1) {
  size_t free_b = 0, total_b = 0;
  PROBE_CHECK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t gran = 2ull << 20;
  if (free_b <= reserve + gran) throw ProbeError("not enough free HBM for a sweep window");
  SweepBuf b;
  const uint64_t span = ((free_b - reserve) / gran) * gran;
  double budget = kYieldBudgetS, yielded = 0;
  static const bool trace = std::getenv("GPUPOOL_SWEEP_TRACE") != nullptr;  // chunk timings
  for (uint64_t at = 0; at < span; at += kSweepChunk) {
    void* p = nullptr;
    yielded += yield_to_probes(yield_dev, &budget);
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(&p, std::min<uint64_t>(kSweepChunk, span - at));
    if (e != hipSuccess) {
      for (void* q : b.chunks) (void)hipFree(q);
      (void)hipGetLastError();
      throw ProbeError(std::string("sweep chunk hipMalloc: ") + hipGetErrorString(e));
    }
    b.chunks.push_back(p);
    if (trace) std::fprintf(stderr, "sweep chunk %zu: %.3f ms\n", b.chunks.size() - 1, ms_since(t0));
  }
  if (trace) std::fprintf(stderr, "sweep alloc: %zu chunks, %.1f ms yielded to probes\n", b.chunks.size(), yielded * 1e3);
  b.span = span;
  return b;
}

inline void sweep_free(SweepBuf& b, int yield_dev = -1) {
  double budget = kYieldBudgetS, yielded = 0;
  for (void* p : b.chunks) {  // one bounded unmap per chunk
    yielded += yield_to_probes(yield_dev, &budget);
    (void)hipFree(p);
  }
  static const bool trace = std::getenv("GPUPOOL_SWEEP_TRACE") != nullptr;
  if (trace) std::fprintf(stderr, "sweep free: %zu chunks, %.1f ms yielded to probes\n", b.chunks.size(), yielded * 1e3);
  b.chunks.clear();
  b.span = 0;
}

// One piece of a window inside one chunk: both polarities, one sync. Adds its time and counters to
// ``r``; ``chunk0``: the piece's first 16-byte chunk counted from the window's start. Test hooks,
// both after the first fill: ``inject_flips`` bits spread over the piece, bit 0 of the piece's
// chunk ``flip_at`` (-1: none).
inline void sweep_piece(DeviceCtx& ctx, const PatternPass& pass, int inject_flips, long long flip_at, uint64_t chunk0,
                        SweepResult* r) {
  unsigned long long* cnt = ctx.sweep_cnt;
  memset_pairs(pass.s, cnt, 4, 2);
  PROBE_CHECK(hipEventRecord(ctx.ev[0], pass.s));
  for (int pi = 0; pi < 2; ++pi) {
    pass.fill(pi);
    if (pi == 0 && inject_flips > 0) pass.inject_flips(inject_flips);
    if (pi == 0 && flip_at >= 0) pass.inject_flip_at(static_cast<uint64_t>(flip_at));
    pass.verify(pi, cnt + 2 * pi);
  }
  PROBE_CHECK(hipEventRecord(ctx.ev[1], pass.s));
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipMemcpyAsync(ctx.host_res, cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, pass.s));
  PROBE_CHECK(hipStreamSynchronize(pass.s));
  float piece_ms = 0;
  PROBE_CHECK(hipEventElapsedTime(&piece_ms, ctx.ev[0], ctx.ev[1]));
  r->ms += piece_ms;
  HbmResult piece;
  fold_pairs(ctx.host_res, 2, &piece);
  r->bad_bits += piece.bad_bits;
  if (piece.first_bad != ~0ull) r->first_bad = std::min(r->first_bad, chunk0 + piece.first_bad);
}

// One window of the rotating HBM sweep (see mi355x_probe_hbm_sweep in probe.h): a buffer of all
// free HBM minus ``reserve`` is allocated once per scrub pass (kept while ``keep``), and each call
// pattern-tests [offset, offset+bytes) of it with the same fill/verify kernels and both polarities.
inline std::string run_sweep(int dev, const char* opts) {
  const SweepOptions o = SweepOptions::parse(opts);
  DeviceCtx& ctx = ensure_ctx(dev);
  auto t0 = std::chrono::steady_clock::now();
  SweepResult r;
  r.dev = dev;
  if (ctx.sweep.empty()) {  // normally pre-allocated by mi355x_probe_sweep_alloc outside the device lock
    ctx.sweep = sweep_alloc_raw(o.reserve);
    r.alloc_ms = ms_since(t0);
  }
  r.span = ctx.sweep.span;
  const SweepWindow w = sweep_window(ctx.sweep.span, kSweepChunk, o.offset, o.bytes);
  r.offset = w.offset;
  r.bytes = w.bytes;
  if (!ctx.sweep_cnt) PROBE_CHECK(hipMalloc(reinterpret_cast<void**>(&ctx.sweep_cnt), 4 * sizeof(unsigned long long)));
  const int cus = ctx.prop.multiProcessorCount;
  // the window may straddle chunks: test it piece by piece (both polarities per piece)
  for (const SweepPiece& p : w.pieces) {
    PatternPass pass;
    pass.s = ctx.stream;
    pass.buf = reinterpret_cast<u32x4*>(static_cast<char*>(ctx.sweep.chunks[p.chunk]) + p.in);
    pass.n16 = p.bytes / 16;
    pass.seed = p.seed;
    pass.fill_grid = hbm_grid(cus, kHbmFillBlocksPerCU, pass.n16);
    pass.verify_grid = hbm_grid(cus, kHbmVerifyBlocksPerCU, pass.n16);
    // "injectFlipAtChunk" counts from the window's start and strikes the piece that holds that chunk
    const bool flip_here = o.inject_chunk >= 0 && static_cast<uint64_t>(o.inject_chunk) >= p.first16 &&
                           static_cast<uint64_t>(o.inject_chunk) - p.first16 < pass.n16;
    sweep_piece(ctx, pass, p.first16 == 0 ? o.inject_flips : 0,
                flip_here ? o.inject_chunk - static_cast<long long>(p.first16) : -1, p.first16, &r);
  }
  if (!o.keep) sweep_free(ctx.sweep);
  return sweep_report(r);
}

}  // namespace
