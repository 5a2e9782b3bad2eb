// mi355x-probe: per-device readiness check for gfx950 (MI355X), the MI355X-native replacement for
// the reference's GPU smoke test (`kubectl run ... nvidia-smi`, GPU调度平台搭建.md:134-138).
//
// A device passes only if
//   1. HBM: two complementary pseudo-random patterns written over `hbmBytes` of HBM3E and read
//      back bit-exactly (stuck-at / coupling faults in both polarities), with the achieved
//      write+read bandwidth reported;
//   2. MFMA: a bf16 GEMM on the matrix cores (`v_mfma_f32_16x16x32_bf16`) is bit-exact against
//      (a) a full VALU fp32 reference on a 256^3 problem with an asymmetric B (catches fragment
//      layout / row<->col faults) and (b) exact u32 (mod 2^32) ABFT row+column checksums on an N^3 problem
//      whose operands are small integers (all partial sums exact in fp32), with TFLOP/s reported.
//
// Design for CDNA4: 64-wide waves; 16-byte vector loads/stores everywhere (Guideline 13);
// HBM kernels grid-stride with 1 (fill) and 3 (verify) workgroups per CU and 4 independent 16-B
// accesses in flight per lane; the GEMM (gemm_bf16_mfma_256p) uses a 256x256x64 tile, 8 waves each
// owning a 64x32 block of every 128x128 quadrant, operands DMA'd HBM->LDS with global_load_lds (two
// stages, XOR-swizzled) in half-tiles that stay in flight across barriers (counted vmcnt), the two
// wave groups one barrier apart, and an XCD-aware bijective workgroup remap (T1) so neighbouring
// tiles share an XCD's L2. Host side: one arena allocation per probe, pinned result slots and one
// stream sync per phase.
//
// This file is the claim probe as a sequence of steps (run_probe) and the C surface. The pieces:
//   types.h          vector types, ProbeError, PROBE_CHECK
//   options.h        every option of every entry point, read once (pure host, unit-tested)
//   arena.h          the layout of the probe's one allocation (pure host, unit-tested)
//   report.h         result structs -> the JSON reports (pure host, unit-tested)
//   hbm.h            pattern kernels and the pattern pass shared by probe, peer checks and sweep
//   census.h         CU identity, the per-CU MFMA census, and the CU-map fold of the per-CU phases
//   gemm_bf16.h      the production GEMM kernel; gemm_bf16_lab.h its A/B siblings
//   abft.h           operand generation, VALU reference, ABFT checksums
//   mfma_phase.h     the GEMM dispatch and the bf16 MFMA phase (launch / finish)
//   lowp.h           FP8 / MXFP8 / MXFP4 phase ("mfmaLowPrecision")
//   hostlink.h       PCIe host-link phase ("hostLinkBytes")
//   lds.h            per-CU LDS march and address test ("ldsCheck")
//   regfile.h        per-SIMD vector register file march ("regCheck")
//   alu.h            per-SIMD vector-ALU instruction program ("aluCheck"); alu_ref.h its host expectation
//   atomics.h        LDS, L2 and device-scope atomic units ("atomCheck"); atomics_ref.h its host expectation
//   ctx.h            per-device state, ensure_ctx() and CounterSets, the two counter sets (and their
//                    make / reset / run / end protocol) that each of the four phases above keeps
//   peer.h           the xGMI checks; sweep.h the HBM sweep
//   sweep_window.h   a sweep window split over the buffer's chunks (pure host, unit-tested)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "mi355x/probe.h"

#include "arena.h"
#include "ctx.h"
#include "hbm.h"
#include "hostlink.h"
#include "lds.h"
#include "lowp.h"
#include "mfma_phase.h"
#include "options.h"
#include "alu.h"
#include "atomics.h"
#include "regfile.h"
#include "peer.h"
#include "report.h"
#include "sweep.h"
#include "types.h"

namespace {

char* dup(const std::string& s) {
  char* p = static_cast<char*>(std::malloc(s.size() + 1));
  std::memcpy(p, s.c_str(), s.size() + 1);
  return p;
}

// ------------------------------------------------------------------ the claim probe, step by step
// The low-precision phase's events and pinned counters, made by the first probe that asks for a dtype.
void ensure_lowp(DeviceCtx& ctx) {
  if (ctx.host_lowp) return;
  for (auto& pair : ctx.lev)
    for (auto& e : pair) PROBE_CHECK(hipEventCreate(&e));
  PROBE_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ctx.host_lowp),
                            lowp::kDtypes * lowp::kSlots * sizeof(unsigned long long)));
}

// With overlap the host-link phase has a stream of its own ("hostLinkStream":1: the tail of the
// MFMA stream instead, for the A/B), made like its buffer by the first probe that asks; serial
// (floors), it runs last on the one stream, alone on the GPU.
hipStream_t host_link_stream(DeviceCtx& ctx, const ProbeOptions& o) {
  if (!o.overlap) return ctx.stream;
  if (o.host_link_on_mfma_stream) return ctx.stream2;
  if (!ctx.hl_stream) PROBE_CHECK(hipStreamCreateWithFlags(&ctx.hl_stream, hipStreamNonBlocking));
  return ctx.hl_stream;
}

// The arena of at least ``need`` bytes: the kept one unless it is too small or more than twice too
// large. !keep: ``transient`` owns it for this probe only.
char* acquire_arena(DeviceCtx& ctx, size_t need, bool keep, DevBuf* transient, bool* reused) {
  if (ctx.arena && (ctx.arena_bytes < need || ctx.arena_bytes > 2 * need)) {
    (void)hipFree(ctx.arena);
    ctx.arena = nullptr;
    ctx.arena_bytes = 0;
  }
  *reused = ctx.arena != nullptr;
  if (!ctx.arena) {
    PROBE_CHECK(hipMalloc(&ctx.arena, need));
    ctx.arena_bytes = need;
  }
  ctx.arena_used = std::chrono::steady_clock::now();
  if (keep) return static_cast<char*>(ctx.arena);
  transient->p = ctx.arena;
  ctx.arena = nullptr;
  ctx.arena_bytes = 0;
  return static_cast<char*>(transient->p);
}

// counters: [2p] = flipped bits, [2p+1] = first bad 16-B index (init all-ones) of pattern p, then
// the MFMA phase's counters. With zeroInKernel (default) the kernels reset them and nothing is
// enqueued here; else memsets on s, and s2 waits for them.
void reset_counters(DeviceCtx& ctx, const ProbeOptions& o, unsigned long long* cnt, hipStream_t s, hipStream_t s2) {
  if (o.zero_in_kernel) return;
  memset_pairs(s, cnt, kResSlots, o.patterns);
  if (o.overlap) {
    PROBE_CHECK(hipEventRecord(ctx.gev[2], s));
    PROBE_CHECK(hipStreamWaitEvent(s2, ctx.gev[2], 0));
  }
}

// The low-precision phase follows the bf16 MFMA phase on its stream, in its own part of the arena.
lowp::Phase lowp_phase(DeviceCtx& ctx, const ProbeOptions& o, char* base, const ArenaLayout& lay) {
  lowp::Phase lp;
  lp.mask = o.lowp_mask;
  lp.region = base + lay.lowp_region;
  lp.cnt = reinterpret_cast<unsigned long long*>(base + lay.lowp_cnt);
  lp.host = ctx.host_lowp;
  lp.ev = ctx.lev;
  lp.gemm_n = o.gemm_n;
  lp.cus = ctx.prop.multiProcessorCount;
  lp.inject_mask = o.inject_lowp;
  lp.inject_at = o.inject_gemm_at.index(o.gemm_n);
  lp.census_fault_xcc = o.lowp_census_fault_xcc;
  lp.poison_c = o.gemm.poison_c;
  return lp;
}

// The HBM test of a claim probe: the arena's pattern region on the device's first stream.
PatternPass hbm_pass(DeviceCtx& ctx, const ProbeOptions& o, int dev, char* base, const ArenaLayout& lay, uint64_t n16) {
  PatternPass pass;
  pass.s = ctx.stream;
  pass.buf = reinterpret_cast<u32x4*>(base + lay.hbm);
  pass.n16 = n16;
  pass.seed = 0xA5A50000u + static_cast<uint32_t>(dev);
  pass.fill_grid = hbm_grid(ctx.prop.multiProcessorCount, o.fill_blocks_per_cu, n16);
  pass.verify_grid = hbm_grid(ctx.prop.multiProcessorCount, o.verify_blocks_per_cu, n16);
  pass.cheap = o.cheap_pattern;
  pass.tiled = o.tiled;
  return pass;
}

// HBM: all patterns back to back on the pass's stream, per-pattern counters and events, then the
// counters' copy. ``after_first_fill``: where "hbmFirst":2 enqueues the MFMA phase.
template <class F>
void enqueue_hbm(DeviceCtx& ctx, const PatternPass& pass, const ProbeOptions& o, unsigned long long* cnt,
                 F&& after_first_fill) {
  PROBE_CHECK(hipEventRecord(ctx.ev[0], pass.s));
  for (int pi = 0; pi < o.patterns; ++pi) {
    unsigned long long* reset = o.zero_in_kernel && pi == 0 ? cnt : nullptr;
    pass.fill(pi, reset, reset ? o.patterns : 0);
    PROBE_CHECK(hipEventRecord(ctx.ev[1 + 2 * pi], pass.s));
    if (pi == 0) {
      after_first_fill();
      if (o.inject_flips > 0) pass.inject_flips(o.inject_flips);
      if (o.inject_chunk >= 0 && static_cast<uint64_t>(o.inject_chunk) < pass.n16)
        pass.inject_flip_at(static_cast<uint64_t>(o.inject_chunk));
    }
    pass.verify(pi, cnt + 2 * pi);
    PROBE_CHECK(hipEventRecord(ctx.ev[2 + 2 * pi], pass.s));
  }
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipMemcpyAsync(ctx.host_res, cnt, 2 * o.patterns * sizeof(unsigned long long), hipMemcpyDeviceToHost, pass.s));
}

// One opt-in per-CU phase of a claim probe (lds.h, regfile.h, alu.h, atomics.h share the shape
// ensure / launch / finish): its plan, whether it goes ahead of the MFMA phase on that phase's
// stream, where its result goes in the report, and whether it is still to be enqueued.
template <class Plan, class Result>
struct Check {
  Plan plan;
  bool on, first;
  bool* has;
  Result* out;
  bool pending = on;
};

std::string run_probe(int dev, const char* opts) {
  const ProbeOptions o = ProbeOptions::parse(opts, dev);
  auto t0 = std::chrono::steady_clock::now();
  DeviceCtx& ctx = ensure_ctx(dev);
  if (o.lowp_mask) ensure_lowp(ctx);
  hostlink::Plan hl = o.host_link;
  hipStream_t s = ctx.stream, s2 = o.overlap ? ctx.stream2 : s, hl_s = s;
  if (hl.n16) {
    hl.alloc_ms = hostlink::ensure(ctx, hl.n16 * 16, hl.coherent);
    hl_s = host_link_stream(ctx, o);
  }
  ProbeReport rep;
  // the opt-in per-CU phases, in the order they are enqueued, finished and reported
  Check<lds::Plan, LdsResult> ld{o.lds, o.lds.on(), o.lds_first, &rep.has_lds, &rep.lds};
  Check<regs::Plan, RegsResult> rg{o.regs, o.regs.on, o.regs_first, &rep.has_regs, &rep.regs};
  Check<alu::Plan, AluResult> al{o.alu, o.alu.on, o.alu_first, &rep.has_alu, &rep.alu};
  Check<atom::Plan, AtomResult> at{o.atom, o.atom.on, o.atom_first, &rep.has_atom, &rep.atom};
  auto each_check = [&](auto&& f) {
    f(ld);
    f(rg);
    f(al);
    f(at);
  };
  each_check([&](auto& c) {
    if (c.pending) ensure(ctx, c.plan);
  });
  PhaseTimes& t = rep.phases;
  t.hbm_first = o.hbm_first;
  t.setup_ms = ms_since(t0);

  // one arena for the whole probe (arena.h)
  auto t_alloc = std::chrono::steady_clock::now();
  const uint64_t n16 = o.hbm_bytes / 16;
  const ArenaLayout lay = ArenaLayout::make(n16, o.gemm_n, o.mfma, o.lowp_mask);
  DevBuf transient;
  char* base = acquire_arena(ctx, lay.need, o.keep_arena, &transient, &t.arena_reused);
  auto* cnt = reinterpret_cast<unsigned long long*>(base + lay.cnt);
  t.alloc_ms = ms_since(t_alloc);

  // enqueue: the HBM test on s, the MFMA phase and the low-precision phase behind it on s2, in
  // "hbmFirst" order; the host link after both, so it overlaps both. The LDS phase ("ldsCheck")
  // never gets a stream of its own: ahead of the MFMA phase on s2, where it overlaps the first HBM
  // fill ("ldsFirst":0 behind it and the low-precision phase), or serial, last on the one stream.
  // The register-file phase ("regCheck", "regsFirst") takes the same places, behind the LDS phase,
  // and the vector-ALU phase ("aluCheck", "aluFirst") behind the register-file phase, the
  // atomic-unit phase ("atomCheck", "atomFirst") behind the vector-ALU phase
  auto t_run = std::chrono::steady_clock::now();
  reset_counters(ctx, o, cnt, s, s2);
  const lowp::Phase lp = lowp_phase(ctx, o, base, lay);
  // ``ahead``: only the phases that go ahead of the MFMA phase; else every one still pending
  auto enqueue_checks = [&](bool ahead) {
    each_check([&](auto& c) {
      if (!c.pending || (ahead && !c.first)) return;
      launch(ctx, s2, c.plan);
      c.pending = false;
    });
  };
  auto enqueue_mfma = [&](int when) {
    if (!o.mfma || o.hbm_first != when) return;
    if (o.overlap) enqueue_checks(true);
    launch_mfma_phase(base, lay, o, ctx, s2);
    lowp::launch(s2, lp);
    if (o.overlap) enqueue_checks(false);
  };
  const PatternPass pass = hbm_pass(ctx, o, dev, base, lay, n16);
  enqueue_mfma(0);
  enqueue_hbm(ctx, pass, o, cnt, [&] { enqueue_mfma(2); });
  enqueue_mfma(1);
  enqueue_checks(false);  // serial, or no MFMA phase to follow
  if (hl.n16) hostlink::launch(ctx, hl_s, hl);
  t.launch_ms = ms_since(t_run);  // host time to enqueue the whole probe

  // one sync per phase, then its fold
  PROBE_CHECK(hipStreamSynchronize(s));
  t.hbm_wall_ms = ms_since(t_run);
  rep.mfma.enabled = o.mfma;
  rep.mfma.n = o.gemm_n;
  rep.mfma.tile = o.gemm.variant.tile;
  rep.mfma.pipe = o.gemm.variant.tile == 256 ? o.gemm.variant.pipe : 0;
  if (o.mfma) {
    PROBE_CHECK(hipStreamSynchronize(s2));
    finish_mfma(o, ctx, &rep.mfma, &rep.cus);
  }
  if (!o.mfma && s2 != s && (ld.on || rg.on || al.on || at.on)) PROBE_CHECK(hipStreamSynchronize(s2));
  each_check([&](auto& c) {
    *c.has = c.on;
    if (c.on) *c.out = finish(ctx, c.plan, o.require_all_cus);
  });
  rep.lowp = lowp::finish(lp, o.require_all_cus);
  t.mfma_wall_ms = o.mfma ? ms_since(t_run) : 0.0;
  rep.has_host_link = hl.n16 != 0;
  if (hl.n16) {
    if (hl_s != s && !(hl_s == ctx.stream2 && o.mfma)) PROBE_CHECK(hipStreamSynchronize(hl_s));
    rep.host_link = hostlink::finish(ctx, hl);
  }
  rep.hbm = fold_passes(ctx.ev, ctx.host_res, o.patterns, n16);
  auto t_free = std::chrono::steady_clock::now();
  if (transient.p) {
    (void)hipFree(transient.p);
    transient.p = nullptr;
  }
  t.free_ms = ms_since(t_free);
  rep.total_ms = ms_since(t0);

  const auto t_report = std::chrono::steady_clock::now();
  rep.dev = dev;
  rep.uuid = ctx.uuid;
  rep.arch = ctx.prop.gcnArchName;
  std::string out = probe_report_open(rep);
  // host time spent building this report after the clock above stopped (timing of the binding)
  out += ",\"reportMs\":" + jnum(ms_since(t_report)) + "}";
  return out;
}

// What every entry point that returns a report shares: the body's report, or, if it throws, the
// sticky HIP error cleared and an error report with the entry point's head.
template <class F>
char* guarded(const std::string& head, F&& body) {
  try {
    return dup(body());
  } catch (const std::exception& e) {
    (void)hipGetLastError();
    return dup(error_report(head, e.what()));
  }
}

// ...and the status-code entry points: 0, or -4 if the body throws.
template <class F>
int guarded_status(F&& body) {
  try {
    body();
    return 0;
  } catch (const std::exception&) {
    (void)hipGetLastError();
    return -4;
  }
}

char* bad_device() { return dup(error_report("", "bad device index")); }

// Copies host operands in, runs ``launch`` on the null stream, copies C out. Throws on any failure.
struct HostOperand {
  const void* host;
  size_t bytes;
};
template <class F>
void gemm_on_host_buffers(int dev, std::vector<HostOperand> in, void* C, size_t c_bytes, bool poison_c, F&& launch) {
  PROBE_CHECK(hipSetDevice(dev));
  std::vector<DevBuf> d(in.size() + 1);
  for (size_t i = 0; i < in.size(); ++i) {
    if (!in[i].host) continue;
    PROBE_CHECK(hipMalloc(&d[i].p, in[i].bytes));
    PROBE_CHECK(hipMemcpy(d[i].p, in[i].host, in[i].bytes, hipMemcpyHostToDevice));
  }
  DevBuf& dc = d.back();
  PROBE_CHECK(hipMalloc(&dc.p, c_bytes));
  // test hook: a tile the kernel never writes comes back as all-ones words (NaN)
  if (poison_c) PROBE_CHECK(hipMemset(dc.p, 0xFF, c_bytes));
  launch(d);
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipMemcpy(C, dc.p, c_bytes, hipMemcpyDeviceToHost));
}

// ------------------------------------------------------------------ the checkers on host buffers (test surfaces)
constexpr int kBf16 = -1;           // the dtype argument of these entry points: bf16, else a lowp::Dtype
constexpr int kMaxCheckDim = 65535;  // m, n, k: the reference's grid has one row of blocks per m

// The contract of mi355x_probe_abft_check and mi355x_probe_gemm_ref.
bool checker_args_ok(int dtype, const void* A, const void* Bt, const void* sA, const void* sB, int m, int n, int k) {
  if (!A || !Bt || m < 1 || n < 1 || k < 1 || m > kMaxCheckDim || n > kMaxCheckDim || k > kMaxCheckDim || n % 4) return false;
  if (dtype == kBf16) return k % 8 == 0 && !sA && !sB;
  if (dtype < 0 || dtype >= lowp::kDtypes || k % 32) return false;
  return lowp::scaled(dtype) ? (sA && sB) : (!sA && !sB);
}

size_t operand_row_bytes(int dtype, int k) {
  return dtype == kBf16 ? static_cast<size_t>(k) * 2 : static_cast<size_t>(k) * lowp::bits_of(dtype) / 8;
}

// A device copy of ``bytes`` of host memory; a null host pointer leaves the buffer null.
void upload(DevBuf& d, const void* host, size_t bytes) {
  if (!host) return;
  PROBE_CHECK(hipMalloc(&d.p, bytes));
  PROBE_CHECK(hipMemcpy(d.p, host, bytes, hipMemcpyHostToDevice));
}

// The production checker sequence of ``dtype`` (mfma_phase.h's enqueue_abft, lowp::enqueue_abft).
void enqueue_checkers(hipStream_t s, int dtype, const void* a, const void* bt, const void* sa, const void* sb, const float* c,
                      int m, int n, int k, float bound, const AbftVectors& v, const AbftCounters& cnt) {
  auto u8 = [](const void* p) { return static_cast<const uint8_t*>(p); };
  if (dtype == kBf16)
    enqueue_abft(s, static_cast<const short*>(a), static_cast<const short*>(bt), c, m, n, k, bound, v, cnt);
  else if (dtype == lowp::kFp8)
    lowp::enqueue_abft<lowp::Fp8>(s, u8(a), u8(bt), u8(sa), u8(sb), c, m, n, k, bound, v, cnt);
  else if (dtype == lowp::kMxFp8)
    lowp::enqueue_abft<lowp::MxFp8>(s, u8(a), u8(bt), u8(sa), u8(sb), c, m, n, k, bound, v, cnt);
  else
    lowp::enqueue_abft<lowp::MxFp4>(s, u8(a), u8(bt), u8(sa), u8(sb), c, m, n, k, bound, v, cnt);
}

void launch_reference(hipStream_t s, int dtype, const void* a, const void* bt, const void* sa, const void* sb, float* r, int m,
                      int n, int k) {
  auto u8 = [](const void* p) { return static_cast<const uint8_t*>(p); };
  if (dtype == kBf16) launch_gemm_ref(s, static_cast<const short*>(a), static_cast<const short*>(bt), r, m, n, k);
  else if (dtype == lowp::kFp8) lowp::launch_gemm_ref<lowp::Fp8>(s, u8(a), u8(bt), u8(sa), u8(sb), r, m, n, k);
  else if (dtype == lowp::kMxFp8) lowp::launch_gemm_ref<lowp::MxFp8>(s, u8(a), u8(bt), u8(sa), u8(sb), r, m, n, k);
  else lowp::launch_gemm_ref<lowp::MxFp4>(s, u8(a), u8(bt), u8(sa), u8(sb), r, m, n, k);
}

// The production operand generator of ``dtype`` with its production grid.
void launch_generator(hipStream_t s, int dtype, void* out, uint64_t count, uint8_t* scales, uint32_t seed, int arg,
                      uint32_t* zero, uint64_t nzero) {
  const dim3 grid(2048), block(256);
  auto* words = static_cast<uint32_t*>(out);
  if (dtype == kBf16)
    hipLaunchKernelGGL(gen_operand, grid, block, 0, s, static_cast<short*>(out), count, seed, arg, zero, nzero);
  else if (dtype == lowp::kFp8)
    hipLaunchKernelGGL(lowp::gen_operand<lowp::Fp8>, grid, block, 0, s, words, count / 4, scales, count / 32, seed, arg);
  else if (dtype == lowp::kMxFp8)
    hipLaunchKernelGGL(lowp::gen_operand<lowp::MxFp8>, grid, block, 0, s, words, count / 4, scales, count / 32, seed, arg);
  else
    hipLaunchKernelGGL(lowp::gen_operand<lowp::MxFp4>, grid, block, 0, s, words, count / 8, scales, count / 32, seed, arg);
}

// A per-CU phase alone, on the HBM stream: what mi355x_probe_lds / _regs / _alu / _atomics share.
// ``block``: the phase's report block; ``dump_of``: where a dump run left its device copy, and how
// much of it the caller's buffer receives.
struct Dump {
  const void* dev;
  size_t bytes;
};
template <class Plan, class Block, class DumpOf>
char* run_check(int dev, const char* opts_json, void* buf, size_t buf_bytes, Block&& block, DumpOf&& dump_of) {
  if (!device_ok(dev)) return bad_device();
  ProbeActive active;
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded(device_head(dev), [&] {
    Plan pl = Plan::parse(opts_json, dev);  // lds: throws on a size outside [16, 163840]
    if (!buf || !buf_bytes) pl.dump_stage = 0;
    DeviceCtx& ctx = ensure_ctx(dev);
    ensure(ctx, pl);
    launch(ctx, ctx.stream, pl);
    PROBE_CHECK(hipStreamSynchronize(ctx.stream));
    const auto r = finish(ctx, pl, opt_bool(opts_json, "requireAllCUs", true));
    if (pl.dump_stage) {
      const Dump d = dump_of(ctx, pl);
      PROBE_CHECK(hipMemcpy(buf, d.dev, std::min(buf_bytes, d.bytes), hipMemcpyDeviceToHost));
    }
    // the block is the whole report, with the usual head
    return "{" + device_head(dev) + ",\"passed\":" + jbool(r.ok()) + "," + block(r).substr(1);
  });
}

}  // namespace

extern "C" {

int mi355x_probe_init(char* err, size_t errlen) {
  std::lock_guard<std::mutex> g(g_mu);
  if (g_count >= 0) return g_count;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    if (err && errlen) std::snprintf(err, errlen, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return -1;
  }
  g_ctx.resize(static_cast<size_t>(n));
  // Warm every context now so a claim-time probe pays no runtime/context initialisation: a real
  // probe, which also loads the code object and pays the first-launch costs.
  g_count = n;
  for (int d = 0; d < n; ++d) {
    if (hipSetDevice(d) != hipSuccess) continue;
    (void)hipFree(nullptr);
    try {
      (void)run_probe(d, "{\"hbmBytes\":1048576,\"patterns\":1,\"gemmN\":256,\"gemmReps\":1,\"keepArena\":0}");
    } catch (const std::exception&) {
      // a broken device fails its real probe later with the actual error
    }
  }
  return n;
}

int mi355x_probe_device_count(void) { return g_count; }

char* mi355x_probe_identify(int dev) {
  if (!device_ok(dev)) return dup("{\"error\":\"bad device\"}");
  hipDeviceProp_t prop{};
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return dup("{\"error\":\"hipGetDeviceProperties failed\"}");
  char bdf[32];
  std::snprintf(bdf, sizeof bdf, "%04x:%02x:%02x.0", prop.pciDomainID, prop.pciBusID, prop.pciDeviceID);
  std::string out = "{" + device_head(dev) + ",\"hipUUID\":" + jstr(hip_uuid(dev)) +
                    ",\"name\":" + jstr(prop.name) + ",\"gcnArch\":" + jstr(prop.gcnArchName) +
                    ",\"bdf\":" + jstr(bdf) + ",\"totalMem\":" + std::to_string(prop.totalGlobalMem) +
                    ",\"computeUnits\":" + std::to_string(prop.multiProcessorCount) + "}";
  return dup(out);
}

char* mi355x_probe_run(int dev, const char* opts_json) {
  if (!device_ok(dev)) return bad_device();
  ProbeActive active;  // the sweep buffer's chunk (un)mapping waits while this runs
  // Per-device serialisation: concurrent probes of DIFFERENT devices run in parallel.
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded(device_head(dev), [&] { return run_probe(dev, opts_json); });
}

char* mi355x_probe_peer_dump(int src, int dst, const char* opts_json, void* io, size_t io_bytes) {
  if (!device_ok(src) || !device_ok(dst)) return bad_device();
  // both devices' probe locks, in index order (no deadlock against a concurrent pair)
  std::lock_guard<std::mutex> a(device_mutex(std::min(src, dst)));
  std::unique_lock<std::mutex> b;
  if (src != dst) b = std::unique_lock<std::mutex>(device_mutex(std::max(src, dst)));
  return guarded(link_head(src, dst), [&] { return run_peer(src, dst, opts_json, io, io_bytes); });
}

char* mi355x_probe_peer(int src, int dst, const char* opts_json) {
  return mi355x_probe_peer_dump(src, dst, opts_json, nullptr, 0);
}

char* mi355x_probe_peer_ring(const int* devs, int n, const char* opts_json) {
  if (g_count < 0 || !devs || n < 2 || n > 64) return dup(error_report("", "bad ring"));
  std::vector<int> ring(devs, devs + n);
  for (int d : ring)
    if (d < 0 || d >= g_count) return bad_device();
  // every distinct device's probe lock, in index order (no deadlock against probes or pairs)
  std::vector<std::unique_lock<std::mutex>> locks;
  for (int d : distinct(ring)) locks.emplace_back(device_mutex(d));
  return guarded("", [&] { return run_peer_ring(ring, opts_json); });
}

// Frees the probe arenas idle for at least ``idle_ms`` (0: all, unconditionally); returns how many
// were freed. With idle_ms > 0 an arena stays while its device holds an HBM sweep buffer or freed one
// less than kSweepClearGrace ago. The host-link phase's pinned buffer stays: trim hands VRAM back to
// a tenant, and that is a few MiB of host RAM.
int mi355x_probe_trim(int idle_ms) {
  if (g_count <= 0) return 0;
  int freed = 0;
  const auto now = std::chrono::steady_clock::now();
  for (int d = 0; d < g_count; ++d) {
    std::lock_guard<std::mutex> g(device_mutex(d));
    DeviceCtx& ctx = ctx_of(d);
    const auto idle = std::chrono::milliseconds(idle_ms);
    bool arena = ctx.arena && now - ctx.arena_used >= idle;
    if (idle_ms > 0 && (!ctx.sweep.empty() || now - ctx.sweep_released < kSweepClearGrace)) arena = false;  // 0 = forced
    const bool peer = ctx.peer_bytes && now - ctx.peer_used >= idle;  // the xGMI ring windows
    if (!arena && !peer) continue;
    if (hipSetDevice(d) != hipSuccess) continue;
    if (peer) free_peer_bufs(ctx);
    if (!arena) continue;
    (void)hipFree(ctx.arena);
    ctx.arena = nullptr;
    ctx.arena_bytes = 0;
    ++freed;
  }
  return freed;
}

char* mi355x_probe_hbm_sweep(int dev, const char* opts_json) {
  if (!device_ok(dev)) return bad_device();
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded(device_head(dev), [&] { return run_sweep(dev, opts_json); });
}

int mi355x_probe_sweep_alloc(int dev, long long reserve) {
  if (!device_ok(dev)) return -1;
  {
    std::lock_guard<std::mutex> g(device_mutex(dev));
    if (!ctx_of(dev).sweep.empty()) return 0;
  }
  SweepBuf b;
  try {
    if (hipSetDevice(dev) != hipSuccess) return -1;
    b = sweep_alloc_raw(static_cast<uint64_t>(std::max(0LL, reserve)), dev);
  } catch (const std::exception&) {
    (void)hipGetLastError();
    return -2;
  }
  std::lock_guard<std::mutex> g(device_mutex(dev));
  DeviceCtx& ctx = ctx_of(dev);
  if (!ctx.sweep.empty()) {  // lost a race with another allocator: keep theirs
    sweep_free(b);
    return 0;
  }
  ctx.sweep = std::move(b);
  return 1;
}

int mi355x_probe_sweep_release(int dev) {
  if (!device_ok(dev)) return -1;
  SweepBuf b;
  {
    std::lock_guard<std::mutex> g(device_mutex(dev));
    DeviceCtx& ctx = ctx_of(dev);
    b = std::move(ctx.sweep);
    ctx.sweep = SweepBuf{};
    ctx.sweep_released = std::chrono::steady_clock::now();
  }
  if (b.empty()) return 0;
  if (hipSetDevice(dev) != hipSuccess) return -1;
  sweep_free(b, dev);  // outside the device lock, chunk by chunk, between probes
  return 1;
}

int mi355x_probe_gemm_bf16_opts(int dev, const void* A, const void* Bt, void* C, int m, int n, int k,
                                const char* opts_json) {
  if (!device_ok(dev)) return -1;
  const GemmOptions o = GemmOptions::parse(opts_json);
  if (!A || !Bt || !C || !gemm_args_ok(o.variant, m, n, k)) return -2;
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded_status([&] {
    const size_t sa = static_cast<size_t>(m) * k * 2, sb = static_cast<size_t>(n) * k * 2;
    gemm_on_host_buffers(dev, {{A, sa}, {Bt, sb}}, C, static_cast<size_t>(m) * n * 4, o.poison_c, [&](std::vector<DevBuf>& d) {
      launch_gemm(nullptr, o.variant, static_cast<const short*>(d[0].p), static_cast<const short*>(d[1].p),
                  static_cast<float*>(d[2].p), m, n, k, nullptr, o.group_m);
    });
  });
}

int mi355x_probe_gemm_lowp(int dev, int dtype, const void* A, const void* Bt, const void* scaleA, const void* scaleBt,
                           void* C, int m, int n, int k, const char* opts_json) {
  if (!device_ok(dev)) return -1;
  if (!A || !Bt || !C || !lowp::gemm_args_ok(dtype, m, n, k)) return -2;
  if (lowp::scaled(dtype) ? (!scaleA || !scaleBt) : (scaleA || scaleBt)) return -2;
  const bool poison_c = opt_bool(opts_json, "poisonC", false);
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded_status([&] {
    const size_t kb = static_cast<size_t>(k) * lowp::bits_of(dtype) / 8, ks = static_cast<size_t>(k) / 32;
    // unscaled: no scale buffers (null device pointers)
    gemm_on_host_buffers(dev, {{A, m * kb}, {Bt, n * kb}, {scaleA, m * ks}, {scaleBt, n * ks}}, C,
                         static_cast<size_t>(m) * n * 4, poison_c, [&](std::vector<DevBuf>& d) {
                           lowp::launch_gemm(nullptr, dtype, static_cast<const uint8_t*>(d[0].p),
                                             static_cast<const uint8_t*>(d[1].p), static_cast<const uint8_t*>(d[2].p),
                                             static_cast<const uint8_t*>(d[3].p), static_cast<float*>(d[4].p), m, n, k);
                         });
  });
}

int mi355x_probe_abft_check(int dev, int dtype, const void* A, const void* Bt, const void* scaleA, const void* scaleBt,
                            const void* C, int m, int n, int k, float bound, unsigned int* vectors,
                            unsigned long long* counts, int nfaults, const long long* fault_index, const float* fault_value,
                            unsigned long long* fault_counts) {
  if (!device_ok(dev)) return -1;
  if (!C || !vectors || !counts || !checker_args_ok(dtype, A, Bt, scaleA, scaleBt, m, n, k)) return -2;
  if (nfaults < 0 || (nfaults > 0 && (!fault_index || !fault_value || !fault_counts))) return -2;
  const long long elems = static_cast<long long>(m) * n;
  for (int i = 0; i < nfaults; ++i)
    if (fault_index[i] < 0 || fault_index[i] >= elems) return -2;
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded_status([&] {
    PROBE_CHECK(hipSetDevice(dev));
    const size_t kb = operand_row_bytes(dtype, k), ks = static_cast<size_t>(k) / 32;
    DevBuf da, db, dsa, dsb, dc, dv, dcnt;
    upload(da, A, m * kb);
    upload(db, Bt, n * kb);
    upload(dsa, scaleA, m * ks);
    upload(dsb, scaleBt, n * ks);
    upload(dc, C, static_cast<size_t>(elems) * 4);
    // the six vectors, each from a 32-byte boundary; the three that accumulate come first
    auto pad8 = [](size_t words) { return (words + 7) & ~static_cast<size_t>(7); };
    const size_t pk = pad8(k), pn = pad8(n), pm = pad8(m), vwords = 2 * pk + 2 * pn + 2 * pm;
    PROBE_CHECK(hipMalloc(&dv.p, vwords * 4));
    auto* v32 = static_cast<uint32_t*>(dv.p);
    const AbftVectors v{v32, v32 + pk, v32 + 2 * pk, v32 + 2 * pk + pn, v32 + 2 * pk + 2 * pn, v32 + 2 * pk + 2 * pn + pm};
    const size_t runs = static_cast<size_t>(nfaults) + 1;
    PROBE_CHECK(hipMalloc(&dcnt.p, runs * 3 * sizeof(unsigned long long)));
    PROBE_CHECK(hipMemset(dcnt.p, 0, runs * 3 * sizeof(unsigned long long)));
    auto* cnt = static_cast<unsigned long long*>(dcnt.p);
    auto* c = static_cast<float*>(dc.p);
    auto check = [&](size_t run) {
      PROBE_CHECK(hipMemsetAsync(v32, 0, (2 * pk + pn) * 4, nullptr));
      enqueue_checkers(nullptr, dtype, da.p, db.p, dsa.p, dsb.p, c, m, n, k, bound, v,
                       AbftCounters{cnt + 3 * run, cnt + 3 * run + 1, cnt + 3 * run + 2});
      PROBE_CHECK(hipGetLastError());
    };
    check(0);
    std::vector<uint32_t> hv(vwords);
    PROBE_CHECK(hipMemcpy(hv.data(), v32, vwords * 4, hipMemcpyDeviceToHost));
    // one fault at a time: the element set, the sequence run, the element put back
    const float* hc = static_cast<const float*>(C);
    for (int i = 0; i < nfaults; ++i) {
      hipLaunchKernelGGL(poke_f32, dim3(1), dim3(1), 0, nullptr, c, static_cast<int64_t>(fault_index[i]), fault_value[i]);
      check(static_cast<size_t>(i) + 1);
      hipLaunchKernelGGL(poke_f32, dim3(1), dim3(1), 0, nullptr, c, static_cast<int64_t>(fault_index[i]), hc[fault_index[i]]);
    }
    std::vector<unsigned long long> hcnt(runs * 3);
    PROBE_CHECK(hipMemcpy(hcnt.data(), cnt, hcnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    // packed for the caller: K, K, N, N, M, M words
    const size_t from[6] = {0, pk, 2 * pk, 2 * pk + pn, 2 * pk + 2 * pn, 2 * pk + 2 * pn + pm};
    const size_t len[6] = {static_cast<size_t>(k), static_cast<size_t>(k), static_cast<size_t>(n),
                           static_cast<size_t>(n), static_cast<size_t>(m), static_cast<size_t>(m)};
    unsigned int* out = vectors;
    for (int i = 0; i < 6; ++i) {
      std::memcpy(out, hv.data() + from[i], len[i] * 4);
      out += len[i];
    }
    std::memcpy(counts, hcnt.data(), 3 * sizeof(unsigned long long));
    if (nfaults) std::memcpy(fault_counts, hcnt.data() + 3, static_cast<size_t>(nfaults) * 3 * sizeof(unsigned long long));
  });
}

int mi355x_probe_gemm_ref(int dev, int dtype, const void* A, const void* Bt, const void* scaleA, const void* scaleBt,
                          void* R, int m, int n, int k) {
  if (!device_ok(dev)) return -1;
  if (!R || !checker_args_ok(dtype, A, Bt, scaleA, scaleBt, m, n, k)) return -2;
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded_status([&] {
    const size_t kb = operand_row_bytes(dtype, k), ks = static_cast<size_t>(k) / 32;
    // the device R starts as 0xFF bytes: an element the reference never writes comes back as NaN
    gemm_on_host_buffers(dev, {{A, m * kb}, {Bt, n * kb}, {scaleA, m * ks}, {scaleBt, n * ks}}, R,
                         static_cast<size_t>(m) * n * 4, true, [&](std::vector<DevBuf>& d) {
                           launch_reference(nullptr, dtype, d[0].p, d[1].p, d[2].p, d[3].p, static_cast<float*>(d[4].p), m, n, k);
                         });
  });
}

int mi355x_probe_count_diff(int dev, const float* x, const float* y, unsigned long long count, unsigned long long* bad) {
  if (!device_ok(dev)) return -1;
  if (!x || !y || !bad || count < 1 || count > (1ull << 31)) return -2;
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded_status([&] {
    PROBE_CHECK(hipSetDevice(dev));
    DevBuf dx, dy, dbad;
    upload(dx, x, count * 4);
    upload(dy, y, count * 4);
    PROBE_CHECK(hipMalloc(&dbad.p, sizeof(unsigned long long)));
    PROBE_CHECK(hipMemset(dbad.p, 0, sizeof(unsigned long long)));
    launch_count_diff(nullptr, static_cast<const float*>(dx.p), static_cast<const float*>(dy.p), count,
                      static_cast<unsigned long long*>(dbad.p));
    PROBE_CHECK(hipGetLastError());
    unsigned long long h = 0;
    PROBE_CHECK(hipMemcpy(&h, dbad.p, sizeof h, hipMemcpyDeviceToHost));
    *bad = h;
  });
}

int mi355x_probe_gen_operands(int dev, int dtype, unsigned int seed, int span_or_scale_lo, unsigned long long count,
                              unsigned long long nzero, void* operand, size_t operand_bytes, void* scales,
                              size_t scale_bytes, void* zero, size_t zero_bytes) {
  if (!device_ok(dev)) return -1;
  if (!operand || count < 1 || count > (1ull << 31) || nzero > (1ull << 28)) return -2;
  if (dtype != kBf16 && (dtype < 0 || dtype >= lowp::kDtypes)) return -2;
  const bool bf16 = dtype == kBf16, has_scales = !bf16 && lowp::scaled(dtype);
  size_t need = 0;
  if (bf16) {
    if (span_or_scale_lo < 1 || span_or_scale_lo > 127) return -2;  // exact in bf16
    need = count * 2;
  } else {
    // whole 32-bit words of elements, no zero region, scales that stay E8M0 powers of two
    if (count % (32 / lowp::bits_of(dtype)) || nzero || zero || span_or_scale_lo < -126 || span_or_scale_lo > 126) return -2;
    need = count * lowp::bits_of(dtype) / 8;
  }
  if (operand_bytes < need || (has_scales ? (!scales || scale_bytes < count / 32) : scales != nullptr)) return -2;
  if (zero ? zero_bytes < nzero * 4 : nzero > 0) return -2;
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded_status([&] {
    PROBE_CHECK(hipSetDevice(dev));
    DevBuf dop, dsc, dz;
    auto filled = [](DevBuf& d, size_t bytes) {  // at least one byte, so an empty region is still a buffer
      PROBE_CHECK(hipMalloc(&d.p, std::max<size_t>(bytes, 16)));
      PROBE_CHECK(hipMemset(d.p, 0xFF, std::max<size_t>(bytes, 16)));
    };
    filled(dop, operand_bytes);
    if (has_scales) filled(dsc, scale_bytes);
    if (zero) filled(dz, zero_bytes);
    launch_generator(nullptr, dtype, dop.p, count, static_cast<uint8_t*>(dsc.p), seed, span_or_scale_lo,
                     static_cast<uint32_t*>(dz.p), nzero);
    PROBE_CHECK(hipGetLastError());
    PROBE_CHECK(hipMemcpy(operand, dop.p, operand_bytes, hipMemcpyDeviceToHost));
    if (has_scales && scale_bytes) PROBE_CHECK(hipMemcpy(scales, dsc.p, scale_bytes, hipMemcpyDeviceToHost));
    if (zero && zero_bytes) PROBE_CHECK(hipMemcpy(zero, dz.p, zero_bytes, hipMemcpyDeviceToHost));
  });
}

void mi355x_probe_host_link_geometry(int* grid, int* threads, int* unroll) {
  if (grid) *grid = hostlink::kGrid;
  if (threads) *threads = hostlink::kThreads;
  if (unroll) *unroll = hostlink::kUnroll;
}

char* mi355x_probe_host_link(int dev, const char* opts_json, void* io, size_t io_bytes) {
  if (!device_ok(dev)) return bad_device();
  const HostLinkOptions o = HostLinkOptions::parse(opts_json);
  if (o.preload && !io) return dup(error_report("", "preload needs a caller buffer"));
  ProbeActive active;
  std::lock_guard<std::mutex> g(device_mutex(dev));
  return guarded(device_head(dev), [&] {
    DeviceCtx& ctx = ensure_ctx(dev);
    const uint64_t bytes = o.preload ? static_cast<uint64_t>(io_bytes) : o.bytes;
    if (bytes < 16 || bytes > hostlink::kMaxBytes) throw ProbeError("host-link size outside [16 B, 4 GiB]");
    hostlink::Plan pl = hostlink::Plan::parse(opts_json, dev, bytes);
    if (o.preload) {
      pl.preload = true;
      pl.patterns = 1;
    }
    pl.alloc_ms = hostlink::ensure(ctx, pl.n16 * 16, pl.coherent);
    if (o.preload) std::memcpy(ctx.hl_buf, io, pl.n16 * 16);
    hostlink::launch(ctx, ctx.stream, pl);
    PROBE_CHECK(hipStreamSynchronize(ctx.stream));
    const HostLinkResult r = hostlink::finish(ctx, pl);
    if (io) std::memcpy(io, ctx.hl_buf, std::min<uint64_t>(io_bytes, pl.n16 * 16));
    // the block is the whole report, with the usual head
    return "{" + device_head(dev) + ",\"passed\":" + jbool(r.ok()) + "," + host_link_block(r).substr(1);
  });
}

int mi355x_probe_gemm_bf16(int dev, const void* A, const void* Bt, void* C, int m, int n, int k) {
  return mi355x_probe_gemm_bf16_opts(dev, A, Bt, C, m, n, k, nullptr);
}

char* mi355x_probe_lds(int dev, const char* opts_json, void* image, size_t image_bytes) {
  return run_check<lds::Plan>(dev, opts_json, image, image_bytes, lds_block, [](DeviceCtx& ctx, const lds::Plan& pl) {
    return Dump{ctx.lds.dump, static_cast<size_t>(pl.n16) * 16};
  });
}

char* mi355x_probe_regs(int dev, const char* opts_json, void* image, size_t image_bytes) {
  return run_check<regs::Plan>(dev, opts_json, image, image_bytes, regs_block, [](DeviceCtx& ctx, const regs::Plan&) {
    return Dump{ctx.regs.dump, regs::kImageBytes};
  });
}

char* mi355x_probe_alu(int dev, const char* opts_json, void* dump, size_t dump_bytes) {
  return run_check<alu::Plan>(dev, opts_json, dump, dump_bytes, alu_block, [](DeviceCtx& ctx, const alu::Plan& pl) {
    return Dump{pl.dump_stage == 3 ? ctx.alu.trace : ctx.alu.dump, pl.dump_bytes()};
  });
}

char* mi355x_probe_atomics(int dev, const char* opts_json, void* dump, size_t dump_bytes) {
  return run_check<atom::Plan>(dev, opts_json, dump, dump_bytes, atom_block, [](DeviceCtx& ctx, const atom::Plan&) {
    return Dump{ctx.atom.dump, atom::kDumpBytes};
  });
}

void mi355x_probe_free(char* p) { std::free(p); }

}  // extern "C"
