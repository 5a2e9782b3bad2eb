// The options of the probe's entry points, read once and up front: every key with its default and
// its clamping, as plain structs. Pure host code (no HIP include), shared by probe.hip and the host
// unit test (native/tests/test_probe_options.cc). The defaults that a measurement chose live here
// with that measurement, next to the option that overrides them for an in-process A/B.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

namespace {

// First occurrence of the quoted key; `true` / `false`, spaces after the colon, else strtoll.
inline long long opt_int(const char* json, const char* key, long long def) {
  if (!json) return def;
  std::string pat = std::string("\"") + key + "\"";
  const char* p = std::strstr(json, pat.c_str());
  if (!p) return def;
  p = std::strchr(p + pat.size(), ':');
  if (!p) return def;
  ++p;
  while (*p == ' ') ++p;
  if (std::strncmp(p, "true", 4) == 0) return 1;
  if (std::strncmp(p, "false", 5) == 0) return 0;
  return std::strtoll(p, nullptr, 10);
}

inline bool opt_bool(const char* json, const char* key, bool def) { return opt_int(json, key, def) != 0; }

// "key":[a, b, ...]: the first ``n`` integers of the array into ``out``; true when all n were there.
inline bool opt_ints(const char* json, const char* key, long long* out, int n) {
  if (!json) return false;
  std::string pat = std::string("\"") + key + "\"";
  const char* p = std::strstr(json, pat.c_str());
  if (!p) return false;
  p = std::strchr(p + pat.size(), ':');
  if (!p) return false;
  ++p;
  while (*p == ' ') ++p;
  if (*p != '[') return false;
  ++p;
  for (int i = 0; i < n; ++i) {
    char* end = nullptr;
    out[i] = std::strtoll(p, &end, 10);
    if (end == p) return false;
    p = end;
    while (*p == ' ') ++p;
    if (i + 1 < n) {
      if (*p != ',') return false;
      ++p;
    }
  }
  return true;
}

// An integer option clamped to [lo, hi].
inline int opt_clamped(const char* json, const char* key, long long lo, long long hi, long long def) {
  return static_cast<int>(std::min(hi, std::max(lo, opt_int(json, key, def))));
}

// An index option: the value when in [0, n), else -1 (a test hook that is off).
inline int opt_index(const char* json, const char* key, long long n) {
  const long long v = opt_int(json, key, -1);
  return v >= 0 && v < n ? static_cast<int>(v) : -1;
}

// A dump stage: 1..max, anything else 0 (no dump).
inline int opt_stage(const char* json, const char* key, long long max) {
  const long long v = opt_int(json, key, 0);
  return v >= 1 && v <= max ? static_cast<int>(v) : 0;
}

// A salt option: whether the caller gave one (>= 0), and its value.
inline void opt_salt(const char* json, const char* key, bool* given, uint32_t* salt) {
  const long long v = opt_int(json, key, -1);
  *given = v >= 0;
  *salt = *given ? static_cast<uint32_t>(v) : 0u;
}

constexpr long long kMaxPatterns = 4;
constexpr long long kMaxInjectFlips = 4096;  // "injectBitFlips" of the probe, the peer checks and the sweep

// Default pattern (probe option "hbmPattern" selects per run, for in-process A/B). Measured on
// MI355X, 9 interleaved rounds (profiles/r3h_probe_pattern_ab.json): 1 GiB test 6.16 -> 6.41 TB/s
// (write 5.77 -> 6.06, read 6.64 -> 6.76), claim-time probe (beside the MFMA phase) 0.98 -> 0.91 ms.
constexpr int kHbmPattern = 1;
// Grid-stride (0) measured faster than tiled (1) for the fill (6.03 vs 5.51 TB/s) and within 4 % for
// the verify: claim-time probe 0.757 vs 0.772 ms (profiles/r4h_probe_hbm_layout_ab_rejected.json).
constexpr int kHbmLayout = 0;
// Grid per HBM kernel, workgroups per CU. Measured on MI355X (scripts/probe_hbm_sweep.py): the
// streaming store kernel is fastest with few long-running waves per CU, the verify kernel with a
// few more loads in flight; the old 8/CU for both was among the slowest settings.
constexpr long long kHbmFillBlocksPerCU = 1, kHbmVerifyBlocksPerCU = 3;

// Tile order of gemm_bf16_mfma_256: 0 row-major, > 1 grouped. Groups of 4 tile rows: 8192^3 1331 vs
// 1118 TFLOP/s (+19 %), 4096^3 unchanged (1366 vs 1372) (profiles/r4q_probe_gemm_group_ab.json).
constexpr int kGemmGroupM = 4;
// K-loop of the 256x256 GEMM ("gemmPipe" selects per probe): 0 the 2-phase loop, 1 the half-tile
// pipeline, 2 the half-tile pipeline with staggered wave groups and a static s_setprio(1) for waves
// 4-7 (default: 4096^3 1411 vs 1276 TFLOP/s for 0, 8192^3 1459 vs 1339, profiles/r6v_gemm_prio_ab.json),
// 21 the same with s_setprio flips around every MFMA cluster instead (1358 / 1430; r6q, r6s), 22 with
// no s_setprio, 3 the 32x32x16 fragment-ring variant (measured slower, r6t: A/B only). Also measured
// and dropped: the phase reads as inline-asm ds_read_b128 in k-sub order with counted lgkmcnt, so a
// quadrant's first MFMAs start on half its fragments (4096^3 1354 vs 1411, 8192^3 1420 vs 1456,
// profiles/r6za_gemm_counted_reads_ab_rejected.json), and tile-row groups of 2/8/16 instead of 4
// (r6z_gemm_group_ab.json).
constexpr int kGemmPipe = 2;

// Which GEMM kernel runs: the options "gemmTile", "gemmPipe", "gemmPrio", "gemmVecC".
struct GemmVariant {
  int tile = 256;        // 128: the older 128x128 register-staged kernel
  int pipe = kGemmPipe;  // K-loop of the 256x256 kernel (see kGemmPipe)
  bool prio = false;     // 2-phase loop only
  bool vec_c = false;    // 2-phase loop only
};

// The GEMM options a probe and mi355x_probe_gemm_bf16_opts share. ``tile`` is what was asked for:
// the host-buffer entry point refuses a tile that is neither 256 nor 128, a probe runs 256 then.
struct GemmOptions {
  GemmVariant variant;
  int group_m = kGemmGroupM;  // tile order (A/B)
  bool poison_c = false;      // test hook
  static GemmOptions parse(const char* json) {
    GemmOptions o;
    o.variant.tile = static_cast<int>(opt_int(json, "gemmTile", 256));
    o.variant.pipe = static_cast<int>(opt_int(json, "gemmPipe", kGemmPipe));
    o.variant.prio = opt_bool(json, "gemmPrio", false);
    o.variant.vec_c = opt_bool(json, "gemmVecC", false);
    o.group_m = static_cast<int>(opt_int(json, "gemmGroupM", kGemmGroupM));
    o.poison_c = opt_bool(json, "poisonC", false);
    return o;
  }
};

namespace lowp {
// "mfmaLowPrecision" is a mask: bit d set asks for dtype d.
enum Dtype { kFp8 = 0, kMxFp8 = 1, kMxFp4 = 2, kDtypes = 3 };
constexpr const char* kNames[kDtypes] = {"fp8", "mxfp8", "mxfp4"};
}  // namespace lowp

namespace hostlink {

// Grid, unroll, temporal / non-temporal access and coherent (fine-grained) / default pinned memory:
// the probe options "hostLinkGrid", "hostLinkUnroll" (4 | 8 | 16), "hostLinkNT", "hostLinkCoherent"
// select per run for the sweep of scripts/hostlink_rates.py. Measured on the MI355X at 64 MiB, alone
// on the GPU, p50 GB/s write / read (profiles/hostlink_rates.json; PCIe Gen5 x16, 63 GB/s spec):
//   * grid: the read needs 16 workgroups to fill the link — 2: 14.0, 4: 28.0, 8: 50.0, 16: 57.2,
//     32: 55.3, 64..256: 56.2-57.1 (unroll 8); the write is at 53-56 from 2 workgroups on. 16
//     workgroups are all the phase takes from the HBM and MFMA phases beside it.
//   * unroll 4 / 8 / 16 at grid 16: 55.7 / 56.1 / 56.2 write, 57.3 / 57.2 / 57.1 read: flat. 8 keeps
//     128 B per lane in flight; at grid 8 only unroll 4 still reads at 57.2 (8: 50.0, 16: 48.5).
//   * temporal stores write 56.1 vs 55.0 non-temporal (56.2 vs 53.8 in an earlier run of the same
//     sweep); loads are the same either way (57.18 vs 57.20). The opposite of the HBM kernels'
//     choice: the data leaves the device whatever the hint says.
//   * coherent (fine-grained) vs default pinned memory: 56.13 / 57.18 vs 56.07 / 57.17, no
//     difference, and no configuration exceeded the link's rate (nothing is served from a cache).
//     Coherent is kept: the host's sample and the flip hook then need no cache maintenance.
// By size at these defaults: 1 MiB 45.2 / 44.3, 4 MiB 51.0 / 53.5, 16 MiB 53.1 / 56.3, 64 MiB
// 56.1 / 57.2, 256 MiB 56.8 / 57.4; run-to-run spread under 0.2 GB/s from 8 MiB up.
constexpr int kGrid = 16;
constexpr int kUnroll = 8;
constexpr bool kNonTemporal = false;
constexpr bool kCoherent = true;
constexpr int kMaxGrid = 1024;
constexpr uint64_t kMaxBytes = 4ull << 30;

// What one run of the phase does (options of mi355x_probe_run / mi355x_probe_host_link).
struct Plan {
  uint64_t n16 = 0;  // 0: the phase is off
  int patterns = 2;
  uint32_t seed = 0;
  long long inject_chunk = -1;  // test hook "injectHostLinkFlipAtChunk"
  bool preload = false;         // no write pass: verify what the caller loaded, polarity 0
  int grid = kGrid, unroll = kUnroll;
  bool nt = kNonTemporal, coherent = kCoherent;
  double alloc_ms = 0;
  // ``bytes``: "hostLinkBytes", or the caller's buffer for a preload.
  static Plan parse(const char* json, int dev, uint64_t bytes) {
    Plan pl;
    pl.n16 = bytes / 16;
    pl.patterns = opt_clamped(json, "hostLinkPatterns", 1, kMaxPatterns, 2);
    pl.seed = 0x4C4B0000u + static_cast<uint32_t>(dev);
    pl.inject_chunk = opt_int(json, "injectHostLinkFlipAtChunk", -1);
    pl.grid = opt_clamped(json, "hostLinkGrid", 1, kMaxGrid, kGrid);
    pl.unroll = static_cast<int>(opt_int(json, "hostLinkUnroll", kUnroll));
    pl.nt = opt_bool(json, "hostLinkNT", kNonTemporal);
    pl.coherent = opt_bool(json, "hostLinkCoherent", kCoherent);
    return pl;
  }
};

}  // namespace hostlink

namespace lds {

// The LDS of one gfx950 CU, which one workgroup of the phase's kernel declares in full.
constexpr uint32_t kBytesPerCU = 163840;
// Workgroups per CU of the grid ("ldsBlocksPerCU" selects per run): the oversubscription that makes
// the dispatcher visit every CU, like the census's 8. Measured on the MI355X, 200 runs per factor
// (scripts/lds_claim_probe_cost.py, profiles/lds_claim_probe_cost.json): alone on the GPU every
// factor from 1 up tested all 256 CUs in every run; inside the overlapped claim probe 1 and 2 each
// had a run that reached 212 / 218 CUs, 4, 8 and 16 none. The kernel's time is linear in the factor
// (alone 0.048 ms per workgroup per CU), so the default is the smallest factor that never fell short.
constexpr int kBlocksPerCU = 4;
constexpr int kMaxBlocksPerCU = 64;
// Where the phase sits on the MFMA stream ("ldsFirst" selects per run): 0 behind the MFMA and
// low-precision phases, 1 ahead of them. Same measurement, 40 alternating rounds: ahead of the MFMA
// phase the kernel overlaps the HBM test's first fill, which needs no LDS, and the claim probe grows
// by a quarter of what the tail position adds.
constexpr int kFirst = 1;

// The address pass writes dword ((t + 256 i) * S) mod N: S is the smallest odd value >= 33 that is
// coprime to N, so d -> d * S mod N is a bijection of the N tested dwords and neighbouring threads
// land 33+ dwords apart. A wrong S leaves dwords unwritten, which the pass then reports.
inline uint32_t stride_for(uint32_t dwords) {
  auto gcd = [](uint32_t a, uint32_t b) {
    while (b) {
      const uint32_t r = a % b;
      a = b;
      b = r;
    }
    return a;
  };
  uint32_t s = 33;
  while (gcd(s, dwords) != 1) s += 2;
  return s;
}

// What one run of the phase does (options of mi355x_probe_run with "ldsCheck" and of mi355x_probe_lds).
struct Plan {
  uint32_t n16 = 0;  // tested 16-byte chunks per workgroup; 0: the phase is off
  int patterns = 2;
  bool salt_given = false;  // else the phase takes the context's run counter
  uint32_t salt = 0;        // "ldsSalt", XORed into the seed
  uint32_t seed = 0;        // 0x4C445300 + dev, before the salt
  int blocks_per_cu = kBlocksPerCU;
  long long flip_byte = -1;   // test hook "injectLdsFlipAtByte"
  int fault_xcc = -1;         // test hook "injectLdsFaultXcc": the flip only on that XCD
  long long skip_chunk = -1;  // test hook "injectLdsSkipChunk"
  int dump_stage = 0;         // "ldsDumpStage" 1 | 2 | 3, only with a caller buffer
  bool on() const { return n16 != 0; }
  uint32_t stride() const { return stride_for(n16 * 4); }
  // "ldsBytes": 16 .. kBytesPerCU, rounded down to whole chunks; anything else throws.
  static Plan parse(const char* json, int dev) {
    Plan pl;
    const long long bytes = opt_int(json, "ldsBytes", kBytesPerCU);
    if (bytes < 16 || bytes > static_cast<long long>(kBytesPerCU))
      throw std::invalid_argument("ldsBytes outside [16, 163840]");
    pl.n16 = static_cast<uint32_t>(bytes / 16);
    pl.patterns = opt_clamped(json, "ldsPatterns", 1, kMaxPatterns, 2);
    opt_salt(json, "ldsSalt", &pl.salt_given, &pl.salt);
    pl.seed = 0x4C445300u + static_cast<uint32_t>(dev);
    pl.blocks_per_cu = opt_clamped(json, "ldsBlocksPerCU", 1, kMaxBlocksPerCU, kBlocksPerCU);
    pl.flip_byte = opt_int(json, "injectLdsFlipAtByte", -1);
    pl.fault_xcc = static_cast<int>(opt_int(json, "injectLdsFaultXcc", -1));
    pl.skip_chunk = opt_int(json, "injectLdsSkipChunk", -1);
    pl.dump_stage = opt_stage(json, "ldsDumpStage", 3);
    return pl;
  }
};

}  // namespace lds

namespace regs {

// The vector register file of one gfx950 SIMD: v0..v255 and a0..a255 of every lane, numbered 0..511.
constexpr int kRegistersPerLane = 512;
constexpr int kLanes = 64;
constexpr int kSimdsPerCU = 4;
// One workgroup's registers as mi355x_probe_regs copies them out: uint32 [wave][register][lane].
constexpr size_t kImageBytes = static_cast<size_t>(kSimdsPerCU) * kRegistersPerLane * kLanes * 4;
// Workgroups per CU of the grid ("regsBlocksPerCU" selects per run): the oversubscription that makes
// the dispatcher visit every CU, like the LDS phase's. A workgroup of this kernel needs a CU empty of
// every other wave, so beside the HBM test it waits for that test's waves to drain. Measured on the
// MI355X, two sweeps of 200 runs per factor (scripts/regs_claim_probe_cost.py,
// profiles/regs_claim_probe_cost.json, regs_claim_probe_cost_run1.json): alone on the GPU every factor
// from 1 up tested all 256 CUs on four SIMDs each in every run (kernel p50 0.043 ms at factor 1, 0.077 at 2,
// linear above: 0.036 ms per workgroup per CU); inside the overlapped claim probe behind the MFMA phase factor 1
// had one run of 400 that reached 251 CUs, 2, 4, 8 and 16 none; ahead of the MFMA phase no factor fell
// short. The default is the smallest factor that never fell short at the default position.
constexpr int kBlocksPerCU = 2;
constexpr int kMaxBlocksPerCU = 64;
// Where the phase sits on the MFMA stream ("regsFirst" selects per run): 0 behind the MFMA and
// low-precision phases, 1 ahead of them. Same measurement, 40 alternating rounds at factor 2: behind
// the MFMA phase the claim probe grows 0.764 -> 0.824 ms (+0.060; +0.126 at factor 4 in the run
// before), ahead of it -> 0.880 ms (+0.115): ahead, the kernel's workgroups wait for CUs the first HBM
// fill occupies (kernel 0.31 ms beside the probe against 0.16 behind, 0.077 alone), so unlike the LDS
// phase this one is cheaper at the tail. Ahead wins only from factor 8 up (1.004 vs 1.031 ms).
constexpr int kFirst = 0;

// What one run of the phase does (options of mi355x_probe_run with "regCheck" and of mi355x_probe_regs).
struct Plan {
  bool on = false;  // false: the phase is off
  int patterns = 2;
  bool salt_given = false;  // else the phase takes the context's run counter
  uint32_t salt = 0;        // "regsSalt", XORed into the seed
  uint32_t seed = 0;        // 0x52454700 + dev, before the salt
  int blocks_per_cu = kBlocksPerCU;
  // test hooks, each off (-1) when out of range
  int flip_u = -1, flip_lane = -1, flip_bit = -1;  // "injectRegFlip":[u, lane, bit]
  int fault_simd = -1;                             // "injectRegFaultSimd": the flip only on that SIMD
  int fault_xcc = -1;                              // "injectRegFaultXcc": the flip only on that XCD
  int skip_u = -1;                                 // "injectRegSkip"
  int dump_stage = 0;                              // "regsDumpStage" 1 | 2, only with a caller buffer
  // the test instantiation of the kernel runs only when a hook or the dump asks for it
  bool test_kernel() const { return flip_u >= 0 || skip_u >= 0 || dump_stage != 0; }
  static Plan parse(const char* json, int dev) {
    Plan pl;
    pl.on = true;
    pl.patterns = opt_clamped(json, "regsPatterns", 1, kMaxPatterns, 2);
    opt_salt(json, "regsSalt", &pl.salt_given, &pl.salt);
    pl.seed = 0x52454700u + static_cast<uint32_t>(dev);
    pl.blocks_per_cu = opt_clamped(json, "regsBlocksPerCU", 1, kMaxBlocksPerCU, kBlocksPerCU);
    long long f[3];
    if (opt_ints(json, "injectRegFlip", f, 3) && f[0] >= 0 && f[0] < kRegistersPerLane && f[1] >= 0 && f[1] < kLanes &&
        f[2] >= 0 && f[2] < 32) {
      pl.flip_u = static_cast<int>(f[0]);
      pl.flip_lane = static_cast<int>(f[1]);
      pl.flip_bit = static_cast<int>(f[2]);
    }
    pl.fault_simd = opt_index(json, "injectRegFaultSimd", kSimdsPerCU);
    pl.fault_xcc = opt_index(json, "injectRegFaultXcc", 8);
    pl.skip_u = opt_index(json, "injectRegSkip", kRegistersPerLane);
    pl.dump_stage = opt_stage(json, "regsDumpStage", 2);
    return pl;
  }
};

}  // namespace regs

namespace alu {

constexpr int kPlanGroups = 6;  // int, f32, f64, f16, lane, trans (alu_ref.h kGroups)
constexpr int kPlanLanes = 64;
constexpr int kSimdsPerCU = 4;
// workgroup 0's digests as mi355x_probe_alu copies them out: uint32 [wave][group][lane]
constexpr size_t kDumpBytes = static_cast<size_t>(kSimdsPerCU) * kPlanGroups * kPlanLanes * 4;
// workgroup 0's trace of the trans group (dump stage 3): uint32 [wave][step][word][lane], the first
// kTraceSteps steps; word 0 is the digest as the step began, words 1..11 the step's results as folded
constexpr int kTraceSteps = 64, kTraceWords = 12;
constexpr size_t kTraceBytes = static_cast<size_t>(kSimdsPerCU) * kTraceSteps * kTraceWords * kPlanLanes * 4;
// Steps per group ("aluIters" selects per run): the largest power of two at which the phase adds no
// more to the claim probe's p50 (1 GiB, 2048^3, overlapped) than the register check's recorded +0.060 ms.
// Measured on the MI355X at 1 workgroup per CU, each step count alternating with the plain probe for
// 40 rounds (scripts/alu_claim_probe_cost.py, profiles/alu_claim_probe_cost.json and _run1.json), added
// p50 in two runs: 1..32 steps +0.025..0.036 ms (the launch, the atomics and the expectation load, not
// the steps), 64 +0.032 / +0.039, 128 +0.061 / +0.055, 256 +0.136, 512 +0.30, 1024 +0.82. 128 sits on
// the limit and crossed it in one of the two runs, so the default is 64. The kernel alone takes
// 0.027 ms at 1 step and 1.33 us per step above ~16 (0.105 ms at 64, 1.39 ms at 1024).
constexpr int kIters = 64;
constexpr int kMaxIters = 4096;  // the step has 20 bits in an operand's index; the twin is exact rational
// Workgroups per CU of the grid ("aluBlocksPerCU" selects per run). The kernel makes no exclusivity
// claim (28 VGPRs, no LDS), so coverage is per (CU, SIMD) and rests on the dispatcher. Same
// measurement, 400 runs per factor and setting, the factors interleaved: 1, 2, 4, 8 and 16 all verified
// 4 x 256 SIMDs in every run, alone on the GPU and inside the overlapped claim probe at either
// position. Unlike the LDS and
// register kernels this one needs nothing of a CU to itself, so its workgroups land beside the HBM
// test's waves. The default is the smallest factor, 1: kernel p50 alone 0.106 ms at 64 steps against
// 0.165 / 0.293 / 0.552 / 1.07 at 2 / 4 / 8 / 16 (waves of one SIMD run one after the other), claim
// probe 0.80 ms against 0.87 / 0.99 / 1.25 / 1.76 behind the MFMA phase. Coverage stays part of ok.
constexpr int kBlocksPerCU = 1;
constexpr int kMaxBlocksPerCU = 64;
// Where the phase sits on the MFMA stream ("aluFirst" selects per run): 0 behind the MFMA and
// low-precision phases, 1 ahead of them. Same measurement, 40 alternating rounds at 1 workgroup per CU
// and 64 steps: the claim probe grows 0.765 -> 0.800 ms behind the MFMA phase (+0.034) and -> 0.804
// ahead of it (+0.038); at 32 steps the run before had it the other way round (+0.031 behind, +0.028
// ahead). The two places differ by less than the plain probe's odd/even-round spread
// (0.007 ms): the default is the one that added less at the default step count, behind.
constexpr int kFirst = 0;
constexpr uint32_t kPlanSeedBase = 0x414C5500u;  // alu_ref.h kSeedBase

// What one run of the phase does (options of mi355x_probe_run with "aluCheck" and of mi355x_probe_alu).
struct Plan {
  bool on = false;  // false: the phase is off
  int iters = kIters;
  int blocks_per_cu = kBlocksPerCU;
  // "aluSeed", else kPlanSeedBase + dev: fixed per device and never salted per run, because the
  // host's expectation table is computed once per (seed, iters) and cached in the context
  uint32_t seed = 0;
  // test hooks, each off (-1) when out of range
  int flip_group = -1, flip_step = -1, flip_lane = -1, flip_bit = -1;  // "injectAluFlip":[group, step, lane, bit]
  int fault_simd = -1;                                                 // "injectAluFaultSimd": the flip only on that SIMD
  int fault_xcc = -1;                                                  // "injectAluFaultXcc": the flip only on that XCD
  int dump_stage = 0;                                                  // "aluDumpStage" 1 | 2 | 3, only with a caller buffer
  // the test instantiation of the kernel runs only when a hook or the dump asks for it
  bool test_kernel() const { return flip_group >= 0 || dump_stage != 0; }
  static Plan parse(const char* json, int dev) {
    Plan pl;
    pl.on = true;
    pl.iters = opt_clamped(json, "aluIters", 1, kMaxIters, kIters);
    pl.blocks_per_cu = opt_clamped(json, "aluBlocksPerCU", 1, kMaxBlocksPerCU, kBlocksPerCU);
    const long long seed = opt_int(json, "aluSeed", -1);
    pl.seed = seed >= 0 ? static_cast<uint32_t>(seed) : kPlanSeedBase + static_cast<uint32_t>(dev);
    long long f[4];
    if (opt_ints(json, "injectAluFlip", f, 4) && f[0] >= 0 && f[0] < kPlanGroups && f[1] >= 0 && f[1] < pl.iters &&
        f[2] >= 0 && f[2] < kPlanLanes && f[3] >= 0 && f[3] < 32) {
      pl.flip_group = static_cast<int>(f[0]);
      pl.flip_step = static_cast<int>(f[1]);
      pl.flip_lane = static_cast<int>(f[2]);
      pl.flip_bit = static_cast<int>(f[3]);
    }
    pl.fault_simd = opt_index(json, "injectAluFaultSimd", kSimdsPerCU);
    pl.fault_xcc = opt_index(json, "injectAluFaultXcc", 8);
    pl.dump_stage = opt_stage(json, "aluDumpStage", 3);
    return pl;
  }
  // what the caller's buffer receives: the digests (stages 1 and 2) or the trans trace (stage 3)
  size_t dump_bytes() const { return dump_stage == 3 ? kTraceBytes : dump_stage ? kDumpBytes : 0; }
};

}  // namespace alu

namespace atom {

constexpr int kPlanLayers = 3;   // lds, l2, dev (atomics_ref.h kLayers)
constexpr int kPlanOps = 22;     // contended 0..16, returning 17..21 (atomics_ref.h kAllOps)
constexpr int kPlanTicket = 22;  // the LDS ticket test as a skip hook's op (atomics_ref.h kTicket)
constexpr int kPlanWideFirst = 12, kPlanWideEnd = 17;  // the 8-byte ops: a flip's bit runs to 63
constexpr int kPlanLanes = 64;
constexpr size_t kPlanDumpWords = 24064;  // atomics_ref.h kDumpWords
constexpr size_t kDumpBytes = kPlanDumpWords * 4;
// Steps per layer ("atomIters" selects per run, 1..kMaxIters). The rule that chose aluIters: the largest
// count at which the phase adds no more to the claim probe's p50 (1 GiB, 2048^3, overlapped) than the
// register check's recorded +0.060 ms, in two runs. Measured on the MI355X at 1 workgroup per CU, each
// step count alternating with the plain probe for 40 rounds (scripts/atomics_claim_probe_cost.py,
// profiles/atomics_claim_probe_cost.json and _run2.json), added p50 in the two runs: 1 step +0.020 /
// +0.019 ms, 2 +0.037 / +0.037, 4 +0.095 / +0.093, 8 +0.228 / +0.231, 16 +0.50, 32 +1.06, 64 +2.17. 2 is
// the largest count within the budget in both runs. The two kernels alone take 0.068 ms at 1 step and
// 0.034 ms per further step (2.24 ms at 64): the dev layer's rows are hit by every workgroup, which is what
// the steps cost. From 2 steps on the returning ops see values other than the initial ones.
constexpr int kIters = 2;
constexpr int kMaxIters = 64;  // bounds the floating-point rows' sums (atomics_ref.h kMaxSumF32)
// Workgroups per CU of the grid ("atomBlocksPerCU" selects per run, 1..kMaxBlocksPerCU). The kernel owns
// nothing (74 VGPRs, 16 KiB of LDS), so coverage is per CU and rests on the dispatcher. Same
// measurement, 400 runs per factor and setting in each of the two runs, the factors interleaved, at 1 step:
// 1, 2, 4, 8 and 16 all verified 256 CUs in every run, alone on the GPU and inside the overlapped claim
// probe at either position. The default is the smallest factor, 1: kernels' p50 alone 0.069 ms against
// 0.118 / 0.218 / 0.423 / 0.830 at 2 / 4 / 8 / 16, claim probe 0.797 ms against 0.826 / 0.921 / 1.129 /
// 1.534 behind the MFMA phase. Coverage stays part of ok.
constexpr int kBlocksPerCU = 1;
constexpr int kMaxBlocksPerCU = 16;
constexpr int kLayerMask = 7;  // "atomLayers": bit 0 lds, 1 l2, 2 dev
// Where the phase sits on the MFMA stream ("atomFirst" selects per run): 0 behind the MFMA and
// low-precision phases and every other opt-in phase, 1 ahead of the MFMA phase. Same measurement, 40
// alternating rounds at 1 step, in the two runs: behind +0.022 / +0.018 ms, ahead +0.017 / +0.023: the two
// places change order between the runs and differ by less than a run does from the next, so the default
// stays where the ALU phase measured cheaper, behind. Not measured at the default of 2 steps.
constexpr int kFirst = 0;
constexpr uint32_t kPlanSeedBase = 0x41544D00u;  // atomics_ref.h kSeedBase

// What one run of the phase does (options of mi355x_probe_run with "atomCheck" and of mi355x_probe_atomics).
struct Plan {
  bool on = false;  // false: the phase is off
  int iters = kIters;
  int blocks_per_cu = kBlocksPerCU;
  int layers = kLayerMask;
  // "atomSeed", else kPlanSeedBase + dev: fixed per device and never salted per run, because the
  // host's expectation table is computed once per (seed, iters) and cached in the context
  uint32_t seed = 0;
  // test hooks, each off (-1) when out of range; both strike wave 0 of the struck workgroups
  int skip_layer = -1, skip_op = -1, skip_step = -1, skip_lane = -1;               // "injectAtomSkip":[layer, op, step, lane]
  int flip_layer = -1, flip_op = -1, flip_step = -1, flip_lane = -1, flip_bit = 0;  // "injectAtomFlip":[layer, op, step, lane, bit]
  int fault_xcc = -1;  // "injectAtomFaultXcc": the hooks only on that XCD
  int fault_wg = -1;   // "injectAtomFaultWorkgroup": the hooks only in that workgroup
  int dump_stage = 0;  // "atomDumpStage" 1 | 2, only with a caller buffer
  bool time_kernels = false;  // "atomTimeKernels": an event between the two kernels (mi355x_probe_atomics only)
  // the test instantiation of the kernel runs only when a hook or the dump asks for it
  bool test_kernel() const { return skip_layer >= 0 || flip_layer >= 0 || dump_stage != 0; }
  static Plan parse(const char* json, int dev) {
    Plan pl;
    pl.on = true;
    pl.iters = opt_clamped(json, "atomIters", 1, kMaxIters, kIters);
    pl.blocks_per_cu = opt_clamped(json, "atomBlocksPerCU", 1, kMaxBlocksPerCU, kBlocksPerCU);
    const long long layers = opt_int(json, "atomLayers", kLayerMask);
    pl.layers = layers >= 1 && layers <= kLayerMask ? static_cast<int>(layers) : kLayerMask;
    const long long seed = opt_int(json, "atomSeed", -1);
    pl.seed = seed >= 0 ? static_cast<uint32_t>(seed) : kPlanSeedBase + static_cast<uint32_t>(dev);
    pl.time_kernels = opt_bool(json, "atomTimeKernels", false);
    pl.dump_stage = opt_stage(json, "atomDumpStage", 2);
    // which (layer, op) pairs exist: the returning ops and the ticket test not in the dev layer
    // layer 3 in a hook: the lds layer's second addressing (slot = lane & 15), contended ops only
    auto known = [](long long layer, long long op, bool ticket_ok) {
      if (layer < 0 || layer > kPlanLayers || op < 0) return false;
      if (op == kPlanTicket) return ticket_ok && layer == 0;
      return op < (layer >= 2 ? kPlanWideEnd : kPlanOps);
    };
    long long f[5];
    if (opt_ints(json, "injectAtomSkip", f, 4) && known(f[0], f[1], true) && f[2] >= 0 && f[2] < pl.iters && f[3] >= 0 &&
        f[3] < kPlanLanes) {
      pl.skip_layer = static_cast<int>(f[0]);
      pl.skip_op = static_cast<int>(f[1]);
      pl.skip_step = static_cast<int>(f[2]);
      pl.skip_lane = static_cast<int>(f[3]);
    }
    if (opt_ints(json, "injectAtomFlip", f, 5) && known(f[0], f[1], false) && f[2] >= 0 && f[2] < pl.iters && f[3] >= 0 &&
        f[3] < kPlanLanes && f[4] >= 0 && f[4] < (f[1] >= kPlanWideFirst && f[1] < kPlanWideEnd ? 64 : 32)) {
      pl.flip_layer = static_cast<int>(f[0]);
      pl.flip_op = static_cast<int>(f[1]);
      pl.flip_step = static_cast<int>(f[2]);
      pl.flip_lane = static_cast<int>(f[3]);
      pl.flip_bit = static_cast<int>(f[4]);
    }
    pl.fault_xcc = opt_index(json, "injectAtomFaultXcc", 8);
    pl.fault_wg = opt_index(json, "injectAtomFaultWorkgroup", kMaxBlocksPerCU * 256);
    return pl;
  }
};

}  // namespace atom

// Where the GEMM fault hooks corrupt C (test hooks "injectGemmFaultRow" / "injectGemmFaultCol"):
// -1 is the element the hooks always took, row n/3 and column n/5; any other value outside [0, n)
// means no fault, like "injectFlipAtChunk".
struct FaultAt {
  long long row = -1, col = -1;
  // the element's index in an n x n C, or -1: no fault
  long long index(int n) const {
    const long long r = row == -1 ? n / 3 : row, c = col == -1 ? n / 5 : col;
    if (r < 0 || r >= n || c < 0 || c >= n) return -1;
    return r * n + c;
  }
};

// Every option of mi355x_probe_run.
struct ProbeOptions {
  uint64_t hbm_bytes = 1ull << 30;
  int patterns = 2;               // 1..kMaxPatterns
  bool cheap_pattern = true;      // "hbmPattern" == 1
  bool tiled = false;             // "hbmLayout" == 1, cheap pattern only
  long long fill_blocks_per_cu = kHbmFillBlocksPerCU;  // "hbmFillBlocksPerCU", else "hbmBlocksPerCU"
  long long verify_blocks_per_cu = kHbmVerifyBlocksPerCU;
  int inject_flips = 0;           // test hook, 0..4096
  long long inject_chunk = -1;    // test hook: one flip, bit 0 of a chunk
  bool mfma = true;
  int gemm_n = 4096;              // a multiple of 256, at least 256
  GemmOptions gemm;               // variant.tile is 256 or 128 here
  int reps = 1;                   // 0 with "gemmSkip" (test hook, with poisonC): C keeps the poison
  int inject_gemm = 0;            // test hook
  FaultAt inject_gemm_at;         // test hook: where injectGemmFault and injectLowpFault strike
  int census_fault_xcc = -1;      // test hook
  bool require_all_cus = true;
  bool cu_keys = false;
  int lowp_mask = 0;              // bit d: also check lowp::Dtype d; needs the MFMA phase
  int inject_lowp = 0;            // test hook: dtype mask
  int lowp_census_fault_xcc = -1;
  // The HBM test is bandwidth-bound with few waves per CU; the MFMA phase is compute-bound and
  // touches ~130 MiB: run them concurrently on two streams (overlap=0: one stream, serial).
  bool overlap = true;
  // Launch order: the HBM test is the probe's critical path (~0.68 ms of kernels for 1 GiB x 2
  // patterns); the MFMA phase (~0.1 ms of GPU time beside it) costs ~20 API calls to enqueue. With
  // hbmFirst 1 the HBM kernels are enqueued first, so the fill starts ~20 launches earlier and the
  // MFMA phase is enqueued while it runs (profiles/r4e_probe_launch_order_ab.json). 0: the MFMA
  // phase first. 2: right after the first fill (in-process A/B), so it starts earlier on the GPU
  // while the rest of the HBM test is still enqueued well ahead of need.
  int hbm_first = 1;
  // The first fill resets the HBM counter pairs and the MFMA phase's first kernel its own slots, so
  // neither stream starts behind memsets or waits on the other — after an idle gap each API call
  // ahead of the first fill costs tens of us (profiles/r4i_probe_idle_gap_ab.json). 0: memsets on
  // the HBM stream, the MFMA stream waits for them (the older path).
  bool zero_in_kernel = true;
  bool keep_arena = true;
  hostlink::Plan host_link;        // n16 == 0: off, and none of its options is looked up
  bool host_link_on_mfma_stream = false;  // "hostLinkStream":1, for the A/B; only with overlap
  lds::Plan lds;                   // "ldsCheck"; n16 == 0: off, and none of its options is looked up
  bool lds_first = lds::kFirst == 1;  // "ldsFirst": 1 ahead of the MFMA phase on its stream, 0 behind it (A/B)
  regs::Plan regs;                 // "regCheck"; !on: off, and none of its options is looked up
  bool regs_first = regs::kFirst == 1;  // "regsFirst": as "ldsFirst"
  alu::Plan alu;                   // "aluCheck"; !on: off, and none of its options is looked up
  bool alu_first = alu::kFirst == 1;  // "aluFirst": as "ldsFirst"
  atom::Plan atom;                 // "atomCheck"; !on: off, and none of its options is looked up
  bool atom_first = atom::kFirst == 1;  // "atomFirst": as "ldsFirst"

  // An opt-in per-CU phase: off, and none of its options looked up, unless ``check_key`` is set.
  // ``first`` comes in as the phase's measured default.
  template <class Plan>
  static void check(const char* json, int dev, const char* check_key, const char* first_key, Plan* plan, bool* first) {
    if (!opt_bool(json, check_key, false)) return;
    *plan = Plan::parse(json, dev);
    plan->dump_stage = 0;  // the dump needs the caller buffer of the phase's own entry point
    *first = opt_int(json, first_key, *first) == 1;
  }

  static ProbeOptions parse(const char* json, int dev = 0) {
    ProbeOptions o;
    o.hbm_bytes = static_cast<uint64_t>(opt_int(json, "hbmBytes", 1LL << 30));
    o.patterns = opt_clamped(json, "patterns", 1, kMaxPatterns, 2);
    o.cheap_pattern = opt_int(json, "hbmPattern", kHbmPattern) == 1;
    o.tiled = o.cheap_pattern && opt_int(json, "hbmLayout", kHbmLayout) == 1;
    o.fill_blocks_per_cu =
        std::max(1LL, opt_int(json, "hbmFillBlocksPerCU", opt_int(json, "hbmBlocksPerCU", kHbmFillBlocksPerCU)));
    o.verify_blocks_per_cu =
        std::max(1LL, opt_int(json, "hbmVerifyBlocksPerCU", opt_int(json, "hbmBlocksPerCU", kHbmVerifyBlocksPerCU)));
    o.inject_flips = opt_clamped(json, "injectBitFlips", 0, kMaxInjectFlips, 0);
    o.inject_chunk = opt_int(json, "injectFlipAtChunk", -1);
    o.mfma = opt_bool(json, "mfma", true);
    o.gemm_n = std::max(256, (static_cast<int>(opt_int(json, "gemmN", 4096)) / 256) * 256);
    o.gemm = GemmOptions::parse(json);
    o.gemm.variant.tile = o.gemm.variant.tile != 128 ? 256 : 128;
    o.reps = opt_int(json, "gemmSkip", 0) ? 0 : static_cast<int>(std::max(1LL, opt_int(json, "gemmReps", 1)));
    o.inject_gemm = static_cast<int>(opt_int(json, "injectGemmFault", 0));
    o.inject_gemm_at.row = opt_int(json, "injectGemmFaultRow", -1);
    o.inject_gemm_at.col = opt_int(json, "injectGemmFaultCol", -1);
    o.census_fault_xcc = static_cast<int>(opt_int(json, "injectCensusFaultXcc", -1));
    o.require_all_cus = opt_bool(json, "requireAllCUs", true);
    o.cu_keys = opt_bool(json, "cuKeys", false);
    o.lowp_mask = o.mfma ? static_cast<int>(opt_int(json, "mfmaLowPrecision", 0)) & ((1 << lowp::kDtypes) - 1) : 0;
    o.inject_lowp = static_cast<int>(opt_int(json, "injectLowpFault", 0));
    o.lowp_census_fault_xcc = static_cast<int>(opt_int(json, "injectLowpCensusFaultXcc", -1));
    o.overlap = opt_bool(json, "overlap", true);
    o.hbm_first = static_cast<int>(opt_int(json, "hbmFirst", 1));
    o.zero_in_kernel = opt_bool(json, "zeroInKernel", true);
    o.keep_arena = opt_bool(json, "keepArena", true);
    const uint64_t hl_bytes = static_cast<uint64_t>(std::max(0LL, opt_int(json, "hostLinkBytes", 0)));
    if (hl_bytes > hostlink::kMaxBytes) throw std::invalid_argument("hostLinkBytes above 4 GiB");
    if (hl_bytes) {
      o.host_link = hostlink::Plan::parse(json, dev, hl_bytes);
      o.host_link_on_mfma_stream = o.overlap && opt_int(json, "hostLinkStream", 0) == 1;
    }
    check(json, dev, "ldsCheck", "ldsFirst", &o.lds, &o.lds_first);
    check(json, dev, "regCheck", "regsFirst", &o.regs, &o.regs_first);
    check(json, dev, "aluCheck", "aluFirst", &o.alu, &o.alu_first);
    check(json, dev, "atomCheck", "atomFirst", &o.atom, &o.atom_first);
    o.atom.time_kernels = false;  // the claim probe records no event between the kernels
    return o;
  }
};

// mi355x_probe_host_link: "preload" verifies the caller's buffer, one pass, polarity 0.
struct HostLinkOptions {
  bool preload = false;
  uint64_t bytes = 0;  // "hostLinkBytes" (ignored for a preload: the caller's buffer decides)
  static HostLinkOptions parse(const char* json) {
    HostLinkOptions o;
    o.preload = opt_bool(json, "preload", false);
    o.bytes = static_cast<uint64_t>(std::max(0LL, opt_int(json, "hostLinkBytes", 0)));
    return o;
  }
};

// "bytes" of mi355x_probe_peer (default 256 MiB) and mi355x_probe_peer_ring (64 MiB): at least 1 MiB.
inline uint64_t peer_bytes(const char* json, long long def) {
  return static_cast<uint64_t>(std::max(1LL << 20, opt_int(json, "bytes", def)));
}

// The seed one call of a peer check fills and verifies a link with: the link's fixed base seed mixed
// with a per-call nonce (peer.h takes it from a process-wide counter). The receive windows outlive a
// call (the ring keeps them, the pair check's fresh allocation usually lands on the last one's
// memory), and with a fixed seed they already hold exactly what the next call expects: a copy that
// delivered nothing would verify. The odd multiplier makes nonce -> seed a bijection for one base,
// and the XOR keeps the seeds of two bases apart within one call.
inline uint32_t peer_call_seed(uint32_t base, uint32_t nonce) { return base ^ (nonce * 0x9E3779B1u); }

// mi355x_probe_peer (default 256 MiB) and mi355x_probe_peer_ring (64 MiB): "bytes" and the test hooks.
struct PeerOptions {
  uint64_t bytes = 0;           // at least 1 MiB; the checks round it down to whole 16-byte chunks
  long long inject_chunk = -1;  // test hook "injectFlipAtChunk": bit 0 of that chunk of the receiving window
  int inject_flips = 0;         // test hook "injectBitFlips", 0..4096, spread over the receiving window
  int inject_link = 0;          // "injectLink": the ring link the two hooks strike (a pair check ignores it)
  bool skip_copy = false;       // test hook "skipCopy": no link's copy is enqueued, everything else runs
  static PeerOptions parse(const char* json, long long def_bytes) {
    PeerOptions o;
    o.bytes = peer_bytes(json, def_bytes);
    o.inject_chunk = opt_int(json, "injectFlipAtChunk", -1);
    o.inject_flips = opt_clamped(json, "injectBitFlips", 0, kMaxInjectFlips, 0);
    o.inject_link = opt_clamped(json, "injectLink", 0, 4096, 0);
    o.skip_copy = opt_bool(json, "skipCopy", false);
    return o;
  }
  // the chunk of an n16-chunk window to flip, or -1: none (out of range: no flip)
  long long flip_chunk(uint64_t n16) const {
    return inject_chunk >= 0 && static_cast<uint64_t>(inject_chunk) < n16 ? inject_chunk : -1;
  }
};

// mi355x_probe_hbm_sweep.
struct SweepOptions {
  uint64_t bytes = 16ull << 30;   // window, at least 1 MiB
  uint64_t reserve = 4ull << 30;  // free HBM left alone when the call has to allocate the buffer
  uint64_t offset = 0;
  bool keep = false;
  int inject_flips = 0;  // test hook, 0..4096, in the window's first piece
  long long inject_chunk = -1;  // test hook "injectFlipAtChunk": bit 0 of that 16-byte chunk of the window
  static SweepOptions parse(const char* json) {
    SweepOptions o;
    o.bytes = static_cast<uint64_t>(std::max(1LL << 20, opt_int(json, "bytes", 16LL << 30)));
    o.reserve = static_cast<uint64_t>(std::max(0LL, opt_int(json, "reserve", 4LL << 30)));
    o.offset = static_cast<uint64_t>(std::max(0LL, opt_int(json, "offset", 0)));
    o.keep = opt_bool(json, "keep", false);
    o.inject_flips = opt_clamped(json, "injectBitFlips", 0, kMaxInjectFlips, 0);
    o.inject_chunk = opt_int(json, "injectFlipAtChunk", -1);
    return o;
  }
};

}  // namespace
