// The text of every report the probe library returns: plain result structs in, JSON out. Key order
// and number formatting are part of the interface (the agent and the tests parse them). Pure host
// code (no HIP include): native/tests/test_probe_report.cc pins every block byte for byte.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace {

inline std::string jnum(double v) {
  char b[64];
  std::snprintf(b, sizeof b, "%.6g", v);
  return b;
}

inline std::string jstr(const std::string& s) {
  std::string o = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') o.push_back('\\');
    if (static_cast<unsigned char>(c) < 0x20) continue;
    o.push_back(c);
  }
  return o + "\"";
}

inline const char* jbool(bool b) { return b ? "true" : "false"; }

// first_bad: a 16-byte chunk index, all-ones = none -> byte offset ``base + 16 * first_bad`` or null
inline std::string joffset(unsigned long long first_bad, unsigned long long base = 0) {
  return first_bad == ~0ull ? std::string("null") : std::to_string(base + first_bad * 16);
}

// "[v0,v1,...]": the per-XCD and per-SIMD counts of the blocks below.
template <class T>
inline std::string jarray(const T* v, int n) {
  std::string out = "[";
  for (int i = 0; i < n; ++i) out += (i ? "," : "") + std::to_string(v[i]);
  return out + "]";
}

// A bit field of a per-CU phase's first_bad key, all-ones = none -> null.
inline std::string first_bad_field(unsigned long long first_bad, int shift, unsigned long long mask) {
  return first_bad == ~0ull ? std::string("null") : std::to_string((first_bad >> shift) & mask);
}

// The tail of a block whose run dumped workgroup 0: its CU key and the SIMD of each of its four waves.
inline std::string dump_tail(int dump_cu, const int* dump_simds) {
  if (dump_cu < 0) return "";
  return ",\"dumpCU\":" + std::to_string(dump_cu) + ",\"dumpSimds\":" + jarray(dump_simds, 4);
}

// A pattern test folded over its passes (hbm.h fold_passes): the HBM phase and the host link.
struct HbmResult {
  unsigned long long bad_bits = 0, first_bad = ~0ull;
  float write_ms = 0, read_ms = 0;
  uint64_t n16 = 0;
  int patterns = 0;
  bool ok() const { return bad_bits == 0; }
};

inline std::string hbm_block(const HbmResult& r) {
  const double bytes_moved = static_cast<double>(r.n16) * 16.0 * r.patterns;
  const double write_gbps = bytes_moved / (r.write_ms * 1e-3) / 1e9;
  const double read_gbps = bytes_moved / (r.read_ms * 1e-3) / 1e9;
  const double gbps = 2.0 * bytes_moved / ((r.write_ms + r.read_ms) * 1e-3) / 1e9;
  return "{\"ok\":" + std::string(jbool(r.ok())) + ",\"bytes\":" + std::to_string(r.n16 * 16) +
         ",\"patterns\":" + std::to_string(r.patterns) + ",\"badBits\":" + std::to_string(r.bad_bits) +
         ",\"firstBadOffset\":" + joffset(r.first_bad) + ",\"writeGBps\":" + jnum(write_gbps) +
         ",\"readGBps\":" + jnum(read_gbps) + ",\"GBps\":" + jnum(gbps) + ",\"ms\":" + jnum(r.write_ms + r.read_ms) + "}";
}

inline double gemm_tflops(int n, double ms) {
  return ms > 0 ? 2.0 * n * static_cast<double>(n) * n / (ms * 1e-3) / 1e12 : 0.0;
}

struct MfmaResult {
  bool ok = true, enabled = false;
  int n = 0, tile = 256, pipe = 0;
  unsigned long long small_bad = 0, abft_bad = 0;
  double tflops = 0, ms = 0;
};

inline std::string mfma_block(const MfmaResult& r) {
  return "{\"ok\":" + std::string(jbool(r.ok)) + ",\"enabled\":" + jbool(r.enabled) + ",\"n\":" + std::to_string(r.n) +
         ",\"tile\":" + std::to_string(r.tile) + ",\"pipe\":" + std::to_string(r.pipe) +
         ",\"elementMismatches\":" + std::to_string(r.small_bad) + ",\"abftMismatches\":" + std::to_string(r.abft_bad) +
         ",\"tflops\":" + jnum(r.tflops) + ",\"ms\":" + jnum(r.ms) + "}";
}

// Which CUs proved their matrix cores (census) and which ran GEMM tiles.
struct CusResult {
  int expected = 0, verified = 0;
  int per_xcd[8] = {};
  int gemm_tiles = 0;
  unsigned long long bad_waves = 0;
  bool want_keys = false;  // "cuKeys": the (xcc, se, sh, cu) key of every verified CU
  std::vector<int> keys;
};

inline std::string cus_block(const CusResult& r) {
  std::string out = "{\"expected\":" + std::to_string(r.expected) + ",\"mfmaVerified\":" + std::to_string(r.verified) +
                    ",\"perXcd\":" + jarray(r.per_xcd, 8) + ",\"gemmTiles\":" + std::to_string(r.gemm_tiles) +
                    ",\"badWaves\":" + std::to_string(r.bad_waves) + ",\"ok\":" +
                    jbool(r.bad_waves == 0 && r.verified >= r.expected);
  if (r.want_keys) {
    out += ",\"cuKeys\":[";
    for (size_t i = 0; i < r.keys.size(); ++i) out += (i ? "," : "") + std::to_string(r.keys[i]);
    out += "]";
  }
  return out + "}";
}

struct LowpResult {
  const char* name = "";
  bool ok = true;
  int n = 0;
  unsigned long long small_bad = 0, abft_bad = 0;
  float ms = 0;
  int verified = 0;
  unsigned long long bad_waves = 0;
};

// One entry per dtype that ran, in dtype order.
inline std::string lowp_block(const std::vector<LowpResult>& rs) {
  std::string out = "{";
  for (const LowpResult& r : rs)
    out += std::string(out.size() > 1 ? "," : "") + "\"" + r.name + "\":{\"ok\":" + jbool(r.ok) +
           ",\"n\":" + std::to_string(r.n) + ",\"elementMismatches\":" + std::to_string(r.small_bad) +
           ",\"abftMismatches\":" + std::to_string(r.abft_bad) + ",\"tflops\":" + jnum(gemm_tflops(r.n, r.ms)) +
           ",\"ms\":" + jnum(r.ms) + ",\"cusVerified\":" + std::to_string(r.verified) +
           ",\"badWaves\":" + std::to_string(r.bad_waves) + "}";
  return out + "}";
}

// The host-link phase: the passes' fold plus the host's own sample of what landed in its DRAM.
struct HostLinkResult {
  HbmResult passes;
  uint32_t seed = 0;
  uint64_t samples = 0, sample_bad = 0;
  bool preload = false;
  double alloc_ms = 0;
  bool ok() const { return passes.bad_bits == 0 && sample_bad == 0; }
};

inline std::string host_link_block(const HostLinkResult& r) {
  const HbmResult& p = r.passes;
  const double moved = static_cast<double>(p.n16) * 16.0 * p.patterns;
  const double write_gbps = !r.preload && p.write_ms > 0 ? moved / (p.write_ms * 1e-3) / 1e9 : 0.0;
  const double read_gbps = p.read_ms > 0 ? moved / (p.read_ms * 1e-3) / 1e9 : 0.0;
  const double gbps = r.preload ? read_gbps : std::min(write_gbps, read_gbps);
  return "{\"ok\":" + std::string(jbool(r.ok())) + ",\"bytes\":" + std::to_string(p.n16 * 16) +
         ",\"patterns\":" + std::to_string(p.patterns) + ",\"seed\":" + std::to_string(r.seed) +
         ",\"badBits\":" + std::to_string(p.bad_bits) + ",\"firstBadOffset\":" + joffset(p.first_bad) +
         ",\"hostSamples\":" + std::to_string(r.samples) + ",\"hostSampleMismatches\":" + std::to_string(r.sample_bad) +
         ",\"writeGBps\":" + jnum(write_gbps) + ",\"readGBps\":" + jnum(read_gbps) + ",\"GBps\":" + jnum(gbps) +
         ",\"ms\":" + jnum((r.preload ? 0.0 : p.write_ms) + p.read_ms) + ",\"allocMs\":" + jnum(r.alloc_ms) + "}";
}

// The LDS phase: which CUs a workgroup marched the LDS of, and what it found there. first_bad is
// (CU key << 32) | byte offset of the lowest faulting byte, all-ones = none.
struct LdsResult {
  uint64_t bytes_per_cu = 0;
  int patterns = 0;
  uint32_t salt = 0;
  unsigned long long workgroups = 0;
  int expected = 0, tested = 0, verified = 0, bad_cus = 0;
  int per_xcd[8] = {};  // verified
  unsigned long long bad_bits = 0, first_bad = ~0ull;
  float ms = 0;
  bool require_all = true;  // "requireAllCUs"
  int dump_cu = -1;         // mi355x_probe_lds with an image: the CU key of the dumped workgroup
  bool ok() const { return bad_bits == 0 && (!require_all || verified >= expected); }
};

inline std::string lds_block(const LdsResult& r) {
  std::string out = "{\"ok\":" + std::string(jbool(r.ok())) + ",\"bytesPerCU\":" + std::to_string(r.bytes_per_cu) +
                    ",\"patterns\":" + std::to_string(r.patterns) + ",\"salt\":" + std::to_string(r.salt) +
                    ",\"workgroups\":" + std::to_string(r.workgroups) + ",\"cusTested\":" + std::to_string(r.tested) +
                    ",\"cusVerified\":" + std::to_string(r.verified) + ",\"perXcd\":" + jarray(r.per_xcd, 8) +
                    ",\"badCUs\":" + std::to_string(r.bad_cus) + ",\"badBits\":" + std::to_string(r.bad_bits) +
                    ",\"firstBadCU\":" + first_bad_field(r.first_bad, 32, 0xFFFFFFFFull) +
                    ",\"firstBadOffset\":" + first_bad_field(r.first_bad, 0, 0xFFFFFFFFull) +
                    ",\"ms\":" + jnum(r.ms);
  if (r.dump_cu >= 0) out += ",\"dumpCU\":" + std::to_string(r.dump_cu);
  return out + "}";
}

// The register-file phase: which CUs a workgroup marched all four SIMDs' vector register files of,
// and what it found there. first_bad is (CU key << 32) | SIMD << 16 | register u << 6 | lane of the
// lowest fault, all-ones = none. registers_per_lane / workgroups_per_cu are what the runtime says of
// the kernel: anything but 512 and 1 and the kernel did not own the file it tested.
struct RegsResult {
  int registers_per_lane = 0, workgroups_per_cu = 0;
  int patterns = 0;
  uint32_t salt = 0;
  unsigned long long workgroups = 0, simd_short = 0;
  int expected = 0, tested = 0, verified = 0, bad_cus = 0;
  int per_xcd[8] = {};  // verified
  unsigned long long bad_bits = 0, first_bad = ~0ull;
  float ms = 0;
  bool require_all = true;  // "requireAllCUs"
  int dump_cu = -1;         // mi355x_probe_regs with an image: the CU key of the dumped workgroup
  int dump_simds[4] = {};   // ... and the SIMD each of its four waves ran on
  bool exclusive() const { return registers_per_lane == 512 && workgroups_per_cu == 1; }
  bool ok() const {
    return bad_bits == 0 && exclusive() && simd_short == 0 && (!require_all || verified >= expected);
  }
};

inline std::string regs_block(const RegsResult& r) {
  auto field = [&](int shift, unsigned long long mask) { return first_bad_field(r.first_bad, shift, mask); };
  std::string out = "{\"ok\":" + std::string(jbool(r.ok())) + ",\"registersPerLane\":" + std::to_string(r.registers_per_lane) +
                    ",\"workgroupsPerCU\":" + std::to_string(r.workgroups_per_cu) +
                    ",\"patterns\":" + std::to_string(r.patterns) + ",\"salt\":" + std::to_string(r.salt) +
                    ",\"workgroups\":" + std::to_string(r.workgroups) + ",\"cusTested\":" + std::to_string(r.tested) +
                    ",\"cusVerified\":" + std::to_string(r.verified) + ",\"simdsTested\":" + std::to_string(4 * r.tested) +
                    ",\"simdShort\":" + std::to_string(r.simd_short) + ",\"perXcd\":" + jarray(r.per_xcd, 8) +
                    ",\"badCUs\":" + std::to_string(r.bad_cus) + ",\"badBits\":" + std::to_string(r.bad_bits) +
                    ",\"firstBadCU\":" + field(32, 0xFFFFFFFFull) + ",\"firstBadSimd\":" + field(16, 3) +
                    ",\"firstBadRegister\":" + field(6, 511) + ",\"firstBadLane\":" + field(0, 63) +
                    ",\"ms\":" + jnum(r.ms);
  if (!r.exclusive()) out += ",\"error\":\"RegisterKernelNotExclusive\"";
  out += dump_tail(r.dump_cu, r.dump_simds);
  return out + "}";
}

// The vector-ALU phase: which (CU, SIMD) pairs a wave ran the whole instruction program on with every
// digest as expected. first_bad is (CU key << 32) | SIMD << 16 | group << 8 | lane of the lowest
// mismatch against the host's expectation, all-ones = none. The transcendental group is checked by
// consensus: trans_digest is the value the first wave published, split_waves the waves that got
// another one, suspect (CU key << 2 | SIMD, or -1) the publisher when more than half of the waves
// differ from it and the first differing wave otherwise.
struct AluResult {
  int iters = 0;
  unsigned long long workgroups = 0;
  unsigned long long waves_per_simd[4] = {};
  int expected = 0;  // CUs of the device
  int simds_tested = 0, simds_verified = 0, cus_verified = 0;
  int per_xcd[8] = {};  // verified SIMDs
  unsigned long long bad_waves = 0, bad_lanes = 0, first_bad = ~0ull;
  int bad_cus = 0;  // CUs with a SIMD in the bad map (a mismatch or a split)
  unsigned long long split_waves = 0;
  long long suspect = -1;
  unsigned long long trans_digest = 0;
  float ms = 0;
  bool require_all = true;  // "requireAllCUs"
  int dump_cu = -1;         // mi355x_probe_alu with a dump buffer: the CU key of the dumped workgroup
  int dump_simds[4] = {};   // ... and the SIMD each of its four waves ran on
  unsigned long long waves() const { return waves_per_simd[0] + waves_per_simd[1] + waves_per_simd[2] + waves_per_simd[3]; }
  bool ok() const {
    return bad_waves == 0 && split_waves == 0 && (!require_all || simds_verified >= 4 * expected);
  }
};

inline std::string alu_block(const AluResult& r) {
  static const char* const kNames[] = {"int", "f32", "f64", "f16", "lane", "trans"};
  const bool none = r.first_bad == ~0ull;
  auto field = [&](int shift, unsigned long long mask) { return first_bad_field(r.first_bad, shift, mask); };
  const unsigned long long g = (r.first_bad >> 8) & 0xFF;
  char hex[24];
  std::snprintf(hex, sizeof hex, "\"%016llx\"", r.trans_digest);
  std::string out = "{\"ok\":" + std::string(jbool(r.ok())) + ",\"iters\":" + std::to_string(r.iters) +
                    ",\"workgroups\":" + std::to_string(r.workgroups) + ",\"waves\":" + std::to_string(r.waves()) +
                    ",\"wavesPerSimd\":" + jarray(r.waves_per_simd, 4) + ",\"simdsTested\":" + std::to_string(r.simds_tested) +
                    ",\"simdsVerified\":" + std::to_string(r.simds_verified) +
                    ",\"cusVerified\":" + std::to_string(r.cus_verified) + ",\"perXcd\":" + jarray(r.per_xcd, 8) +
                    ",\"badWaves\":" + std::to_string(r.bad_waves) + ",\"badLanes\":" + std::to_string(r.bad_lanes) +
                    ",\"badCUs\":" + std::to_string(r.bad_cus) +
                    ",\"firstBadCU\":" + field(32, 0xFFFFFFFFull) + ",\"firstBadSimd\":" + field(16, 3) +
                    ",\"firstBadGroup\":" + (none || g > 5 ? std::string("null") : "\"" + std::string(kNames[g]) + "\"") +
                    ",\"firstBadLane\":" + field(0, 63) + ",\"splitWaves\":" + std::to_string(r.split_waves) +
                    ",\"suspectCU\":" + (r.suspect < 0 ? std::string("null") : std::to_string(r.suspect >> 2)) +
                    ",\"suspectSimd\":" + (r.suspect < 0 ? std::string("null") : std::to_string(r.suspect & 3)) +
                    ",\"transDigest\":" + hex + ",\"ms\":" + jnum(r.ms);
  out += dump_tail(r.dump_cu, r.dump_simds);
  return out + "}";
}

// The atomic-unit phase: which CUs' workgroups ran the whole atomic program with every final value
// and every returned value as expected. first_bad is atomics_ref.h's fault_key of the lowest
// mismatch (layer, op, slot, row / XCD, CU key), all-ones = none.
struct AtomResult {
  int iters = 0, layers = 0;
  unsigned long long workgroups = 0;
  unsigned long long wg_per_xcd[8] = {};
  int expected = 0;  // CUs of the device
  int cus_tested = 0, cus_verified = 0, bad_cus = 0;
  int per_xcd[8] = {};  // verified CUs
  unsigned long long bad_workgroups = 0, lds_bad_slots = 0, l2_bad_slots = 0, dev_bad_slots = 0, bad_returns = 0,
                     ticket_faults = 0, first_bad = ~0ull;
  float ms = 0;
  bool require_all = true;  // "requireAllCUs"
  int dump_cu = -1;         // mi355x_probe_atomics with a dump buffer: the CU key of the dumped workgroup
  int dump_simds[4] = {};   // ... and the SIMD each of its four waves ran on
  float march_ms = -1, verify_ms = -1;  // mi355x_probe_atomics with "atomTimeKernels": each kernel's time
  bool ok() const {
    return !bad_workgroups && !lds_bad_slots && !l2_bad_slots && !dev_bad_slots && !bad_returns && !ticket_faults &&
           !bad_cus && (!require_all || cus_verified >= expected);
  }
};

inline std::string atom_block(const AtomResult& r) {
  static const char* const kLayerNames[] = {"lds", "l2", "dev"};
  static const char* const kOpNames[] = {"add", "sub", "and", "or", "xor", "umin", "umax", "smin", "smax", "add_f32",
                                         "pk_add_f16", "pk_add_bf16", "add_x2", "umax_x2", "xor_x2", "add_f64", "max_f64",
                                         "add_rtn", "inc", "dec", "swap", "cas", "ticket", "returns"};
  const bool none = r.first_bad == ~0ull;
  const unsigned long long layer = r.first_bad >> 60, op = (r.first_bad >> 52) & 0xFF, slot = (r.first_bad >> 36) & 0xFFFF,
                           xcc = (r.first_bad >> 32) & 0xF;
  auto name = [&](const char* const* t, unsigned long long i, unsigned long long n) {
    return none || i >= n ? std::string("null") : "\"" + std::string(t[i]) + "\"";
  };
  std::string out = "{\"ok\":" + std::string(jbool(r.ok())) + ",\"iters\":" + std::to_string(r.iters) +
                    ",\"layers\":" + std::to_string(r.layers) + ",\"workgroups\":" + std::to_string(r.workgroups) +
                    ",\"wgPerXcd\":" + jarray(r.wg_per_xcd, 8) + ",\"cusTested\":" + std::to_string(r.cus_tested) +
                    ",\"cusVerified\":" + std::to_string(r.cus_verified) + ",\"perXcd\":" + jarray(r.per_xcd, 8) +
                    ",\"badCUs\":" + std::to_string(r.bad_cus) + ",\"badWorkgroups\":" + std::to_string(r.bad_workgroups) +
                    ",\"ldsBadSlots\":" + std::to_string(r.lds_bad_slots) + ",\"l2BadSlots\":" + std::to_string(r.l2_bad_slots) +
                    ",\"devBadSlots\":" + std::to_string(r.dev_bad_slots) + ",\"badReturns\":" + std::to_string(r.bad_returns) +
                    ",\"ticketFaults\":" + std::to_string(r.ticket_faults) +
                    // the dev layer's rows belong to no CU
                    ",\"firstBadCU\":" + (none || layer == 2 ? std::string("null") : std::to_string(r.first_bad & 0x7FF)) +
                    ",\"firstBadLayer\":" + name(kLayerNames, layer, 3) + ",\"firstBadOp\":" + name(kOpNames, op, 24) +
                    ",\"firstBadSlot\":" + (none ? std::string("null") : std::to_string(slot)) +
                    // lds, l2: the CU's XCD; dev: the row's XCD, 8 for the row every workgroup hits
                    ",\"firstBadXcc\":" + (none ? std::string("null") : std::to_string(xcc)) + ",\"ms\":" + jnum(r.ms);
  out += dump_tail(r.dump_cu, r.dump_simds);
  if (r.march_ms >= 0) out += ",\"marchMs\":" + jnum(r.march_ms) + ",\"verifyMs\":" + jnum(r.verify_ms);
  return out + "}";
}

// Host wall-clock of a probe's steps.
struct PhaseTimes {
  bool arena_reused = false;
  double setup_ms = 0, alloc_ms = 0, launch_ms = 0;
  int hbm_first = 1;
  double hbm_wall_ms = 0, mfma_wall_ms = 0, free_ms = 0;
};

inline std::string phases_block(const PhaseTimes& t) {
  return "{\"arenaReused\":" + std::string(jbool(t.arena_reused)) + ",\"setupMs\":" + jnum(t.setup_ms) +
         ",\"allocMs\":" + jnum(t.alloc_ms) + ",\"launchMs\":" + jnum(t.launch_ms) +
         ",\"hbmFirst\":" + std::to_string(t.hbm_first) + ",\"hbmWallMs\":" + jnum(t.hbm_wall_ms) +
         ",\"mfmaWallMs\":" + jnum(t.mfma_wall_ms) + ",\"freeMs\":" + jnum(t.free_ms) + "}";
}

// The head of a report about one device / one peer link; also what an error report starts with.
inline std::string device_head(int dev) { return "\"device\":" + std::to_string(dev); }

// Everything mi355x_probe_run reports. "cus" only with the MFMA phase, "lowp" only with a dtype,
// "hostLink", "lds", "regs", "alu" and "atomics" only when asked for.
struct ProbeReport {
  int dev = 0;
  std::string uuid, arch;
  HbmResult hbm;
  MfmaResult mfma;
  CusResult cus;
  std::vector<LowpResult> lowp;
  bool has_host_link = false;
  HostLinkResult host_link;
  bool has_lds = false;
  LdsResult lds;
  bool has_regs = false;
  RegsResult regs;
  bool has_alu = false;
  AluResult alu;
  bool has_atom = false;
  AtomResult atom;
  double total_ms = 0;
  PhaseTimes phases;
  bool passed() const {
    bool ok = hbm.ok() && mfma.ok && (!has_host_link || host_link.ok()) && (!has_lds || lds.ok()) &&
              (!has_regs || regs.ok()) && (!has_alu || alu.ok()) && (!has_atom || atom.ok());
    for (const LowpResult& l : lowp) ok = ok && l.ok;
    return ok;
  }
};

// The report up to and including "phases", unclosed: the caller appends "reportMs" (the host time
// spent in here, timing of the binding) and the closing brace.
inline std::string probe_report_open(const ProbeReport& r) {
  std::string out;
  out.reserve(2048);  // one allocation for the whole report
  out += "{" + device_head(r.dev);
  out += ",\"hipUUID\":" + jstr(r.uuid);
  out += ",\"gcnArch\":" + jstr(r.arch);
  out += ",\"passed\":" + std::string(jbool(r.passed()));
  out += ",\"hbm\":" + hbm_block(r.hbm);
  out += ",\"mfma\":" + mfma_block(r.mfma);
  if (r.mfma.enabled) out += ",\"cus\":" + cus_block(r.cus);
  if (!r.lowp.empty()) out += ",\"lowp\":" + lowp_block(r.lowp);
  if (r.has_host_link) out += ",\"hostLink\":" + host_link_block(r.host_link);
  if (r.has_lds) out += ",\"lds\":" + lds_block(r.lds);
  if (r.has_regs) out += ",\"regs\":" + regs_block(r.regs);
  if (r.has_alu) out += ",\"alu\":" + alu_block(r.alu);
  if (r.has_atom) out += ",\"atomics\":" + atom_block(r.atom);
  out += ",\"ms\":" + jnum(r.total_ms);
  out += ",\"phases\":" + phases_block(r.phases);
  return out;
}
inline std::string link_head(int src, int dst) {
  return "\"src\":" + std::to_string(src) + ",\"dst\":" + std::to_string(dst);
}

// ``head`` empty: a report with no head.
inline std::string error_report(const std::string& head, const std::string& what) {
  return "{" + head + (head.empty() ? "" : ",") + "\"passed\":false,\"error\":" + jstr(what) + "}";
}

// One xGMI link: mi355x_probe_peer's whole report and an entry of the ring's "links".
struct PeerLink {
  int src = 0, dst = 0;
  std::string error;  // non-empty: no peer access
  unsigned long long bad_bits = 0, first_bad = ~0ull;  // first_bad: a 16-byte chunk of the receiving window
  uint64_t bytes = 0;
  float ms = 0;
  uint32_t seed = 0;  // what the link was verified with (peer_call_seed: it differs from call to call)
  bool ok() const { return error.empty() && bad_bits == 0; }
};

inline std::string peer_link_block(const PeerLink& l) {
  if (!l.error.empty())
    return "{" + link_head(l.src, l.dst) + ",\"canAccessPeer\":false,\"passed\":false,\"error\":" + jstr(l.error) + "}";
  const double gbps = l.ms > 0 ? static_cast<double>(l.bytes) / (l.ms * 1e-3) / 1e9 : 0.0;
  return "{" + link_head(l.src, l.dst) + ",\"canAccessPeer\":true,\"passed\":" + jbool(l.bad_bits == 0) +
         ",\"badBits\":" + std::to_string(l.bad_bits) + ",\"firstBadOffset\":" + joffset(l.first_bad) +
         ",\"bytes\":" + std::to_string(l.bytes) + ",\"GBps\":" + jnum(gbps) + ",\"ms\":" + jnum(l.ms) +
         ",\"seed\":" + std::to_string(l.seed) + "}";
}

inline std::string peer_ring_report(uint64_t bytes, const std::vector<PeerLink>& links) {
  std::string out = "{\"bytes\":" + std::to_string(bytes) + ",\"links\":[";
  bool all_ok = true;
  for (size_t i = 0; i < links.size(); ++i) {
    all_ok = all_ok && links[i].ok();
    out += (i ? "," : "") + peer_link_block(links[i]);
  }
  return out + "],\"passed\":" + jbool(all_ok) + "}";
}

// One window of the HBM sweep; first_bad counts 16-byte chunks from the window's start.
struct SweepResult {
  int dev = 0;
  uint64_t offset = 0, bytes = 0, span = 0;
  unsigned long long bad_bits = 0, first_bad = ~0ull;
  float ms = 0;
  double alloc_ms = 0;
};

inline std::string sweep_report(const SweepResult& r) {
  const double gbps = r.ms > 0 ? 4.0 * static_cast<double>(r.bytes) / (r.ms * 1e-3) / 1e9 : 0.0;
  return "{" + device_head(r.dev) + ",\"passed\":" + jbool(r.bad_bits == 0) + ",\"offset\":" + std::to_string(r.offset) +
         ",\"bytes\":" + std::to_string(r.bytes) + ",\"span\":" + std::to_string(r.span) +
         ",\"badBits\":" + std::to_string(r.bad_bits) + ",\"firstBadOffset\":" + joffset(r.first_bad, r.offset) +
         ",\"GBps\":" + jnum(gbps) + ",\"ms\":" + jnum(r.ms) + ",\"allocMs\":" + jnum(r.alloc_ms) + "}";
}

}  // namespace
