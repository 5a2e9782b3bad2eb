// The probe's options (native/src/probe/options.h): defaults, clamps, fall-backs and the strings
// the project itself sends, against opt_int key by key.
#include <algorithm>
#include <string>
#include <vector>

#include "../src/probe/options.h"
#include "gpupool/api.h"
#include "gpupool/json.h"
#include "testing.h"

using namespace gpupool;

static ProbeOptions parse(const std::string& s) { return ProbeOptions::parse(s.c_str()); }

static void expect_defaults(const ProbeOptions& o) {
  EXPECT_EQ(o.hbm_bytes, 1ull << 30);
  EXPECT_EQ(o.patterns, 2);
  EXPECT_TRUE(o.cheap_pattern);
  EXPECT_TRUE(!o.tiled);
  EXPECT_EQ(o.fill_blocks_per_cu, 1LL);
  EXPECT_EQ(o.verify_blocks_per_cu, 3LL);
  EXPECT_EQ(o.inject_flips, 0);
  EXPECT_EQ(o.inject_chunk, -1LL);
  EXPECT_TRUE(o.mfma);
  EXPECT_EQ(o.gemm_n, 4096);
  EXPECT_EQ(o.gemm.variant.tile, 256);
  EXPECT_EQ(o.gemm.variant.pipe, kGemmPipe);
  EXPECT_TRUE(!o.gemm.variant.prio && !o.gemm.variant.vec_c && !o.gemm.poison_c);
  EXPECT_EQ(o.gemm.group_m, kGemmGroupM);
  EXPECT_EQ(o.reps, 1);
  EXPECT_EQ(o.inject_gemm, 0);
  EXPECT_EQ(o.inject_gemm_at.row, -1LL);
  EXPECT_EQ(o.inject_gemm_at.col, -1LL);
  EXPECT_EQ(o.census_fault_xcc, -1);
  EXPECT_TRUE(o.require_all_cus);
  EXPECT_TRUE(!o.cu_keys);
  EXPECT_EQ(o.lowp_mask, 0);
  EXPECT_EQ(o.inject_lowp, 0);
  EXPECT_EQ(o.lowp_census_fault_xcc, -1);
  EXPECT_TRUE(o.overlap);
  EXPECT_EQ(o.hbm_first, 1);
  EXPECT_TRUE(o.zero_in_kernel);
  EXPECT_TRUE(o.keep_arena);
  EXPECT_EQ(o.host_link.n16, 0ull);
  EXPECT_TRUE(!o.host_link_on_mfma_stream);
}

TEST(probe_options_defaults) {
  expect_defaults(ProbeOptions::parse(nullptr));
  expect_defaults(parse("{}"));
}

TEST(probe_options_clamps) {
  const int gemm_in[] = {0, 255, 256, 300, 4097}, gemm_out[] = {256, 256, 256, 256, 4096};
  for (int i = 0; i < 5; ++i) EXPECT_EQ(parse("{\"gemmN\":" + std::to_string(gemm_in[i]) + "}").gemm_n, gemm_out[i]);
  const int pat_in[] = {0, 1, 4, 9}, pat_out[] = {1, 1, 4, 4};
  for (int i = 0; i < 4; ++i) EXPECT_EQ(parse("{\"patterns\":" + std::to_string(pat_in[i]) + "}").patterns, pat_out[i]);
  const int inj_in[] = {-1, 4096, 5000}, inj_out[] = {0, 4096, 4096};
  for (int i = 0; i < 3; ++i)
    EXPECT_EQ(parse("{\"injectBitFlips\":" + std::to_string(inj_in[i]) + "}").inject_flips, inj_out[i]);
  EXPECT_EQ(parse(R"({"gemmTile":128})").gemm.variant.tile, 128);
  EXPECT_EQ(parse(R"({"gemmTile":64})").gemm.variant.tile, 256);  // a probe runs 256 unless 128 is asked for
  EXPECT_EQ(GemmOptions::parse(R"({"gemmTile":64})").variant.tile, 64);  // the host-buffer entry point refuses it
  EXPECT_EQ(parse(R"({"gemmReps":0})").reps, 1);
  EXPECT_EQ(parse(R"({"gemmReps":5})").reps, 5);
  EXPECT_EQ(parse(R"({"gemmReps":5,"gemmSkip":1})").reps, 0);
}

TEST(probe_options_bool_forms_and_spaces) {
  EXPECT_TRUE(!parse(R"({"mfma":false})").mfma);
  EXPECT_TRUE(parse(R"({"mfma":true})").mfma);
  EXPECT_TRUE(!parse(R"({"mfma":   false})").mfma);
  EXPECT_TRUE(!parse(R"({"overlap":0})").overlap);
  EXPECT_TRUE(parse(R"({"cuKeys": true})").cu_keys);
  EXPECT_EQ(parse(R"({"gemmN":  512})").gemm_n, 512);
  EXPECT_EQ(parse(R"({"gemmN":512,"gemmN":1024})").gemm_n, 512);  // first occurrence
}

TEST(probe_options_hbm_blocks_fallback) {
  auto both = [](const std::string& s) {
    const ProbeOptions o = parse(s);
    return std::to_string(o.fill_blocks_per_cu) + "/" + std::to_string(o.verify_blocks_per_cu);
  };
  EXPECT_EQ(both("{}"), std::string("1/3"));
  EXPECT_EQ(both(R"({"hbmBlocksPerCU":8})"), std::string("8/8"));
  EXPECT_EQ(both(R"({"hbmBlocksPerCU":8,"hbmFillBlocksPerCU":2})"), std::string("2/8"));
  EXPECT_EQ(both(R"({"hbmBlocksPerCU":8,"hbmVerifyBlocksPerCU":5})"), std::string("8/5"));
  EXPECT_EQ(both(R"({"hbmFillBlocksPerCU":0,"hbmVerifyBlocksPerCU":-2})"), std::string("1/1"));
  // a key that is only the tail of another key is not that key
  EXPECT_EQ(both(R"({"hbmFillBlocksPerCU":4})"), std::string("4/3"));
  EXPECT_EQ(opt_int(R"({"hbmFillBlocksPerCU":4})", "hbmBlocksPerCU", -7), -7LL);
}

TEST(probe_options_low_precision_mask) {
  EXPECT_EQ(parse(R"({"mfmaLowPrecision":7})").lowp_mask, 7);
  EXPECT_EQ(parse(R"({"mfmaLowPrecision":15})").lowp_mask, 7);
  EXPECT_EQ(parse(R"({"mfmaLowPrecision":5})").lowp_mask, 5);
  EXPECT_EQ(parse(R"({"mfma":false,"mfmaLowPrecision":7})").lowp_mask, 0);
}

TEST(probe_options_gemm_fault_position) {
  const ProbeOptions d = parse(R"({"injectGemmFault":1})");
  EXPECT_EQ(d.inject_gemm_at.row, -1LL);
  EXPECT_EQ(d.inject_gemm_at.col, -1LL);
  EXPECT_EQ(d.inject_gemm_at.index(512), 170LL * 512 + 102);  // n/3, n/5: where the hook always struck
  EXPECT_EQ(d.inject_gemm_at.index(1024), 341LL * 1024 + 204);
  const ProbeOptions at = parse(R"({"injectGemmFault":1,"injectGemmFaultRow":511,"injectGemmFaultCol":0})");
  EXPECT_EQ(at.inject_gemm, 1);  // the longer keys are not the mode's key
  EXPECT_EQ(at.inject_gemm_at.index(512), 511LL * 512);
  EXPECT_EQ(at.inject_gemm_at.index(256), -1LL);  // row out of range: no fault
  EXPECT_EQ(parse(R"({"injectGemmFaultRow":0,"injectGemmFaultCol":0})").inject_gemm_at.index(256), 0LL);
  EXPECT_EQ(parse(R"({"injectGemmFaultRow":3})").inject_gemm_at.index(500), 3LL * 500 + 100);  // one default
  EXPECT_EQ(parse(R"({"injectGemmFaultCol":512})").inject_gemm_at.index(512), -1LL);
  EXPECT_EQ(parse(R"({"injectGemmFaultCol":-2})").inject_gemm_at.index(512), -1LL);
  EXPECT_EQ(parse(R"({"injectGemmFaultRow":-7,"injectGemmFaultCol":5})").inject_gemm_at.index(512), -1LL);
  EXPECT_EQ(parse(R"({"injectGemmFaultRow":65535,"injectGemmFaultCol":65535})").inject_gemm_at.index(65536),
            65535LL * 65536 + 65535);  // no 32-bit wrap
}

TEST(probe_options_host_link) {
  EXPECT_EQ(parse(R"({"hostLinkBytes":0,"hostLinkPatterns":3})").host_link.patterns, 2);  // off: nothing is looked up
  const ProbeOptions at = parse(R"({"hostLinkBytes":4294967296})");
  EXPECT_EQ(at.host_link.n16, (4ull << 30) / 16);
  EXPECT_THROW(parse(R"({"hostLinkBytes":4294967297})"));
  const ProbeOptions o = ProbeOptions::parse(
      R"({"hostLinkBytes":1048576,"hostLinkPatterns":9,"hostLinkGrid":5000,"hostLinkUnroll":4,"hostLinkNT":1,)"
      R"("hostLinkCoherent":0,"injectHostLinkFlipAtChunk":12,"hostLinkStream":1})",
      3);
  EXPECT_EQ(o.host_link.n16, 65536ull);
  EXPECT_EQ(o.host_link.patterns, 4);
  EXPECT_EQ(o.host_link.grid, hostlink::kMaxGrid);
  EXPECT_EQ(o.host_link.unroll, 4);
  EXPECT_TRUE(o.host_link.nt && !o.host_link.coherent);
  EXPECT_EQ(o.host_link.inject_chunk, 12LL);
  EXPECT_EQ(o.host_link.seed, 0x4C4B0003u);
  EXPECT_TRUE(o.host_link_on_mfma_stream);
  EXPECT_TRUE(!parse(R"({"hostLinkBytes":1048576,"hostLinkStream":1,"overlap":0})").host_link_on_mfma_stream);
  EXPECT_EQ(parse(R"({"hostLinkBytes":1048576,"hostLinkGrid":0})").host_link.grid, 1);
}

TEST(probe_options_other_entry_points) {
  EXPECT_EQ(peer_bytes(nullptr, 256LL << 20), 256ull << 20);
  EXPECT_EQ(peer_bytes(R"({"bytes":4096})", 64LL << 20), 1ull << 20);
  EXPECT_EQ(peer_bytes(R"({"bytes":2097152})", 64LL << 20), 2ull << 20);
  const SweepOptions d = SweepOptions::parse(nullptr);
  EXPECT_EQ(d.bytes, 16ull << 30);
  EXPECT_EQ(d.reserve, 4ull << 30);
  EXPECT_EQ(d.offset, 0ull);
  EXPECT_TRUE(!d.keep);
  const SweepOptions s = SweepOptions::parse(R"({"bytes":1,"reserve":-5,"offset":-1,"keep":1,"injectBitFlips":9999})");
  EXPECT_EQ(s.bytes, 1ull << 20);
  EXPECT_EQ(s.reserve, 0ull);
  EXPECT_EQ(s.offset, 0ull);
  EXPECT_TRUE(s.keep);
  EXPECT_EQ(s.inject_flips, 4096);
  EXPECT_EQ(d.inject_chunk, -1LL);
  EXPECT_EQ(s.inject_chunk, -1LL);
  EXPECT_EQ(SweepOptions::parse(R"({"injectFlipAtChunk": 65536})").inject_chunk, 65536LL);
  const HostLinkOptions h = HostLinkOptions::parse(R"({"preload":true,"hostLinkBytes":64})");
  EXPECT_TRUE(h.preload);
  EXPECT_EQ(h.bytes, 64ull);
}

TEST(probe_options_peer) {
  // defaults: the entry point's size, no hook
  for (long long def : {256LL << 20, 64LL << 20}) {
    const PeerOptions d = PeerOptions::parse(nullptr, def);
    EXPECT_EQ(d.bytes, static_cast<uint64_t>(def));
    EXPECT_EQ(d.inject_chunk, -1LL);
    EXPECT_EQ(d.inject_flips, 0);
    EXPECT_EQ(d.inject_link, 0);
    EXPECT_TRUE(!d.skip_copy);
    EXPECT_EQ(d.flip_chunk(65536), -1LL);
  }
  // what probe.peer / probe.peer_ring send
  const PeerOptions o = PeerOptions::parse(
      R"({"bytes": 4194312, "injectFlipAtChunk": 262143, "injectBitFlips": 37, "injectLink": 2, "skipCopy": 1})", 64LL << 20);
  EXPECT_EQ(o.bytes, 4194312ull);  // the checks round down to 16, not the parser
  EXPECT_EQ(o.bytes, peer_bytes(R"({"bytes": 4194312})", 64LL << 20));
  EXPECT_EQ(o.inject_chunk, 262143LL);
  EXPECT_EQ(o.inject_flips, 37);
  EXPECT_EQ(o.inject_link, 2);
  EXPECT_TRUE(o.skip_copy);
  // the flip is in range only below n16: the last chunk yes, one past it and anything negative no
  EXPECT_EQ(o.flip_chunk(262144), 262143LL);
  EXPECT_EQ(o.flip_chunk(262143), -1LL);
  EXPECT_EQ(PeerOptions::parse(R"({"injectFlipAtChunk":0})", 1 << 20).flip_chunk(1), 0LL);
  EXPECT_EQ(PeerOptions::parse(R"({"injectFlipAtChunk":-7})", 1 << 20).flip_chunk(65536), -1LL);
  // clamps
  const PeerOptions c = PeerOptions::parse(R"({"bytes":16,"injectBitFlips":9999,"injectLink":-3,"skipCopy":false})", 64LL << 20);
  EXPECT_EQ(c.bytes, 1ull << 20);
  EXPECT_EQ(c.inject_flips, 4096);
  EXPECT_EQ(c.inject_link, 0);
  EXPECT_TRUE(!c.skip_copy);
  EXPECT_EQ(PeerOptions::parse(R"({"injectBitFlips":-1})", 1 << 20).inject_flips, 0);
  EXPECT_TRUE(PeerOptions::parse(R"({"skipCopy":true})", 1 << 20).skip_copy);
}

TEST(probe_peer_call_seed) {
  const uint32_t pair01 = 0x5EED0000u + 1, ring0 = 0x5EED0000u, ring1 = 0x5EED0000u + 0x9E37u;
  // one base: no two of many consecutive calls share a seed, and none equals the bare base
  for (uint32_t base : {pair01, ring0, ring1}) {
    std::vector<uint32_t> seen;
    for (uint32_t nonce = 1; nonce <= 4096; ++nonce) seen.push_back(peer_call_seed(base, nonce));
    for (uint32_t s : seen) EXPECT_TRUE(s != base);
    std::sort(seen.begin(), seen.end());
    EXPECT_TRUE(std::adjacent_find(seen.begin(), seen.end()) == seen.end());
  }
  // one call: the devices of a ring keep distinct seeds (a window copied from the wrong source fails)
  for (uint32_t nonce : {1u, 2u, 0x80000000u, 0xFFFFFFFFu})
    for (uint32_t a = 0; a < 64; ++a)
      for (uint32_t b = a + 1; b < 64; ++b)
        EXPECT_TRUE(peer_call_seed(0x5EED0000u + a * 0x9E37u, nonce) != peer_call_seed(0x5EED0000u + b * 0x9E37u, nonce));
  // the counter wrapping after 2^32 calls is the only repeat
  EXPECT_EQ(peer_call_seed(ring0, 0), ring0);
  EXPECT_EQ(peer_call_seed(ring0, 1), ring0 ^ 0x9E3779B1u);
}

// Every field against the opt_int expression it replaces in run_probe, on a string the project sends.
static void expect_matches_opt_int(const std::string& str) {
  const char* j = str.c_str();
  const ProbeOptions o = ProbeOptions::parse(j);
  EXPECT_EQ(o.hbm_bytes, static_cast<uint64_t>(opt_int(j, "hbmBytes", 1LL << 30)));
  EXPECT_EQ(o.mfma, opt_int(j, "mfma", 1) != 0);
  EXPECT_EQ(o.gemm_n, std::max(256, (static_cast<int>(opt_int(j, "gemmN", 4096)) / 256) * 256));
  EXPECT_EQ(o.patterns, static_cast<int>(std::min(kMaxPatterns, std::max(1LL, opt_int(j, "patterns", 2)))));
  EXPECT_EQ(o.inject_flips, static_cast<int>(std::min(4096LL, std::max(0LL, opt_int(j, "injectBitFlips", 0)))));
  EXPECT_EQ(o.inject_gemm, static_cast<int>(opt_int(j, "injectGemmFault", 0)));
  EXPECT_EQ(o.inject_chunk, opt_int(j, "injectFlipAtChunk", -1));
  EXPECT_EQ(o.gemm.variant.tile, opt_int(j, "gemmTile", 256) != 128 ? 256 : 128);
  EXPECT_EQ(o.gemm.group_m, static_cast<int>(opt_int(j, "gemmGroupM", kGemmGroupM)));
  EXPECT_EQ(o.gemm.variant.pipe, static_cast<int>(opt_int(j, "gemmPipe", kGemmPipe)));
  EXPECT_EQ(o.gemm.variant.prio, opt_int(j, "gemmPrio", 0) != 0);
  EXPECT_EQ(o.gemm.variant.vec_c, opt_int(j, "gemmVecC", 0) != 0);
  EXPECT_EQ(o.gemm.poison_c, opt_int(j, "poisonC", 0) != 0);
  EXPECT_EQ(o.lowp_mask, o.mfma ? static_cast<int>(opt_int(j, "mfmaLowPrecision", 0)) & 7 : 0);
  EXPECT_EQ(o.inject_lowp, static_cast<int>(opt_int(j, "injectLowpFault", 0)));
  EXPECT_EQ(o.lowp_census_fault_xcc, static_cast<int>(opt_int(j, "injectLowpCensusFaultXcc", -1)));
  EXPECT_EQ(o.overlap, opt_int(j, "overlap", 1) != 0);
  EXPECT_EQ(o.keep_arena, opt_int(j, "keepArena", 1) != 0);
  EXPECT_EQ(o.zero_in_kernel, opt_int(j, "zeroInKernel", 1) != 0);
  EXPECT_EQ(o.require_all_cus, opt_int(j, "requireAllCUs", 1) != 0);
  EXPECT_EQ(o.reps, opt_int(j, "gemmSkip", 0) ? 0 : static_cast<int>(std::max(1LL, opt_int(j, "gemmReps", 1))));
  EXPECT_EQ(o.census_fault_xcc, static_cast<int>(opt_int(j, "injectCensusFaultXcc", -1)));
  EXPECT_EQ(o.cu_keys, opt_int(j, "cuKeys", 0) != 0);
  EXPECT_EQ(o.hbm_first, static_cast<int>(opt_int(j, "hbmFirst", 1)));
  EXPECT_EQ(o.fill_blocks_per_cu, std::max(1LL, opt_int(j, "hbmFillBlocksPerCU", opt_int(j, "hbmBlocksPerCU", 1))));
  EXPECT_EQ(o.verify_blocks_per_cu, std::max(1LL, opt_int(j, "hbmVerifyBlocksPerCU", opt_int(j, "hbmBlocksPerCU", 3))));
  EXPECT_EQ(o.cheap_pattern, opt_int(j, "hbmPattern", kHbmPattern) == 1);
  EXPECT_EQ(o.tiled, o.cheap_pattern && opt_int(j, "hbmLayout", kHbmLayout) == 1);
  const uint64_t hl = static_cast<uint64_t>(std::max(0LL, opt_int(j, "hostLinkBytes", 0)));
  EXPECT_EQ(o.host_link.n16, hl / 16);
  if (hl) {
    EXPECT_EQ(o.host_link.patterns, static_cast<int>(std::min(kMaxPatterns, std::max(1LL, opt_int(j, "hostLinkPatterns", 2)))));
    EXPECT_EQ(o.host_link.inject_chunk, opt_int(j, "injectHostLinkFlipAtChunk", -1));
    EXPECT_EQ(o.host_link.grid, static_cast<int>(std::min<long long>(hostlink::kMaxGrid,
                                                                       std::max(1LL, opt_int(j, "hostLinkGrid", hostlink::kGrid)))));
    EXPECT_EQ(o.host_link.unroll, static_cast<int>(opt_int(j, "hostLinkUnroll", hostlink::kUnroll)));
    EXPECT_EQ(o.host_link.nt, opt_int(j, "hostLinkNT", hostlink::kNonTemporal) != 0);
    EXPECT_EQ(o.host_link.coherent, opt_int(j, "hostLinkCoherent", hostlink::kCoherent) != 0);
    EXPECT_EQ(o.host_link_on_mfma_stream, o.overlap && opt_int(j, "hostLinkStream", 0) == 1);
  }
}

TEST(probe_options_strings_the_project_sends) {
  // the warm-up probe of mi355x_probe_init
  const std::string warm = R"({"hbmBytes":1048576,"patterns":1,"gemmN":256,"gemmReps":1,"keepArena":0})";
  expect_matches_opt_int(warm);
  const ProbeOptions w = parse(warm);
  EXPECT_EQ(w.hbm_bytes, 1048576ull);
  EXPECT_EQ(w.patterns, 1);
  EXPECT_EQ(w.gemm_n, 256);
  EXPECT_TRUE(!w.keep_arena);
  // the pool's probe options, default and with the opt-in phases
  auto pool = [](const std::string& probe) {
    return Mi355xPoolSpec::from(Json::parse(R"({"kind":"Mi355xPool","spec":{"replicas":1,"probe":)" + probe + "}}")["spec"])
        .probe_json()
        .dump();
  };
  const std::string plain = pool("{}");
  expect_matches_opt_int(plain);
  EXPECT_EQ(parse(plain).host_link.n16, 0ull);
  const std::string full = pool(R"({"mfmaLowPrecision":["fp8","mxfp4"],"hostLinkCheck":true})");
  EXPECT_TRUE(full.find("hostLinkBytes") != std::string::npos);
  expect_matches_opt_int(full);
  EXPECT_TRUE(parse(full).host_link.n16 > 0);
}
