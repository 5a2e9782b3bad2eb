// spec.probe.ldsCheck on the host side: the probe library's options ("ldsCheck" and the phase's keys),
// the address pass's stride, the "lds" report block byte for byte, and the manager's API layer (parse,
// the probe options sent with claims and rechecks, InvalidSpec validation, the device status).
#include <string>
#include <vector>

#include "../src/probe/options.h"
#include "../src/probe/report.h"
#include "gpupool/api.h"
#include "gpupool/json.h"
#include "gpupool/provider.h"
#include "testing.h"

using namespace gpupool;
using S = std::string;

static ProbeOptions parse(const S& s, int dev = 0) { return ProbeOptions::parse(s.c_str(), dev); }

static void expect_off(const ProbeOptions& o) {
  const lds::Plan d;
  EXPECT_EQ(o.lds.n16, 0u);
  EXPECT_EQ(o.lds.patterns, d.patterns);
  EXPECT_TRUE(!o.lds.salt_given);
  EXPECT_EQ(o.lds.salt, 0u);
  EXPECT_EQ(o.lds.seed, 0u);
  EXPECT_EQ(o.lds.blocks_per_cu, lds::kBlocksPerCU);
  EXPECT_EQ(o.lds.flip_byte, -1LL);
  EXPECT_EQ(o.lds.fault_xcc, -1);
  EXPECT_EQ(o.lds.skip_chunk, -1LL);
  EXPECT_EQ(o.lds.dump_stage, 0);
  EXPECT_EQ(o.lds_first, lds::kFirst == 1);
}

TEST(lds_options_off_looks_nothing_up) {
  expect_off(ProbeOptions::parse(nullptr));
  expect_off(parse("{}"));
  expect_off(parse(R"({"ldsCheck":0,"ldsBytes":1600,"ldsPatterns":3,"ldsSalt":9,"ldsBlocksPerCU":2,"ldsFirst":1,)"
                   R"("injectLdsFlipAtByte":5,"injectLdsFaultXcc":3,"injectLdsSkipChunk":1,"ldsDumpStage":2})"));
  expect_off(parse(R"({"ldsCheck":false,"ldsBytes":8})"));  // not even the range check
}

TEST(lds_options_defaults_and_clamps) {
  const ProbeOptions o = parse(R"({"ldsCheck":1})", 3);
  EXPECT_EQ(o.lds.n16, 10240u);
  EXPECT_EQ(o.lds.patterns, 2);
  EXPECT_TRUE(!o.lds.salt_given);
  EXPECT_EQ(o.lds.seed, 0x4C445303u);
  EXPECT_EQ(o.lds.blocks_per_cu, lds::kBlocksPerCU);
  EXPECT_EQ(o.lds.flip_byte, -1LL);
  EXPECT_EQ(o.lds.fault_xcc, -1);
  EXPECT_EQ(o.lds.skip_chunk, -1LL);
  EXPECT_EQ(o.lds.dump_stage, 0);
  EXPECT_EQ(o.lds_first, lds::kFirst == 1);
  EXPECT_TRUE(parse(R"({"ldsCheck":true})").lds.n16 == 10240u);
  // every other option of the probe is what it is without the check
  const ProbeOptions plain = parse("{}");
  EXPECT_EQ(o.hbm_bytes, plain.hbm_bytes);
  EXPECT_EQ(o.gemm_n, plain.gemm_n);
  EXPECT_EQ(o.overlap, plain.overlap);
  EXPECT_EQ(o.host_link.n16, 0ull);

  const long long bytes_in[] = {16, 31, 1600, 163832, 163840}, n16_out[] = {1, 1, 100, 10239, 10240};
  for (int i = 0; i < 5; ++i)
    EXPECT_EQ(parse("{\"ldsCheck\":1,\"ldsBytes\":" + std::to_string(bytes_in[i]) + "}").lds.n16,
              static_cast<uint32_t>(n16_out[i]));
  for (const char* bad : {"0", "8", "15", "-16", "163841", "200000"}) {
    bool threw = false;
    try {
      parse(S("{\"ldsCheck\":1,\"ldsBytes\":") + bad + "}");
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    EXPECT_TRUE(threw);
  }
  const int pat_in[] = {0, 1, 4, 9}, pat_out[] = {1, 1, 4, 4};
  for (int i = 0; i < 4; ++i)
    EXPECT_EQ(parse("{\"ldsCheck\":1,\"ldsPatterns\":" + std::to_string(pat_in[i]) + "}").lds.patterns, pat_out[i]);
  const int blk_in[] = {-1, 0, 1, 16, 64, 1000}, blk_out[] = {1, 1, 1, 16, 64, 64};
  for (int i = 0; i < 6; ++i)
    EXPECT_EQ(parse("{\"ldsCheck\":1,\"ldsBlocksPerCU\":" + std::to_string(blk_in[i]) + "}").lds.blocks_per_cu, blk_out[i]);
  const ProbeOptions s = parse(R"({"ldsCheck":1,"ldsSalt":0})");
  EXPECT_TRUE(s.lds.salt_given && s.lds.salt == 0u);
  const ProbeOptions h = parse(R"({"ldsCheck":1,"ldsSalt":77,"ldsFirst":1,"injectLdsFlipAtByte":163839,)"
                               R"("injectLdsFaultXcc":3,"injectLdsSkipChunk":10239,"ldsDumpStage":2})");
  EXPECT_TRUE(h.lds.salt_given && h.lds.salt == 77u);
  EXPECT_TRUE(h.lds_first);
  EXPECT_EQ(h.lds.flip_byte, 163839LL);
  EXPECT_EQ(h.lds.fault_xcc, 3);
  EXPECT_EQ(h.lds.skip_chunk, 10239LL);
  EXPECT_EQ(h.lds.dump_stage, 0);  // a probe has no caller buffer to dump into
  EXPECT_TRUE(!parse(R"({"ldsCheck":1,"ldsFirst":0})").lds_first);
  // the phase alone reads the stage, 1..3
  const int st_in[] = {0, 1, 3, 4, -1}, st_out[] = {0, 1, 3, 0, 0};
  for (int i = 0; i < 5; ++i)
    EXPECT_EQ(lds::Plan::parse(("{\"ldsDumpStage\":" + std::to_string(st_in[i]) + "}").c_str(), 0).dump_stage, st_out[i]);
  EXPECT_EQ(lds::Plan::parse(nullptr, 0).n16, 10240u);
}

TEST(lds_stride_is_odd_coprime_and_a_bijection) {
  for (uint32_t n : {4u, 400u, 660u, 1028u, 16388u, 40956u, 40960u}) {
    const uint32_t s = lds::stride_for(n);
    EXPECT_TRUE(s >= 33 && (s & 1));
    uint32_t a = s, b = n;
    while (b) {
      const uint32_t r = a % b;
      a = b;
      b = r;
    }
    EXPECT_EQ(a, 1u);
    for (uint32_t c = 33; c < s; c += 2) {  // the smallest such value: every smaller candidate shares a factor
      uint32_t x = c, y = n;
      while (y) {
        const uint32_t r = x % y;
        x = y;
        y = r;
      }
      EXPECT_TRUE(x > 1);
    }
    std::vector<unsigned char> hit(n, 0);
    for (uint32_t d = 0; d < n; ++d) ++hit[static_cast<uint64_t>(d) * s % n];
    size_t once = 0;
    for (unsigned char h : hit) once += h == 1;
    EXPECT_EQ(once, static_cast<size_t>(n));
  }
  EXPECT_EQ(lds::stride_for(4), 33u);
  EXPECT_EQ(lds::stride_for(40960), 33u);
  EXPECT_EQ(lds::stride_for(660), 37u);  // 660 = 33 * 20 shares 3 and 11 with 33, 5 with 35
  lds::Plan pl;
  pl.n16 = 165;  // 660 dwords
  EXPECT_EQ(pl.stride(), 37u);
}

static LdsResult clean() {
  LdsResult r;
  r.bytes_per_cu = 163840;
  r.patterns = 2;
  r.salt = 5;
  r.workgroups = 1024;
  r.expected = r.tested = r.verified = 256;
  for (int& x : r.per_xcd) x = 32;
  r.ms = 0.125f;
  return r;
}

TEST(lds_block_byte_for_byte) {
  EXPECT_EQ(lds_block(clean()),
            S(R"({"ok":true,"bytesPerCU":163840,"patterns":2,"salt":5,"workgroups":1024,"cusTested":256,"cusVerified":256,)"
              R"("perXcd":[32,32,32,32,32,32,32,32],"badCUs":0,"badBits":0,"firstBadCU":null,"firstBadOffset":null,"ms":0.125})"));
  LdsResult f = clean();
  f.verified = 255;
  f.per_xcd[3] = 31;
  f.bad_cus = 1;
  f.bad_bits = 3;
  f.first_bad = (0x365ull << 32) | 163839ull;
  EXPECT_TRUE(!f.ok());
  EXPECT_EQ(lds_block(f),
            S(R"({"ok":false,"bytesPerCU":163840,"patterns":2,"salt":5,"workgroups":1024,"cusTested":256,"cusVerified":255,)"
              R"("perXcd":[32,32,32,31,32,32,32,32],"badCUs":1,"badBits":3,"firstBadCU":869,"firstBadOffset":163839,"ms":0.125})"));
  // coverage: short of every CU fails unless "requireAllCUs" is off; a bad bit fails either way
  LdsResult s = clean();
  s.tested = s.verified = 250;
  EXPECT_TRUE(!s.ok());
  s.require_all = false;
  EXPECT_TRUE(s.ok());
  f.require_all = false;
  EXPECT_TRUE(!f.ok());
  // the phase alone, with an image: the dumped workgroup's CU after "ms"
  LdsResult d = clean();
  d.dump_cu = 17;
  const S out = lds_block(d);
  EXPECT_TRUE(out.size() > 13 && out.substr(out.size() - 24) == S(R"(,"ms":0.125,"dumpCU":17})"));
}

static ProbeReport plain_report() {
  ProbeReport r;
  r.uuid = "GPU-ab";
  r.arch = "gfx950";
  r.hbm.n16 = 65536;
  r.hbm.patterns = 2;
  r.hbm.write_ms = 0.5f;
  r.hbm.read_ms = 0.25f;
  r.mfma.enabled = true;
  r.mfma.n = 256;
  r.cus.expected = r.cus.verified = 256;
  r.total_ms = 2.5;
  return r;
}

TEST(lds_block_in_the_report_only_when_asked) {
  const ProbeReport r = plain_report();
  const S base = probe_report_open(r);
  EXPECT_TRUE(base.find("\"lds\"") == S::npos);
  // the default report, byte for byte what it was
  EXPECT_EQ(base,
            S(R"({"device":0,"hipUUID":"GPU-ab","gcnArch":"gfx950","passed":true,"hbm":{"ok":true,"bytes":1048576,"patterns":2,)"
              R"("badBits":0,"firstBadOffset":null,"writeGBps":4.1943,"readGBps":8.38861,"GBps":5.59241,"ms":0.75},)"
              R"("mfma":{"ok":true,"enabled":true,"n":256,"tile":256,"pipe":0,"elementMismatches":0,"abftMismatches":0,"tflops":0,"ms":0},)"
              R"("cus":{"expected":256,"mfmaVerified":256,"perXcd":[0,0,0,0,0,0,0,0],"gemmTiles":0,"badWaves":0,"ok":true},)"
              R"("ms":2.5,"phases":{"arenaReused":false,"setupMs":0,"allocMs":0,"launchMs":0,"hbmFirst":1,"hbmWallMs":0,"mfmaWallMs":0,"freeMs":0})"));
  ProbeReport q = r;
  q.lds = clean();  // a result without the flag reports nothing and fails nothing
  q.lds.bad_bits = 1;
  EXPECT_EQ(probe_report_open(q), base);
  q.has_lds = true;
  q.has_host_link = true;
  q.host_link.passes = r.hbm;
  const S out = probe_report_open(q);
  EXPECT_TRUE(out.find("\"passed\":false") != S::npos);
  const size_t hl = out.find(",\"hostLink\":{"), ld = out.find(",\"lds\":{\"ok\":false"), ms = out.find(",\"ms\":2.5,\"phases\"");
  EXPECT_TRUE(hl != S::npos && ld != S::npos && ms != S::npos);
  EXPECT_TRUE(hl < ld && ld < ms);
  q.lds.bad_bits = 0;
  EXPECT_TRUE(probe_report_open(q).find("\"passed\":true") != S::npos);
}

static Json pool(const S& probe) {
  return Json::parse(R"({"kind":"Mi355xPool","spec":{"replicas":1,"probe":)" + probe + "}}");
}

TEST(lds_spec_parse_validate_and_status) {
  auto none = Mi355xPoolSpec::from(pool("{}")["spec"]);
  EXPECT_TRUE(!none.probe_lds_check);
  // the default claim and the recheck policy carry today's options
  EXPECT_TRUE(!none.probe_json().contains("ldsCheck"));
  EXPECT_TRUE(!none.policy_json()["probe"].contains("ldsCheck"));
  EXPECT_EQ(none.probe_json().dump(), Mi355xPoolSpec::from(pool(R"({"ldsCheck":false})")["spec"]).probe_json().dump());
  auto on = Mi355xPoolSpec::from(pool(R"({"ldsCheck":true})")["spec"]);
  EXPECT_TRUE(on.probe_lds_check);
  EXPECT_TRUE(on.probe_json()["ldsCheck"].as_bool(false));
  EXPECT_TRUE(on.policy_json().path("probe.ldsCheck").as_bool(false));
  EXPECT_TRUE(!on.probe_json().contains("hostLinkCheck"));

  for (const char* good : {R"({"ldsCheck":true})", R"({"ldsCheck":false})", R"({"ldsCheck":true,"hostLinkCheck":true})"})
    EXPECT_TRUE(validate_mi355x(pool(good)).empty());
  for (const char* bad : {R"({"ldsCheck":"yes"})", R"({"ldsCheck":1})", R"({"ldsCheck":null})"}) {
    auto errs = validate_mi355x(pool(bad));
    EXPECT_EQ(errs.size(), 1u);
    EXPECT_TRUE(errs.size() == 1 && errs[0].find("spec.probe.ldsCheck") != S::npos);
  }

  auto view = [](const S& probe) {
    return DeviceView::from(Json::parse(R"({"uuid":"u0","state":"Claimed","healthy":true,"probe":)" + probe + "}"))
        .status_json();
  };
  Json with = view(R"({"passed":true,"lds":{"ok":true,"cusTested":256,"cusVerified":256}})");
  EXPECT_EQ(with.path("probe.ldsVerifiedCUs").as_int(0), static_cast<int64_t>(256));
  Json failed = view(R"j({"passed":false,"error":"LDSPatternMismatch: 1 flipped bit(s) on 1 CU(s), first on CU 0/0/0/0 at LDS offset 0",
                         "lds":{"ok":false,"badBits":1,"cusTested":256,"cusVerified":255}})j");
  EXPECT_EQ(failed.path("probe.ldsVerifiedCUs").as_int(0), static_cast<int64_t>(255));
  Json none_st = view(R"({"passed":true})");
  EXPECT_TRUE(!none_st["probe"].contains("ldsVerifiedCUs"));
}
