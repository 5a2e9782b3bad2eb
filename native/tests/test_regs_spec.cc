// spec.probe.registerCheck on the host side: the probe library's options ("regCheck" and the phase's
// keys), the "regs" report block byte for byte, ok under each failing condition, and the manager's API
// layer (parse, the probe options sent with claims and rechecks, InvalidSpec validation, the device status).
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
static regs::Plan plan(const S& s) { return regs::Plan::parse(s.c_str(), 0); }

static void expect_no_hooks(const regs::Plan& p) {
  EXPECT_EQ(p.flip_u, -1);
  EXPECT_EQ(p.flip_lane, -1);
  EXPECT_EQ(p.flip_bit, -1);
  EXPECT_EQ(p.fault_simd, -1);
  EXPECT_EQ(p.fault_xcc, -1);
  EXPECT_EQ(p.skip_u, -1);
  EXPECT_EQ(p.dump_stage, 0);
  EXPECT_TRUE(!p.test_kernel());
}

static void expect_off(const ProbeOptions& o) {
  const regs::Plan d;
  EXPECT_TRUE(!o.regs.on);
  EXPECT_EQ(o.regs.patterns, d.patterns);
  EXPECT_TRUE(!o.regs.salt_given);
  EXPECT_EQ(o.regs.salt, 0u);
  EXPECT_EQ(o.regs.seed, 0u);
  EXPECT_EQ(o.regs.blocks_per_cu, regs::kBlocksPerCU);
  expect_no_hooks(o.regs);
  EXPECT_EQ(o.regs_first, regs::kFirst == 1);
}

TEST(regs_options_off_looks_nothing_up) {
  expect_off(ProbeOptions::parse(nullptr));
  expect_off(parse("{}"));
  expect_off(parse(R"({"regCheck":0,"regsPatterns":3,"regsSalt":9,"regsBlocksPerCU":2,"regsFirst":0,)"
                   R"("injectRegFlip":[5,6,7],"injectRegFaultSimd":1,"injectRegFaultXcc":3,"injectRegSkip":1,"regsDumpStage":2})"));
  expect_off(parse(R"({"regCheck":false,"ldsCheck":1})"));
  EXPECT_TRUE(parse(R"({"regCheck":false,"ldsCheck":1})").lds.n16 != 0u);  // the LDS option is another option
  EXPECT_TRUE(!parse(R"({"regCheck":1})").lds.n16);
}

TEST(regs_options_defaults_and_clamps) {
  const ProbeOptions o = parse(R"({"regCheck":1})", 3);
  EXPECT_TRUE(o.regs.on);
  EXPECT_EQ(o.regs.patterns, 2);
  EXPECT_TRUE(!o.regs.salt_given);
  EXPECT_EQ(o.regs.seed, 0x52454703u);
  EXPECT_EQ(o.regs.blocks_per_cu, regs::kBlocksPerCU);
  expect_no_hooks(o.regs);
  EXPECT_EQ(o.regs_first, regs::kFirst == 1);
  EXPECT_TRUE(parse(R"({"regCheck":true})").regs.on);
  // every other option of the probe is what it is without the check
  const ProbeOptions plain = parse("{}");
  EXPECT_EQ(o.hbm_bytes, plain.hbm_bytes);
  EXPECT_EQ(o.gemm_n, plain.gemm_n);
  EXPECT_EQ(o.overlap, plain.overlap);
  EXPECT_EQ(o.host_link.n16, 0ull);
  EXPECT_EQ(o.lds.n16, 0u);

  const int pat_in[] = {0, 1, 4, 9}, pat_out[] = {1, 1, 4, 4};
  for (int i = 0; i < 4; ++i)
    EXPECT_EQ(parse("{\"regCheck\":1,\"regsPatterns\":" + std::to_string(pat_in[i]) + "}").regs.patterns, pat_out[i]);
  const int blk_in[] = {-1, 0, 1, 16, 64, 1000}, blk_out[] = {1, 1, 1, 16, 64, 64};
  for (int i = 0; i < 6; ++i)
    EXPECT_EQ(parse("{\"regCheck\":1,\"regsBlocksPerCU\":" + std::to_string(blk_in[i]) + "}").regs.blocks_per_cu, blk_out[i]);
  const ProbeOptions s = parse(R"({"regCheck":1,"regsSalt":0})");
  EXPECT_TRUE(s.regs.salt_given && s.regs.salt == 0u);
  const ProbeOptions h = parse(R"({"regCheck":1,"regsSalt":77,"regsFirst":1,"injectRegFlip":[511, 63, 31],)"
                               R"("injectRegFaultSimd":3,"injectRegFaultXcc":7,"injectRegSkip":511,"regsDumpStage":2})");
  EXPECT_TRUE(h.regs.salt_given && h.regs.salt == 77u);
  EXPECT_TRUE(h.regs_first);
  EXPECT_EQ(h.regs.flip_u, 511);
  EXPECT_EQ(h.regs.flip_lane, 63);
  EXPECT_EQ(h.regs.flip_bit, 31);
  EXPECT_EQ(h.regs.fault_simd, 3);
  EXPECT_EQ(h.regs.fault_xcc, 7);
  EXPECT_EQ(h.regs.skip_u, 511);
  EXPECT_EQ(h.regs.dump_stage, 0);  // a probe has no caller buffer to dump into
  EXPECT_TRUE(h.regs.test_kernel());
  EXPECT_TRUE(!parse(R"({"regCheck":1,"regsFirst":0})").regs_first);
  EXPECT_TRUE(parse(R"({"regCheck":1,"regsFirst":1})").regs_first);
  // the phase alone reads the stage, 1..2
  const int st_in[] = {0, 1, 2, 3, -1}, st_out[] = {0, 1, 2, 0, 0};
  for (int i = 0; i < 5; ++i) {
    const regs::Plan p = plan("{\"regsDumpStage\":" + std::to_string(st_in[i]) + "}");
    EXPECT_EQ(p.dump_stage, st_out[i]);
    EXPECT_EQ(p.test_kernel(), st_out[i] != 0);
  }
  EXPECT_TRUE(regs::Plan::parse(nullptr, 0).on);
  EXPECT_EQ(regs::kImageBytes, static_cast<size_t>(4 * 512 * 64 * 4));
}

TEST(regs_hooks_out_of_range_are_off) {
  // the flip needs all three of u < 512, lane < 64, bit < 32
  for (const char* off : {R"({"injectRegFlip":[512,0,0]})", R"({"injectRegFlip":[0,64,0]})", R"({"injectRegFlip":[0,0,32]})",
                          R"({"injectRegFlip":[-1,0,0]})", R"({"injectRegFlip":[0,-1,0]})", R"({"injectRegFlip":[0,0,-1]})",
                          R"({"injectRegFlip":[1,2]})", R"({"injectRegFlip":7})", R"({"injectRegFlip":[]})",
                          R"({"injectRegFlip":[1,,2]})"}) {
    const regs::Plan p = plan(off);
    expect_no_hooks(p);
  }
  const regs::Plan z = plan(R"({"injectRegFlip":[0,0,0]})");
  EXPECT_TRUE(z.flip_u == 0 && z.flip_lane == 0 && z.flip_bit == 0 && z.test_kernel());
  const regs::Plan sp = plan(R"({"injectRegFlip": [ 16 , 31 ,5 ]})");
  EXPECT_TRUE(sp.flip_u == 16 && sp.flip_lane == 31 && sp.flip_bit == 5);
  for (const char* off : {R"({"injectRegSkip":512})", R"({"injectRegSkip":-1})", R"({"injectRegSkip":100000})"})
    expect_no_hooks(plan(off));
  EXPECT_TRUE(plan(R"({"injectRegSkip":0})").skip_u == 0 && plan(R"({"injectRegSkip":0})").test_kernel());
  for (const char* off : {R"({"injectRegFaultSimd":4})", R"({"injectRegFaultSimd":-2})", R"({"injectRegFaultXcc":8})",
                          R"({"injectRegFaultXcc":-1})"}) {
    const regs::Plan p = plan(off);
    EXPECT_EQ(p.fault_simd, -1);
    EXPECT_EQ(p.fault_xcc, -1);
    EXPECT_TRUE(!p.test_kernel());  // a place without a flip launches the production kernel
  }
  EXPECT_EQ(plan(R"({"injectRegFaultSimd":0})").fault_simd, 0);
  EXPECT_EQ(plan(R"({"injectRegFaultXcc":0})").fault_xcc, 0);
  long long v[3] = {7, 7, 7};
  EXPECT_TRUE(!opt_ints(nullptr, "k", v, 3));
  EXPECT_TRUE(!opt_ints(R"({"k":[1,2,x]})", "k", v, 3));
  EXPECT_TRUE(opt_ints(R"({"k":[1,-2,3,4]})", "k", v, 3) && v[0] == 1 && v[1] == -2 && v[2] == 3);
}

static RegsResult clean() {
  RegsResult r;
  r.registers_per_lane = 512;
  r.workgroups_per_cu = 1;
  r.patterns = 2;
  r.salt = 5;
  r.workgroups = 1024;
  r.expected = r.tested = r.verified = 256;
  for (int& x : r.per_xcd) x = 32;
  r.ms = 0.125f;
  return r;
}

TEST(regs_block_byte_for_byte) {
  EXPECT_TRUE(clean().ok());
  EXPECT_EQ(regs_block(clean()),
            S(R"({"ok":true,"registersPerLane":512,"workgroupsPerCU":1,"patterns":2,"salt":5,"workgroups":1024,)"
              R"("cusTested":256,"cusVerified":256,"simdsTested":1024,"simdShort":0,"perXcd":[32,32,32,32,32,32,32,32],)"
              R"("badCUs":0,"badBits":0,"firstBadCU":null,"firstBadSimd":null,"firstBadRegister":null,"firstBadLane":null,)"
              R"("ms":0.125})"));
  RegsResult f = clean();
  f.verified = 255;
  f.per_xcd[3] = 31;
  f.bad_cus = 1;
  f.bad_bits = 3;
  f.first_bad = (0x365ull << 32) | (2ull << 16) | (259ull << 6) | 40ull;  // a3, lane 40, SIMD 2
  EXPECT_TRUE(!f.ok());
  EXPECT_EQ(regs_block(f),
            S(R"({"ok":false,"registersPerLane":512,"workgroupsPerCU":1,"patterns":2,"salt":5,"workgroups":1024,)"
              R"("cusTested":256,"cusVerified":255,"simdsTested":1024,"simdShort":0,"perXcd":[32,32,32,31,32,32,32,32],)"
              R"("badCUs":1,"badBits":3,"firstBadCU":869,"firstBadSimd":2,"firstBadRegister":259,"firstBadLane":40,)"
              R"("ms":0.125})"));
  RegsResult top = clean();
  top.bad_bits = 1;
  top.first_bad = (2047ull << 32) | (3ull << 16) | (511ull << 6) | 63ull;
  const S t = regs_block(top);
  EXPECT_TRUE(t.find(R"("firstBadCU":2047,"firstBadSimd":3,"firstBadRegister":511,"firstBadLane":63,)") != S::npos);
  // the phase alone, with an image: the dumped workgroup's CU and its waves' SIMDs after "ms"
  RegsResult d = clean();
  d.dump_cu = 17;
  d.dump_simds[0] = 2;
  d.dump_simds[1] = 0;
  d.dump_simds[2] = 3;
  d.dump_simds[3] = 1;
  const S out = regs_block(d);
  const S tail = R"(,"ms":0.125,"dumpCU":17,"dumpSimds":[2,0,3,1]})";
  EXPECT_TRUE(out.size() > tail.size() && out.substr(out.size() - tail.size()) == tail);
}

TEST(regs_ok_under_each_failing_condition) {
  // coverage: short of every CU fails unless "requireAllCUs" is off
  RegsResult s = clean();
  s.tested = s.verified = 250;
  EXPECT_TRUE(!s.ok());
  s.require_all = false;
  EXPECT_TRUE(s.ok());
  // a bad bit fails either way
  RegsResult b = clean();
  b.bad_bits = 1;
  EXPECT_TRUE(!b.ok());
  b.require_all = false;
  EXPECT_TRUE(!b.ok());
  // a workgroup on fewer than four SIMDs fails either way
  RegsResult h = clean();
  h.simd_short = 1;
  EXPECT_TRUE(!h.ok());
  h.require_all = false;
  EXPECT_TRUE(!h.ok());
  EXPECT_TRUE(regs_block(h).find(R"("simdShort":1,)") != S::npos);
  // a kernel that did not own its CU fails, names the error, and is never a silently weaker test
  for (int regs_per_lane : {0, 256, 504, 520})
    for (int per_cu : {1, 2}) {
      RegsResult e = clean();
      e.registers_per_lane = regs_per_lane;
      e.workgroups_per_cu = per_cu;
      e.require_all = false;
      EXPECT_TRUE(!e.exclusive() && !e.ok());
      const S out = regs_block(e);
      EXPECT_TRUE(out.find(R"("ok":false,"registersPerLane":)" + std::to_string(regs_per_lane)) != S::npos);
      EXPECT_TRUE(out.find(R"(,"ms":0.125,"error":"RegisterKernelNotExclusive"})") != S::npos);
    }
  RegsResult two = clean();
  two.workgroups_per_cu = 2;
  EXPECT_TRUE(!two.ok());
  two.workgroups_per_cu = 0;
  EXPECT_TRUE(!two.ok());
  EXPECT_TRUE(regs_block(clean()).find("error") == S::npos);
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

static LdsResult clean_lds() {
  LdsResult r;
  r.bytes_per_cu = 163840;
  r.patterns = 2;
  r.workgroups = 1024;
  r.expected = r.tested = r.verified = 256;
  return r;
}

TEST(regs_block_in_the_report_only_when_asked) {
  const ProbeReport r = plain_report();
  const S base = probe_report_open(r);
  EXPECT_TRUE(base.find("\"regs\"") == S::npos);
  // the default report, byte for byte what it was
  EXPECT_EQ(base,
            S(R"({"device":0,"hipUUID":"GPU-ab","gcnArch":"gfx950","passed":true,"hbm":{"ok":true,"bytes":1048576,"patterns":2,)"
              R"("badBits":0,"firstBadOffset":null,"writeGBps":4.1943,"readGBps":8.38861,"GBps":5.59241,"ms":0.75},)"
              R"("mfma":{"ok":true,"enabled":true,"n":256,"tile":256,"pipe":0,"elementMismatches":0,"abftMismatches":0,"tflops":0,"ms":0},)"
              R"("cus":{"expected":256,"mfmaVerified":256,"perXcd":[0,0,0,0,0,0,0,0],"gemmTiles":0,"badWaves":0,"ok":true},)"
              R"("ms":2.5,"phases":{"arenaReused":false,"setupMs":0,"allocMs":0,"launchMs":0,"hbmFirst":1,"hbmWallMs":0,"mfmaWallMs":0,"freeMs":0})"));
  ProbeReport q = r;
  q.regs = clean();  // a result without the flag reports nothing and fails nothing
  q.regs.bad_bits = 1;
  EXPECT_EQ(probe_report_open(q), base);
  q.has_regs = true;
  q.has_lds = true;
  q.lds = clean_lds();
  const S out = probe_report_open(q);
  EXPECT_TRUE(out.find("\"passed\":false") != S::npos);
  const size_t ld = out.find(",\"lds\":{\"ok\":true"), rg = out.find(",\"regs\":{\"ok\":false"),
               ms = out.find(",\"ms\":2.5,\"phases\"");
  EXPECT_TRUE(ld != S::npos && rg != S::npos && ms != S::npos);
  EXPECT_TRUE(ld < rg && rg < ms);
  q.regs.bad_bits = 0;
  EXPECT_TRUE(probe_report_open(q).find("\"passed\":true") != S::npos);
  q.regs.workgroups_per_cu = 2;  // "passed" needs the exclusivity check too
  EXPECT_TRUE(probe_report_open(q).find("\"passed\":false") != S::npos);
}

static Json pool(const S& probe) {
  return Json::parse(R"({"kind":"Mi355xPool","spec":{"replicas":1,"probe":)" + probe + "}}");
}

TEST(regs_spec_parse_validate_and_status) {
  auto none = Mi355xPoolSpec::from(pool("{}")["spec"]);
  EXPECT_TRUE(!none.probe_register_check);
  // the default claim and the recheck policy carry today's options
  EXPECT_TRUE(!none.probe_json().contains("registerCheck"));
  EXPECT_TRUE(!none.policy_json()["probe"].contains("registerCheck"));
  EXPECT_EQ(none.probe_json().dump(), Mi355xPoolSpec::from(pool(R"({"registerCheck":false})")["spec"]).probe_json().dump());
  auto on = Mi355xPoolSpec::from(pool(R"({"registerCheck":true})")["spec"]);
  EXPECT_TRUE(on.probe_register_check);
  EXPECT_TRUE(on.probe_json()["registerCheck"].as_bool(false));
  EXPECT_TRUE(on.policy_json().path("probe.registerCheck").as_bool(false));
  EXPECT_TRUE(!on.probe_json().contains("ldsCheck"));

  for (const char* good : {R"({"registerCheck":true})", R"({"registerCheck":false})", R"({"registerCheck":true,"ldsCheck":true})"})
    EXPECT_TRUE(validate_mi355x(pool(good)).empty());
  for (const char* bad : {R"({"registerCheck":"yes"})", R"({"registerCheck":1})", R"({"registerCheck":null})"}) {
    auto errs = validate_mi355x(pool(bad));
    EXPECT_EQ(errs.size(), 1u);
    EXPECT_TRUE(errs.size() == 1 && errs[0].find("spec.probe.registerCheck") != S::npos);
  }

  auto view = [](const S& probe) {
    return DeviceView::from(Json::parse(R"({"uuid":"u0","state":"Claimed","healthy":true,"probe":)" + probe + "}"))
        .status_json();
  };
  Json with = view(R"({"passed":true,"regs":{"ok":true,"cusTested":256,"cusVerified":256}})");
  EXPECT_EQ(with.path("probe.regsVerifiedCUs").as_int(0), static_cast<int64_t>(256));
  EXPECT_TRUE(!with["probe"].contains("ldsVerifiedCUs"));
  Json failed = view(R"j({"passed":false,"error":"RegisterFileMismatch: 1 flipped bit(s) on 1 CU(s), first on CU 0/0/0/0 SIMD 0 register v17 lane 0",
                         "regs":{"ok":false,"badBits":1,"cusTested":256,"cusVerified":255}})j");
  EXPECT_EQ(failed.path("probe.regsVerifiedCUs").as_int(0), static_cast<int64_t>(255));
  Json none_st = view(R"({"passed":true})");
  EXPECT_TRUE(!none_st["probe"].contains("regsVerifiedCUs"));
}
