// The probe's report text (native/src/probe/report.h), block by block and byte for byte: key order,
// "%.6g" numbers and the null of an absent firstBadOffset are what the agent and the tests parse.
#include <string>
#include <vector>

#include "../src/probe/report.h"
#include "testing.h"

using S = std::string;

static HbmResult passes(unsigned long long bad, unsigned long long first, int patterns = 2) {
  HbmResult r;
  r.bad_bits = bad;
  r.first_bad = first;
  r.write_ms = 0.5f;
  r.read_ms = 0.25f;
  r.n16 = 65536;
  r.patterns = patterns;
  return r;
}

static const char* kHbmOk =
    R"({"ok":true,"bytes":1048576,"patterns":2,"badBits":0,"firstBadOffset":null,"writeGBps":4.1943,"readGBps":8.38861,"GBps":5.59241,"ms":0.75})";
static const char* kMfma =
    R"({"ok":true,"enabled":true,"n":256,"tile":256,"pipe":2,"elementMismatches":0,"abftMismatches":0,"tflops":1.5,"ms":0.25})";
static const char* kCus =
    R"({"expected":256,"mfmaVerified":256,"perXcd":[32,32,32,32,32,32,32,32],"gemmTiles":1,"badWaves":0,"ok":true})";
static const char* kPhases =
    R"({"arenaReused":true,"setupMs":0.125,"allocMs":0.25,"launchMs":0.5,"hbmFirst":1,"hbmWallMs":1.5,"mfmaWallMs":1.75,"freeMs":0})";

TEST(probe_report_numbers_and_strings) {
  EXPECT_EQ(jnum(0), S("0"));
  EXPECT_EQ(jnum(1234567.0), S("1.23457e+06"));
  EXPECT_EQ(jnum(0.1), S("0.1"));
  EXPECT_EQ(jstr("a\"b\\c\n"), S(R"("a\"b\\c")"));  // quotes and backslashes escaped, control characters dropped
}

TEST(probe_report_hbm_block) {
  EXPECT_EQ(hbm_block(passes(0, ~0ull)), S(kHbmOk));
  EXPECT_EQ(hbm_block(passes(3, 5)),
            S(R"({"ok":false,"bytes":1048576,"patterns":2,"badBits":3,"firstBadOffset":80,"writeGBps":4.1943,"readGBps":8.38861,"GBps":5.59241,"ms":0.75})"));
}

static MfmaResult mfma() {
  MfmaResult m;
  m.enabled = true;
  m.n = 256;
  m.pipe = 2;
  m.tflops = 1.5;
  m.ms = 0.25;
  return m;
}

static CusResult cus() {
  CusResult c;
  c.expected = c.verified = 256;
  for (int& x : c.per_xcd) x = 32;
  c.gemm_tiles = 1;
  return c;
}

TEST(probe_report_mfma_and_cus_blocks) {
  EXPECT_EQ(mfma_block(mfma()), S(kMfma));
  MfmaResult off;
  off.n = 4096;
  EXPECT_EQ(mfma_block(off),
            S(R"({"ok":true,"enabled":false,"n":4096,"tile":256,"pipe":0,"elementMismatches":0,"abftMismatches":0,"tflops":0,"ms":0})"));
  EXPECT_EQ(cus_block(cus()), S(kCus));
  CusResult keys = cus();
  keys.want_keys = true;
  keys.keys = {0, 1, 257};
  EXPECT_EQ(cus_block(keys),
            S(R"({"expected":256,"mfmaVerified":256,"perXcd":[32,32,32,32,32,32,32,32],"gemmTiles":1,"badWaves":0,"ok":true,"cuKeys":[0,1,257]})"));
  CusResult missing = cus();
  missing.verified = 255;
  missing.per_xcd[7] = 31;
  missing.bad_waves = 2;
  EXPECT_EQ(cus_block(missing),
            S(R"({"expected":256,"mfmaVerified":255,"perXcd":[32,32,32,32,32,32,32,31],"gemmTiles":1,"badWaves":2,"ok":false})"));
}

static LowpResult lowp_entry(const char* name) {
  LowpResult r;
  r.name = name;
  r.n = 256;
  r.ms = 0.5f;
  r.verified = 256;
  return r;
}

TEST(probe_report_low_precision_block) {
  const S fp8 = R"("fp8":{"ok":true,"n":256,"elementMismatches":0,"abftMismatches":0,"tflops":0.0671089,"ms":0.5,"cusVerified":256,"badWaves":0})";
  EXPECT_EQ(lowp_block({lowp_entry("fp8")}), "{" + fp8 + "}");
  LowpResult bad = lowp_entry("mxfp8");
  bad.ok = false;
  bad.abft_bad = 2;
  const S mxfp8 = R"("mxfp8":{"ok":false,"n":256,"elementMismatches":0,"abftMismatches":2,"tflops":0.0671089,"ms":0.5,"cusVerified":256,"badWaves":0})";
  const S mxfp4 = R"("mxfp4":{"ok":true,"n":256,"elementMismatches":0,"abftMismatches":0,"tflops":0.0671089,"ms":0.5,"cusVerified":256,"badWaves":0})";
  EXPECT_EQ(lowp_block({lowp_entry("fp8"), bad, lowp_entry("mxfp4")}), "{" + fp8 + "," + mxfp8 + "," + mxfp4 + "}");
}

TEST(probe_report_host_link_block) {
  HostLinkResult r;
  r.passes = passes(0, ~0ull);
  r.seed = 7;
  r.samples = 1026;
  r.alloc_ms = 1.5;
  EXPECT_EQ(host_link_block(r),
            S(R"({"ok":true,"bytes":1048576,"patterns":2,"seed":7,"badBits":0,"firstBadOffset":null,"hostSamples":1026,"hostSampleMismatches":0,"writeGBps":4.1943,"readGBps":8.38861,"GBps":4.1943,"ms":0.75,"allocMs":1.5})"));
  r.sample_bad = 1;  // the link's verify passed but host memory holds something else
  EXPECT_TRUE(!r.ok());
  HostLinkResult pre;  // a preload: no write pass, one pattern, no host sample
  pre.passes = passes(1, 9, 1);
  pre.passes.write_ms = 0.125f;
  pre.seed = 7;
  pre.preload = true;
  EXPECT_EQ(host_link_block(pre),
            S(R"({"ok":false,"bytes":1048576,"patterns":1,"seed":7,"badBits":1,"firstBadOffset":144,"hostSamples":0,"hostSampleMismatches":0,"writeGBps":0,"readGBps":4.1943,"GBps":4.1943,"ms":0.25,"allocMs":0})"));
}

static PhaseTimes phases() {
  PhaseTimes t;
  t.arena_reused = true;
  t.setup_ms = 0.125;
  t.alloc_ms = 0.25;
  t.launch_ms = 0.5;
  t.hbm_wall_ms = 1.5;
  t.mfma_wall_ms = 1.75;
  return t;
}

TEST(probe_report_whole_probe) {
  EXPECT_EQ(phases_block(phases()), S(kPhases));
  ProbeReport r;
  r.uuid = "GPU-ab";
  r.arch = "gfx950";
  r.hbm = passes(0, ~0ull);
  r.mfma = mfma();
  r.cus = cus();
  r.total_ms = 2.5;
  r.phases = phases();
  const S head = R"({"device":0,"hipUUID":"GPU-ab","gcnArch":"gfx950","passed":true,"hbm":)";
  EXPECT_EQ(probe_report_open(r), head + kHbmOk + ",\"mfma\":" + kMfma + ",\"cus\":" + kCus + ",\"ms\":2.5,\"phases\":" + kPhases);
  // without the MFMA phase there is no "cus"; the opt-in blocks sit between "cus" and "ms"
  ProbeReport q = r;
  q.mfma = MfmaResult{};
  q.lowp = {lowp_entry("fp8")};
  q.has_host_link = true;
  q.host_link.passes = passes(0, ~0ull);
  q.host_link.sample_bad = 1;
  const S out = probe_report_open(q);
  EXPECT_TRUE(out.find("\"passed\":false") != S::npos);
  EXPECT_TRUE(out.find("\"cus\"") == S::npos);
  const size_t mf = out.find("\"mfma\":{"), lp = out.find(",\"lowp\":{\"fp8\""), hl = out.find(",\"hostLink\":{"),
               ms = out.find(",\"ms\":2.5,\"phases\"");
  EXPECT_TRUE(mf != S::npos && lp != S::npos && hl != S::npos && ms != S::npos);
  EXPECT_TRUE(mf < lp && lp < hl && hl < ms);
}

TEST(probe_report_error_peer_and_sweep) {
  EXPECT_EQ(error_report(device_head(3), "x \"q\""), S(R"({"device":3,"passed":false,"error":"x \"q\""})"));
  EXPECT_EQ(error_report(link_head(1, 2), "e"), S(R"({"src":1,"dst":2,"passed":false,"error":"e"})"));
  EXPECT_EQ(error_report("", "bad ring"), S(R"({"passed":false,"error":"bad ring"})"));
  PeerLink ok;
  ok.dst = 1;
  ok.bytes = 1048576;
  ok.ms = 0.5f;
  ok.seed = 0xFFFFFFFFu;
  const S a = R"({"src":0,"dst":1,"canAccessPeer":true,"passed":true,"badBits":0,"firstBadOffset":null,"bytes":1048576,"GBps":2.09715,"ms":0.5,"seed":4294967295})";
  EXPECT_EQ(peer_link_block(ok), a);
  PeerLink bad = ok;
  bad.bad_bits = 3;
  bad.first_bad = 65535;  // a chunk index: reported as its byte offset
  bad.seed = 7;
  const S c = R"({"src":0,"dst":1,"canAccessPeer":true,"passed":false,"badBits":3,"firstBadOffset":1048560,"bytes":1048576,"GBps":2.09715,"ms":0.5,"seed":7})";
  EXPECT_EQ(peer_link_block(bad), c);
  EXPECT_EQ(peer_ring_report(1048576, {ok, bad}), "{\"bytes\":1048576,\"links\":[" + a + "," + c + "],\"passed\":false}");
  PeerLink no = ok;
  no.src = 1;
  no.dst = 0;
  no.error = "hipDeviceCanAccessPeer=0";
  const S b = R"({"src":1,"dst":0,"canAccessPeer":false,"passed":false,"error":"hipDeviceCanAccessPeer=0"})";
  EXPECT_EQ(peer_link_block(no), b);
  EXPECT_EQ(peer_ring_report(1048576, {ok, ok}), "{\"bytes\":1048576,\"links\":[" + a + "," + a + "],\"passed\":true}");
  EXPECT_EQ(peer_ring_report(1048576, {ok, no}), "{\"bytes\":1048576,\"links\":[" + a + "," + b + "],\"passed\":false}");
  SweepResult s;
  s.offset = 32;
  s.bytes = 1048576;
  s.span = 2097152;
  s.ms = 0.5f;
  EXPECT_EQ(sweep_report(s),
            S(R"({"device":0,"passed":true,"offset":32,"bytes":1048576,"span":2097152,"badBits":0,"firstBadOffset":null,"GBps":8.38861,"ms":0.5,"allocMs":0})"));
  s.bad_bits = 4;
  s.first_bad = 2;
  EXPECT_EQ(sweep_report(s),
            S(R"({"device":0,"passed":false,"offset":32,"bytes":1048576,"span":2097152,"badBits":4,"firstBadOffset":64,"GBps":8.38861,"ms":0.5,"allocMs":0})"));
}
