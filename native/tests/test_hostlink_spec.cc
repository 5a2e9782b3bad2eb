// spec.probe.hostLinkCheck / hostLinkBytes / minHostLinkGBps through the manager's API layer: parse,
// the probe options sent with claims and rechecks, InvalidSpec validation and the device status.
#include <string>

#include "gpupool/api.h"
#include "gpupool/json.h"
#include "gpupool/provider.h"
#include "testing.h"

using namespace gpupool;

static Json pool(const std::string& probe) {
  return Json::parse(R"({"kind":"Mi355xPool","spec":{"replicas":1,"probe":)" + probe + "}}");
}

TEST(hostlink_spec_parse_and_probe_json) {
  auto none = Mi355xPoolSpec::from(pool("{}")["spec"]);
  EXPECT_TRUE(!none.probe_host_link_check);
  EXPECT_EQ(none.probe_host_link_bytes, static_cast<int64_t>(gen::kDefaultProbeHostLinkBytes));
  // the default claim and the recheck policy carry today's options
  for (const char* k : {"hostLinkCheck", "hostLinkBytes", "minHostLinkGBps"}) {
    EXPECT_TRUE(!none.probe_json().contains(k));
    EXPECT_TRUE(!none.policy_json()["probe"].contains(k));
  }
  EXPECT_EQ(none.probe_json().dump(), Mi355xPoolSpec::from(pool(R"({"hostLinkCheck":false,"hostLinkBytes":2097152})")["spec"])
                                          .probe_json()
                                          .dump());
  auto on = Mi355xPoolSpec::from(pool(R"({"hostLinkCheck":true,"hostLinkBytes":16777216,"minHostLinkGBps":40})")["spec"]);
  EXPECT_TRUE(on.probe_host_link_check);
  EXPECT_TRUE(on.probe_json()["hostLinkCheck"].as_bool(false));
  EXPECT_EQ(on.probe_json()["hostLinkBytes"].as_int(0), static_cast<int64_t>(16777216));
  EXPECT_EQ(on.probe_json()["minHostLinkGBps"].as_double(0), 40.0);
  EXPECT_EQ(on.policy_json().path("probe.hostLinkBytes").as_int(0), static_cast<int64_t>(16777216));
  auto dflt = Mi355xPoolSpec::from(pool(R"({"hostLinkCheck":true})")["spec"]);
  EXPECT_EQ(dflt.probe_json()["hostLinkBytes"].as_int(0), static_cast<int64_t>(gen::kDefaultProbeHostLinkBytes));
}

TEST(hostlink_spec_invalid) {
  for (const char* good : {R"({"hostLinkCheck":true})", R"({"hostLinkCheck":false,"minHostLinkGBps":0})",
                           R"({"hostLinkCheck":true,"hostLinkBytes":1048576,"minHostLinkGBps":45.5})",
                           R"({"hostLinkCheck":true,"hostLinkBytes":1073741824})", R"({"hostLinkBytes":4194304})"})
    EXPECT_TRUE(validate_mi355x(pool(good)).empty());
  for (const char* bad : {R"({"hostLinkCheck":"yes"})", R"({"hostLinkCheck":true,"hostLinkBytes":1048575})",
                          R"({"hostLinkCheck":true,"hostLinkBytes":1073741825})",
                          R"({"hostLinkCheck":true,"minHostLinkGBps":-1})", R"({"minHostLinkGBps":40})",
                          R"({"hostLinkCheck":false,"minHostLinkGBps":40})"}) {
    auto errs = validate_mi355x(pool(bad));
    EXPECT_EQ(errs.size(), 1u);
    EXPECT_TRUE(errs.size() == 1 && errs[0].find("ostLink") != std::string::npos);
  }
}

TEST(hostlink_device_status_reports_the_slower_direction) {
  auto view = [](const std::string& probe) {
    return DeviceView::from(Json::parse(R"({"uuid":"u0","state":"Claimed","healthy":true,"probe":)" + probe + "}"))
        .status_json();
  };
  Json with = view(R"({"passed":true,"hostLink":{"ok":true,"writeGBps":55.5,"readGBps":51.25,"GBps":51.25}})");
  EXPECT_EQ(with.path("probe.hostLinkGBps").as_double(0), 51.25);
  Json failed = view(R"j({"passed":false,"error":"HostLinkMismatch: 1 flipped bit(s), first at offset 0",
                         "hostLink":{"ok":false,"badBits":1,"GBps":50}})j");
  EXPECT_EQ(failed.path("probe.hostLinkGBps").as_double(0), 50.0);
  Json none = view(R"({"passed":true})");
  EXPECT_TRUE(!none["probe"].contains("hostLinkGBps"));
}
