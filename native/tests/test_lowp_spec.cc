// spec.probe.mfmaLowPrecision through the manager's API layer: parse, the probe options sent with
// claims, InvalidSpec validation and the device status the pool reports.
#include <string>

#include "gpupool/api.h"
#include "gpupool/json.h"
#include "gpupool/provider.h"
#include "testing.h"

using namespace gpupool;

static Json pool(const std::string& probe) {
  return Json::parse(R"({"kind":"Mi355xPool","spec":{"replicas":1,"probe":)" + probe + "}}");
}

TEST(lowp_spec_parse_and_probe_json) {
  auto none = Mi355xPoolSpec::from(pool("{}")["spec"]);
  EXPECT_TRUE(none.probe_mfma_low_precision.empty());
  EXPECT_TRUE(!none.probe_json().contains("mfmaLowPrecision"));  // the default claim carries today's options
  auto empty = Mi355xPoolSpec::from(pool(R"({"mfmaLowPrecision":[]})")["spec"]);
  EXPECT_TRUE(!empty.probe_json().contains("mfmaLowPrecision"));
  auto two = Mi355xPoolSpec::from(pool(R"({"mfmaLowPrecision":["fp8","mxfp4"]})")["spec"]);
  EXPECT_EQ(two.probe_mfma_low_precision.size(), 2u);
  EXPECT_EQ(two.probe_mfma_low_precision[1], std::string("mxfp4"));
  EXPECT_EQ(two.probe_json()["mfmaLowPrecision"].dump(), std::string(R"(["fp8","mxfp4"])"));
  EXPECT_EQ(two.policy_json().path("probe.mfmaLowPrecision").size(), 2u);  // rechecks use the same options
}

TEST(lowp_spec_invalid) {
  for (const char* good : {R"({"mfmaLowPrecision":[]})", R"({"mfmaLowPrecision":["fp8","mxfp8","mxfp4"]})",
                           R"({"mfma":true,"mfmaLowPrecision":["mxfp4"]})", R"({"mfma":false,"mfmaLowPrecision":[]})",
                           R"({"mfma":false})"})
    EXPECT_TRUE(validate_mi355x(pool(good)).empty());
  for (const char* bad : {R"({"mfmaLowPrecision":["fp6"]})", R"({"mfmaLowPrecision":["fp8","fp8"]})",
                          R"({"mfmaLowPrecision":"fp8"})", R"({"mfmaLowPrecision":[8]})",
                          R"({"mfma":false,"mfmaLowPrecision":["fp8"]})"}) {
    auto errs = validate_mi355x(pool(bad));
    EXPECT_EQ(errs.size(), 1u);
    EXPECT_TRUE(errs[0].find("mfmaLowPrecision") != std::string::npos);
  }
}

TEST(lowp_device_status_lists_verified_dtypes) {
  auto view = [](const std::string& probe) {
    return DeviceView::from(Json::parse(R"({"uuid":"u0","state":"Claimed","healthy":true,"probe":)" + probe + "}"))
        .status_json();
  };
  Json both = view(R"({"passed":true,"lowp":{"fp8":{"ok":true},"mxfp4":{"ok":true}}})");
  EXPECT_EQ(both.path("probe.lowPrecisionVerified").dump(), std::string(R"(["fp8","mxfp4"])"));
  Json one = view(R"j({"passed":false,"error":"MFMAResultMismatch(mxfp4): 0 element / 2 ABFT mismatch(es)",
                       "lowp":{"fp8":{"ok":true},"mxfp4":{"ok":false}}})j");
  EXPECT_EQ(one.path("probe.lowPrecisionVerified").dump(), std::string(R"(["fp8"])"));
  Json none = view(R"({"passed":true})");
  EXPECT_TRUE(!none["probe"].contains("lowPrecisionVerified"));
}
