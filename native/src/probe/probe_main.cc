// mi355x-probe CLI: `mi355x-probe [--device N|--all] [--hbm-bytes B] [--gemm-n N] [--no-mfma]
// [--low-precision fp8,mxfp8,mxfp4] [--host-link-bytes N] [--lds-check] [--register-check] [--alu-check] [--atomics-check] [--list]`. Prints one JSON object per probed device and exits 0 iff every probe passed.
// Equivalent of the reference's in-pod `nvidia-smi` smoke check (GPU调度平台搭建.md:134-138),
// but it exercises HBM and the matrix cores instead of only enumerating the device.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "mi355x/probe.h"

int main(int argc, char** argv) {
  long long hbm = 1LL << 30;
  int gemm_n = 4096;
  bool mfma = true, all = true, list = false;
  int device = -1;
  int lowp_mask = 0;  // "mfmaLowPrecision": bit 0 fp8, 1 mxfp8, 2 mxfp4
  long long host_link = 0;  // "hostLinkBytes": the PCIe host-link phase (0 = off)
  // the opt-in per-CU phases: the flag, the library's option, whether the flag was given
  struct {
    const char* flag;
    const char* option;
    bool on;
  } checks[] = {{"--lds-check", "ldsCheck", false},       // the per-CU LDS phase
                {"--register-check", "regCheck", false},  // the per-SIMD register-file phase
                {"--alu-check", "aluCheck", false},       // the per-SIMD vector-ALU phase
                {"--atomics-check", "atomCheck", false}}; // the atomic-unit phase
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "missing value for %s\n", a.c_str());
        std::exit(2);
      }
      return argv[++i];
    };
    const auto check = std::find_if(std::begin(checks), std::end(checks), [&](const auto& c) { return a == c.flag; });
    if (check != std::end(checks)) {
      check->on = true;
    } else if (a == "--device") {
      device = std::atoi(next());
      all = false;
    } else if (a == "--all") {
      all = true;
    } else if (a == "--hbm-bytes") {
      hbm = std::atoll(next());
    } else if (a == "--gemm-n") {
      gemm_n = std::atoi(next());
    } else if (a == "--no-mfma") {
      mfma = false;
    } else if (a == "--low-precision") {
      std::string v = next();
      for (size_t p = 0; p <= v.size();) {
        const size_t q = std::min(v.find(',', p), v.size());
        const std::string d = v.substr(p, q - p);
        if (d == "fp8") lowp_mask |= 1;
        else if (d == "mxfp8") lowp_mask |= 2;
        else if (d == "mxfp4") lowp_mask |= 4;
        else {
          std::fprintf(stderr, "unknown low-precision dtype '%s' (fp8, mxfp8, mxfp4)\n", d.c_str());
          return 2;
        }
        p = q + 1;
      }
    } else if (a == "--host-link-bytes") {
      host_link = std::atoll(next());
    } else if (a == "--list") {
      list = true;
    } else if (a == "-h" || a == "--help") {
      std::printf("usage: mi355x-probe [--device N|--all] [--hbm-bytes B] [--gemm-n N] [--no-mfma] [--low-precision fp8,mxfp8,mxfp4] [--host-link-bytes N] [--lds-check] [--register-check] [--alu-check] [--atomics-check] [--list]\n");
      return 0;
    } else {
      std::fprintf(stderr, "unknown argument %s\n", a.c_str());
      return 2;
    }
  }
  char err[256] = {0};
  int n = mi355x_probe_init(err, sizeof err);
  if (n < 0) {
    std::fprintf(stderr, "probe init failed: %s\n", err);
    return 3;
  }
  if (n == 0) {
    std::fprintf(stderr, "no HIP devices visible\n");
    return 3;
  }
  std::vector<int> devs;
  if (all) {
    for (int d = 0; d < n; ++d) devs.push_back(d);
  } else {
    if (device < 0 || device >= n) {
      std::fprintf(stderr, "device %d out of range [0,%d)\n", device, n);
      return 2;
    }
    devs.push_back(device);
  }
  if (list) {
    for (int d : devs) {
      char* s = mi355x_probe_identify(d);
      std::printf("%s\n", s);
      mi355x_probe_free(s);
    }
    return 0;
  }
  // optional keys only when asked for: the plain command line sends the options it always sent
  std::string opts_s = "{\"hbmBytes\":" + std::to_string(hbm) + ",\"mfma\":" + (mfma ? "true" : "false") +
                       ",\"gemmN\":" + std::to_string(gemm_n);
  if (lowp_mask) opts_s += ",\"mfmaLowPrecision\":" + std::to_string(lowp_mask);
  if (host_link > 0) opts_s += ",\"hostLinkBytes\":" + std::to_string(host_link);
  for (const auto& c : checks)
    if (c.on) opts_s += std::string(",\"") + c.option + "\":1";
  opts_s += "}";
  const char* opts = opts_s.c_str();
  std::vector<std::string> results(devs.size());
  std::vector<std::thread> ths;
  for (size_t i = 0; i < devs.size(); ++i) {
    ths.emplace_back([&, i] {
      char* s = mi355x_probe_run(devs[i], opts);
      results[i] = s;
      mi355x_probe_free(s);
    });
  }
  for (auto& t : ths) t.join();
  int rc = 0;
  for (const auto& r : results) {
    std::printf("%s\n", r.c_str());
    if (r.find("\"passed\":true") == std::string::npos) rc = 1;
  }
  return rc;
}
