// What the probe library keeps per device between calls: streams, events, pinned result slots and
// the cached allocations (arena, host-link buffer, peer windows, sweep buffer), and ensure_ctx(),
// which every entry point calls before it touches them.
#pragma once

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "arena.h"    // kResSlots
#include "options.h"  // kMaxPatterns, lowp::kDtypes
#include "types.h"

namespace {

struct SweepBuf {
  std::vector<void*> chunks;  // kSweepChunk bytes each, the last one possibly shorter (sweep_window.h)
  uint64_t span = 0;
  bool empty() const { return chunks.empty(); }
};

struct DeviceCtx {
  hipStream_t stream = nullptr;   // HBM pattern test
  hipStream_t stream2 = nullptr;  // MFMA checks, overlapped with the bandwidth-bound HBM test
  hipEvent_t ev[1 + 2 * kMaxPatterns] = {};
  hipEvent_t gev[3] = {};         // GEMM timing + "counters zeroed" hand-off between the streams
  hipDeviceProp_t prop{};
  unsigned long long* host_res = nullptr;
  // low-precision phase ("mfmaLowPrecision"): created by the first probe that asks for a dtype
  hipEvent_t lev[lowp::kDtypes][2] = {};
  unsigned long long* host_lowp = nullptr;
  // host-link phase ("hostLinkBytes"): created by the first probe that asks. The pinned buffer is
  // grown when a larger size is asked for, never shrunk, kept for the life of the process (trim
  // leaves it: it is host RAM, not VRAM) and only ever freed or replaced by ensure_host_link, under
  // the device's probe lock and after every stream that can use it has been synchronised.
  hipStream_t hl_stream = nullptr;  // only with "overlap"
  hipEvent_t hev[1 + 2 * kMaxPatterns] = {};
  void* hl_buf = nullptr;  // host address
  void* hl_dev = nullptr;  // the same memory as the GPU addresses it
  uint64_t hl_bytes = 0;
  bool hl_coherent = true;
  unsigned long long* hl_cnt = nullptr;  // device counter pairs, one per pass
  unsigned long long* hl_res = nullptr;  // their pinned copy
  // LDS phase ("ldsCheck"): created by the first probe that asks. Two sets of device counters: the
  // kernel of one run counts into set lds_set and resets the other for the next run (lds.h).
  hipEvent_t lds_ev[2] = {};
  unsigned long long* lds_cnt = nullptr;  // device, 2 sets
  unsigned long long* lds_res = nullptr;  // pinned copy of the set a run used
  int lds_set = 0;
  bool lds_clean = false;    // both sets hold their reset values
  uint32_t lds_runs = 0;     // the default "ldsSalt"
  void* lds_dump = nullptr;  // device copy of workgroup 0's LDS (mi355x_probe_lds with an image)
  // register-file phase ("regCheck"): as the LDS phase's. regs_attr[i] is what the runtime says of
  // rf_march<i>: registers per lane and workgroups per CU, asked once (0: not yet).
  hipEvent_t regs_ev[2] = {};
  unsigned long long* regs_cnt = nullptr;  // device, 2 sets
  unsigned long long* regs_res = nullptr;  // pinned copy of the set a run used
  int regs_set = 0;
  bool regs_clean = false;
  uint32_t regs_runs = 0;     // the default "regsSalt"
  void* regs_dump = nullptr;  // device image uint32[4][512][64] (mi355x_probe_regs with an image)
  int regs_attr[2][2] = {};
  // vector-ALU phase ("aluCheck"): events, counter sets and pinned result as the LDS phase's.
  // alu_exp holds the host's expectation uint32[5][64] of (alu_exp_seed, alu_exp_iters), computed
  // and uploaded once per context and pair; alu_exp1 the one of the dump's stage 1 (one step).
  hipEvent_t alu_ev[2] = {};
  unsigned long long* alu_cnt = nullptr;  // device, 2 sets
  unsigned long long* alu_res = nullptr;  // pinned copy of the set a run used
  int alu_set = 0;
  bool alu_clean = false;
  uint32_t* alu_exp = nullptr;  // device
  uint32_t alu_exp_seed = 0;
  int alu_exp_iters = 0;        // 0: nothing uploaded yet
  void* alu_dump = nullptr;     // device uint32[4][6][64] (mi355x_probe_alu with a dump buffer)
  void* alu_trace = nullptr;    // device uint32[4][64][12][64] (... with "aluDumpStage":3: the trans trace)
  // atomic-unit phase ("atomCheck"): events, counter sets and pinned result as the LDS phase's.
  // atom_mem is one allocation for atom_wgs workgroups: their private regions, the nine dev
  // row-sets and the records; made by the first probe that asks, grown for a larger grid, never
  // shrunk. atom_verify leaves every word at its op's identity, so a run needs no memset.
  // atom_exp holds the host's expectation (atomics_ref.h kExpWords) of (atom_exp_seed, atom_exp_iters).
  hipEvent_t atom_ev[3] = {};  // [2]: between the two kernels, recorded only for "atomTimeKernels"
  unsigned long long* atom_cnt = nullptr;  // device, 2 sets
  unsigned long long* atom_res = nullptr;  // pinned copy of the set a run used
  int atom_set = 0;
  bool atom_clean = false;
  uint32_t* atom_mem = nullptr;  // device
  int atom_wgs = 0;              // the grid atom_mem was sized for
  uint32_t* atom_exp = nullptr;  // device
  uint32_t atom_exp_seed = 0;
  int atom_exp_iters = 0;        // 0: nothing uploaded yet
  uint32_t* atom_dump = nullptr;  // device uint32[kDumpWords] (mi355x_probe_atomics with a dump buffer)
  // The probe arena is kept between probes (a hipMalloc of ~1.2 GiB costs ~0.25 ms, a fifth of a
  // probe) and freed by mi355x_probe_trim once idle, so a pod on the GPU gets the memory back.
  void* arena = nullptr;
  size_t arena_bytes = 0;
  std::chrono::steady_clock::time_point arena_used{};
  // HBM sweep buffer (mi355x_probe_hbm_sweep): nearly all free HBM, held only for a scrub pass
  SweepBuf sweep;
  unsigned long long* sweep_cnt = nullptr;
  // Freed VRAM is cleared by the driver before it is handed out again (~6 s for ~282 GiB measured,
  // profiles/r2h_sweep_claim_diag.txt): an arena hipMalloc issued in that window waits for it. The
  // arena is therefore allocated before the sweep buffer and not trimmed while a sweep is held or
  // for kSweepClearGrace after its release, so a claim-time probe never allocates behind a clear.
  std::chrono::steady_clock::time_point sweep_released{};
  // xGMI ring check (mi355x_probe_peer_ring): send / receive windows kept between claims like the
  // arena (a 64 MiB hipMalloc + hipFree pair per link per claim cost more than the copy), freed by
  // the same idle trim
  void* peer_send = nullptr;
  void* peer_recv = nullptr;
  uint64_t peer_bytes = 0;
  unsigned long long* peer_cnt = nullptr;
  std::chrono::steady_clock::time_point peer_used{};
  std::string uuid;  // hip_uuid(), cached: the runtime query is not free on a cold CPU
  bool ready = false;
};

constexpr std::chrono::seconds kSweepClearGrace{30};

std::mutex g_mu;
std::vector<DeviceCtx> g_ctx;
int g_count = -1;

inline std::mutex& device_mutex(int dev) {
  static std::vector<std::mutex> mu(64);
  return mu[static_cast<size_t>(dev) % mu.size()];
}

inline DeviceCtx& ctx_of(int dev) { return g_ctx[static_cast<size_t>(dev)]; }
inline bool device_ok(int dev) { return g_count >= 0 && dev >= 0 && dev < g_count; }

inline double ms_since(std::chrono::steady_clock::time_point a) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

inline std::string hip_uuid(int dev) {
  hipUUID u{};
  if (hipDeviceGetUuid(&u, dev) != hipSuccess) return "";
  std::string s(u.bytes, u.bytes + 16);
  // ROCm reports the ASIC serial as ASCII hex: "GPU-<serial>" is the ROCR_VISIBLE_DEVICES form.
  bool ascii = true;
  for (char c : s) ascii = ascii && ((c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'));
  if (ascii) return "GPU-" + s;
  char buf[40];
  std::string hex;
  for (int i = 0; i < 16; ++i) {
    std::snprintf(buf, sizeof buf, "%02x", static_cast<unsigned char>(u.bytes[i]));
    hex += buf;
  }
  return "GPU-" + hex;
}

// The device's streams, events, properties and pinned result slots, made by the first call that
// needs them. Selects the device; the caller holds its probe lock.
inline DeviceCtx& ensure_ctx(int dev) {
  PROBE_CHECK(hipSetDevice(dev));
  DeviceCtx& ctx = ctx_of(dev);
  if (ctx.ready) return ctx;
  PROBE_CHECK(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
  PROBE_CHECK(hipStreamCreateWithFlags(&ctx.stream2, hipStreamNonBlocking));
  for (auto& e : ctx.ev) PROBE_CHECK(hipEventCreate(&e));
  for (auto& e : ctx.gev) PROBE_CHECK(hipEventCreate(&e));
  PROBE_CHECK(hipGetDeviceProperties(&ctx.prop, dev));
  // pinned result slots: device->host copies of the counters are truly async (one sync per phase)
  PROBE_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ctx.host_res), kResSlots * sizeof(unsigned long long)));
  ctx.uuid = hip_uuid(dev);
  ctx.ready = true;
  return ctx;
}

}  // namespace
