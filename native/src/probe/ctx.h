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

// The counters of one opt-in per-CU phase (lds.h, regfile.h, alu.h, atomics.h): two sets on the
// device, a pinned copy of the set a run used, and the two events around the run's kernels.
//
// The kernel of a run counts into one set with atomics and its workgroup 0 resets the OTHER set for
// the next run with plain stores: a reset of the set in use would race with the atomics of
// workgroups on other XCDs (their L2s are not coherent inside one kernel), and the end of the kernel
// is what makes the plain stores visible to the next run's atomics. So run() hands the kernel
// ``set`` to count into and ``set ^ 1`` to reset, end() flips ``set``, and ``clean`` says that both
// sets hold their reset values: false from run() until end() has seen the run finish, so a run that
// threw before end() is recovered from by the next reset().
struct CounterSets {
  hipEvent_t ev[2] = {};
  unsigned long long* cnt = nullptr;  // device, 2 sets
  unsigned long long* res = nullptr;  // pinned copy of the set a run used
  int set = 0;
  bool clean = false;  // both sets hold their reset values

  // The events, the two sets of ``slots`` counters and the pinned copy, on first use.
  void make(int slots) {
    if (res) return;  // set last: a failure half way is picked up by the next probe that asks
    for (auto& e : ev)
      if (!e) PROBE_CHECK(hipEventCreate(&e));
    if (!cnt) PROBE_CHECK(hipMalloc(reinterpret_cast<void**>(&cnt), 2 * slots * sizeof(unsigned long long)));
    PROBE_CHECK(hipHostMalloc(reinterpret_cast<void**>(&res), slots * sizeof(unsigned long long)));
    clean = false;
  }

  // Both sets to the phase's reset_value(slot), set 0 the next to count into. For sets that are not
  // clean (first use, or a run that never reached end()); the caller has synchronised every stream
  // a run may be on. ``also``: what else the phase puts right before the sets count as clean.
  template <int kSlots, class Reset, class Also>
  void reset(Reset reset_value, Also&& also) {
    unsigned long long init[2 * kSlots];
    for (int i = 0; i < 2 * kSlots; ++i) init[i] = reset_value(i % kSlots);
    PROBE_CHECK(hipMemcpy(cnt, init, sizeof init, hipMemcpyHostToDevice));
    also();
    set = 0;
    clean = true;
  }
  template <int kSlots, class Reset>
  void reset(Reset reset_value) {
    reset<kSlots>(reset_value, [] {});
  }

  // Enqueues a run on stream s: an event, ``kernels(cnt, next)`` (the set to count into and the one
  // to reset), an event, the copy of the run's set to ``res``. No host synchronise.
  template <class Kernels>
  void run(hipStream_t s, int slots, Kernels&& kernels) {
    unsigned long long* mine = cnt + set * slots;
    clean = false;  // until end() has seen this run end
    PROBE_CHECK(hipEventRecord(ev[0], s));
    kernels(mine, cnt + (set ^ 1) * slots);
    PROBE_CHECK(hipEventRecord(ev[1], s));
    PROBE_CHECK(hipGetLastError());
    PROBE_CHECK(hipMemcpyAsync(res, mine, slots * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  }

  // After the stream's synchronise: the run's time between the events; the next run takes the other
  // set, which this run's kernel reset.
  float end() {
    float ms = 0;
    PROBE_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    set ^= 1;
    clean = true;
    return ms;
  }
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
  // The opt-in per-CU phases, each made by the first probe that asks: its counter sets (above) and
  // what else it keeps between runs.
  struct {  // "ldsCheck" (lds.h)
    CounterSets sets;
    uint32_t runs = 0;     // the default "ldsSalt"
    void* dump = nullptr;  // device copy of workgroup 0's LDS (mi355x_probe_lds with an image)
  } lds;
  // regs.attr[i] is what the runtime says of rf_march<i>: registers per lane and workgroups per CU,
  // asked once (0: not yet).
  struct {  // "regCheck" (regfile.h)
    CounterSets sets;
    uint32_t runs = 0;     // the default "regsSalt"
    void* dump = nullptr;  // device image uint32[4][512][64] (mi355x_probe_regs with an image)
    int attr[2][2] = {};
  } regs;
  // alu.exp holds the host's expectation uint32[5][64] of (exp_seed, exp_iters), computed and
  // uploaded once per context and pair.
  struct {  // "aluCheck" (alu.h)
    CounterSets sets;
    uint32_t* exp = nullptr;  // device
    uint32_t exp_seed = 0;
    int exp_iters = 0;        // 0: nothing uploaded yet
    void* dump = nullptr;     // device uint32[4][6][64] (mi355x_probe_alu with a dump buffer)
    void* trace = nullptr;    // device uint32[4][64][12][64] (... with "aluDumpStage":3: the trans trace)
  } alu;
  // atom.mem is one allocation for atom.wgs workgroups: their private regions, the nine dev row-sets
  // and the records; made by the first probe that asks, grown for a larger grid, never shrunk.
  // atom_verify leaves every word at its op's identity, so a run needs no memset. atom.exp holds
  // the host's expectation (atomics_ref.h kExpWords) of (exp_seed, exp_iters).
  struct {  // "atomCheck" (atomics.h)
    CounterSets sets;
    hipEvent_t ev_mid = nullptr;  // between the two kernels, recorded only for "atomTimeKernels"
    uint32_t* mem = nullptr;      // device
    int wgs = 0;                  // the grid mem was sized for
    uint32_t* exp = nullptr;      // device
    uint32_t exp_seed = 0;
    int exp_iters = 0;            // 0: nothing uploaded yet
    uint32_t* dump = nullptr;     // device uint32[kDumpWords] (mi355x_probe_atomics with a dump buffer)
  } atom;
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

// What a phase does before it resets its counter sets or replaces a buffer a run may still use.
inline void sync_streams(DeviceCtx& c) {
  PROBE_CHECK(hipStreamSynchronize(c.stream));
  PROBE_CHECK(hipStreamSynchronize(c.stream2));
}

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
