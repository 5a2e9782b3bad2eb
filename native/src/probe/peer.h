// The xGMI checks (mi355x_probe_peer, mi355x_probe_peer_ring): a pattern written on the source,
// copied over the peer link, every bit verified on the destination. Callers hold the probe lock of
// every device involved.
#pragma once

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "ctx.h"
#include "hbm.h"
#include "options.h"
#include "report.h"

namespace {

// src may reach dst's memory; false: the link has no peer access.
inline bool enable_peer(int src, int dst) {
  int can = 0;
  PROBE_CHECK(hipDeviceCanAccessPeer(&can, src, dst));
  if (!can) return false;
  PROBE_CHECK(hipSetDevice(src));
  hipError_t e = hipDeviceEnablePeerAccess(dst, 0);
  if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) PROBE_CHECK(e);
  (void)hipGetLastError();  // clear a sticky "already enabled"
  return true;
}

// The two halves of a link's pattern pass: the source fills on its stream, the receiver verifies
// what arrived into ``cnt`` (reset by memsets) and copies the pair to its result slots.
inline PatternPass peer_pass(DeviceCtx& c, void* buf, uint64_t n16, uint32_t seed) {
  PatternPass p;
  p.s = c.stream;
  p.buf = static_cast<u32x4*>(buf);
  p.n16 = n16;
  p.seed = seed;
  p.fill_grid = hbm_grid(c.prop.multiProcessorCount, kHbmFillBlocksPerCU, n16);
  p.verify_grid = hbm_grid(c.prop.multiProcessorCount, kHbmVerifyBlocksPerCU, n16);
  return p;
}

// ``hooks``: the test hooks that strike this link's receiving window, on the receiver's stream
// behind the copy (the host has waited for it) and ahead of the verify; null: none.
inline void peer_verify(DeviceCtx& cd, const PatternPass& pass, unsigned long long* cnt, const PeerOptions* hooks = nullptr) {
  memset_pairs(cd.stream, cnt, 1, 1);
  if (hooks && hooks->inject_flips > 0) pass.inject_flips(hooks->inject_flips);
  if (hooks && hooks->flip_chunk(pass.n16) >= 0) pass.inject_flip_at(static_cast<uint64_t>(hooks->flip_chunk(pass.n16)));
  pass.verify(0, cnt);
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipMemcpyAsync(cd.host_res, cnt, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, cd.stream));
}

// The nonce of one run_peer / run_peer_ring call (options.h peer_call_seed): no two calls of a
// process verify against the same pattern, so what an earlier call left in a window never passes.
inline uint32_t next_peer_nonce() {
  static std::atomic<uint32_t> calls{0};
  return calls.fetch_add(1) + 1;
}

// One direction of the xGMI peer check (see mi355x_probe_peer in probe.h). ``io``: the first
// min(io_bytes, tested bytes) of what the destination holds after the verify (mi355x_probe_peer_dump).
inline std::string run_peer(int src, int dst, const char* opts, void* io = nullptr, size_t io_bytes = 0) {
  const PeerOptions o = PeerOptions::parse(opts, 256LL << 20);
  const uint64_t n16 = o.bytes / 16;
  DeviceCtx& cs = ensure_ctx(src);
  DeviceCtx& cd = ensure_ctx(dst);
  PeerLink link;
  link.src = src;
  link.dst = dst;
  link.bytes = n16 * 16;
  if (src != dst && !enable_peer(src, dst)) {
    link.error = "hipDeviceCanAccessPeer=0";
    return peer_link_block(link);
  }
  DevBuf sbuf, dbuf, cnt_buf;
  PROBE_CHECK(hipSetDevice(src));
  PROBE_CHECK(hipMalloc(&sbuf.p, n16 * 16));
  PROBE_CHECK(hipSetDevice(dst));
  PROBE_CHECK(hipMalloc(&dbuf.p, n16 * 16));
  PROBE_CHECK(hipMalloc(&cnt_buf.p, 2 * sizeof(unsigned long long)));
  const uint32_t seed = link.seed = peer_call_seed(0x5EED0000u + static_cast<uint32_t>(src * 16 + dst), next_peer_nonce());
  // src: write the pattern
  PROBE_CHECK(hipSetDevice(src));
  peer_pass(cs, sbuf.p, n16, seed).fill(0);
  PROBE_CHECK(hipGetLastError());
  // the copy over the peer link, timed on src's stream
  PROBE_CHECK(hipEventRecord(cs.gev[0], cs.stream));
  if (!o.skip_copy) PROBE_CHECK(hipMemcpyPeerAsync(dbuf.p, dst, sbuf.p, src, n16 * 16, cs.stream));
  PROBE_CHECK(hipEventRecord(cs.gev[1], cs.stream));
  PROBE_CHECK(hipStreamSynchronize(cs.stream));
  PROBE_CHECK(hipEventElapsedTime(&link.ms, cs.gev[0], cs.gev[1]));
  // dst: verify every bit that arrived
  PROBE_CHECK(hipSetDevice(dst));
  peer_verify(cd, peer_pass(cd, dbuf.p, n16, seed), static_cast<unsigned long long*>(cnt_buf.p), &o);
  PROBE_CHECK(hipStreamSynchronize(cd.stream));
  link.bad_bits = cd.host_res[0];
  link.first_bad = cd.host_res[1];
  if (io && io_bytes) PROBE_CHECK(hipMemcpy(io, dbuf.p, std::min<uint64_t>(io_bytes, n16 * 16), hipMemcpyDeviceToHost));
  return peer_link_block(link);
}

// Cached peer windows of one device (caller holds its lock, device selected).
inline void ensure_peer_bufs(DeviceCtx& c, uint64_t bytes) {
  if (c.peer_bytes != bytes) {
    if (c.peer_send) (void)hipFree(c.peer_send);
    if (c.peer_recv) (void)hipFree(c.peer_recv);
    c.peer_send = c.peer_recv = nullptr;
    c.peer_bytes = 0;
    PROBE_CHECK(hipMalloc(&c.peer_send, bytes));
    PROBE_CHECK(hipMalloc(&c.peer_recv, bytes));
    c.peer_bytes = bytes;
  }
  if (!c.peer_cnt) PROBE_CHECK(hipMalloc(&c.peer_cnt, 2 * sizeof(unsigned long long)));
}

inline void free_peer_bufs(DeviceCtx& c) {
  if (c.peer_send) (void)hipFree(c.peer_send);
  if (c.peer_recv) (void)hipFree(c.peer_recv);
  c.peer_send = c.peer_recv = nullptr;
  c.peer_bytes = 0;
}

inline std::vector<int> distinct(std::vector<int> devs) {
  std::sort(devs.begin(), devs.end());
  devs.erase(std::unique(devs.begin(), devs.end()), devs.end());
  return devs;
}

inline void sync_streams(const std::vector<int>& devs) {
  for (int d : devs) {
    PROBE_CHECK(hipSetDevice(d));
    PROBE_CHECK(hipStreamSynchronize(ctx_of(d).stream));
  }
}

inline uint32_t ring_seed(int dev) { return 0x5EED0000u + static_cast<uint32_t>(dev) * 0x9E37u; }

// Ring step 2: all links at once, each timed on its source's stream. A source with two outgoing
// links (only with repeated devices) times them back to back on its one stream.
inline void ring_copy(const std::vector<int>& uniq, uint64_t bytes, std::vector<PeerLink>& links, bool skip_copy) {
  const size_t n = links.size();
  std::vector<hipEvent_t> t0(n, nullptr), t1(n, nullptr);
  struct EvGuard {
    std::vector<hipEvent_t>& a;
    std::vector<hipEvent_t>& b;
    ~EvGuard() {
      for (auto* v : {&a, &b})
        for (hipEvent_t e : *v)
          if (e) (void)hipEventDestroy(e);
    }
  } guard{t0, t1};
  for (size_t i = 0; i < n; ++i) {
    if (!links[i].error.empty()) continue;
    DeviceCtx& cs = ctx_of(links[i].src);
    PROBE_CHECK(hipSetDevice(links[i].src));
    PROBE_CHECK(hipEventCreate(&t0[i]));
    PROBE_CHECK(hipEventCreate(&t1[i]));
    PROBE_CHECK(hipEventRecord(t0[i], cs.stream));
    if (!skip_copy)
      PROBE_CHECK(hipMemcpyPeerAsync(ctx_of(links[i].dst).peer_recv, links[i].dst, cs.peer_send, links[i].src, bytes, cs.stream));
    PROBE_CHECK(hipEventRecord(t1[i], cs.stream));
  }
  sync_streams(uniq);
  for (size_t i = 0; i < n; ++i) {
    if (!links[i].error.empty()) continue;
    PROBE_CHECK(hipSetDevice(links[i].src));
    PROBE_CHECK(hipEventElapsedTime(&links[i].ms, t0[i], t1[i]));
  }
}

// Ring step 3: every receiving link verifies what arrived. The receivers of a batch of consecutive
// links are distinct devices (each has one counter pair and one result slot), so the batch's
// verifies run concurrently, one per receiver, and the host waits once per receiver; a receiver
// named again (only with repeated devices, e.g. [0, 0] on a 1-GPU box) starts the next batch and is
// verified against that link's source pattern in turn. The test hooks strike link "injectLink".
inline void ring_verify(uint64_t n16, std::vector<PeerLink>& links, const PeerOptions& o) {
  const size_t n = links.size();
  for (size_t i = 0; i < n;) {
    std::vector<size_t> batch;
    std::vector<int> used;
    for (; i < n; ++i) {
      if (links[i].error.empty()) {
        if (std::find(used.begin(), used.end(), links[i].dst) != used.end()) break;
        used.push_back(links[i].dst);
      }
      batch.push_back(i);
    }
    for (size_t j : batch) {
      if (!links[j].error.empty()) continue;
      DeviceCtx& cd = ctx_of(links[j].dst);
      PROBE_CHECK(hipSetDevice(links[j].dst));
      peer_verify(cd, peer_pass(cd, cd.peer_recv, n16, links[j].seed), cd.peer_cnt,
                  j == static_cast<size_t>(o.inject_link) ? &o : nullptr);
    }
    for (size_t j : batch) {
      if (!links[j].error.empty()) continue;
      DeviceCtx& cd = ctx_of(links[j].dst);
      PROBE_CHECK(hipSetDevice(links[j].dst));
      PROBE_CHECK(hipStreamSynchronize(cd.stream));
      links[j].bad_bits = cd.host_res[0];
      links[j].first_bad = cd.host_res[1];
    }
  }
}

// The whole xGMI ring at once (see mi355x_probe_peer_ring in probe.h): link i copies devs[i]'s send
// window into devs[i+1]'s receive window. On an MI355X node every GPU pair has its own xGMI link, so
// the n copies of a ring use n distinct links and run concurrently, one per source stream: the check
// costs one copy time instead of n (a pair-at-a-time check also serialised pairs sharing a device).
// Phases: every source fills its window (one pattern per source device and call), every link copies, the host
// waits for all copies, every receiver verifies the bits that arrived. A device may appear more than
// once (a 1-GPU box runs [0, 0]: local copies through the same code).
inline std::string run_peer_ring(const std::vector<int>& devs, const char* opts) {
  const PeerOptions o = PeerOptions::parse(opts, 64LL << 20);
  const uint64_t bytes = o.bytes / 16 * 16;
  const uint64_t n16 = bytes / 16;
  const uint32_t nonce = next_peer_nonce();
  const size_t n = devs.size();
  const std::vector<int> uniq = distinct(devs);
  for (int d : uniq) {
    DeviceCtx& c = ensure_ctx(d);
    ensure_peer_bufs(c, bytes);
    c.peer_used = std::chrono::steady_clock::now();
  }
  std::vector<PeerLink> links(n);
  for (size_t i = 0; i < n; ++i) {  // peer access for every link (idempotent)
    links[i].src = devs[i];
    links[i].dst = devs[(i + 1) % n];
    links[i].bytes = bytes;
    links[i].seed = peer_call_seed(ring_seed(links[i].src), nonce);
    if (links[i].src != links[i].dst && !enable_peer(links[i].src, links[i].dst)) links[i].error = "hipDeviceCanAccessPeer=0";
  }
  for (int d : uniq) {  // 1. each source device writes its pattern once, all devices at once
    DeviceCtx& c = ctx_of(d);
    PROBE_CHECK(hipSetDevice(d));
    peer_pass(c, c.peer_send, n16, peer_call_seed(ring_seed(d), nonce)).fill(0);
    PROBE_CHECK(hipGetLastError());
  }
  sync_streams(uniq);  // the copies below read other devices' windows: every fill must be done
  ring_copy(uniq, bytes, links, o.skip_copy);
  ring_verify(n16, links, o);
  return peer_ring_report(bytes, links);
}

}  // namespace
