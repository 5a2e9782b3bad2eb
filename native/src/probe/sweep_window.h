// One window of the rotating HBM sweep, split over the chunks of the sweep buffer: the arithmetic of
// run_sweep (sweep.h) on its own. Pure host code (no HIP include), shared by probe.hip and the host
// unit test (native/tests/test_probe_sweep.cc), which compares it byte by byte with a brute-force
// reference.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

// The HBM sweep buffer is allocated as kSweepChunk pieces, not one ~282 GiB allocation: freeing
// one huge mapping held the process's address-space lock for ~2.5 s, and every thread of the agent
// that mapped memory meanwhile (a thread start, a large malloc) stalled behind it — a claim issued
// right after a scrub waited 2.46 s (profiles/r2o_scrub_claim_diag.txt). Per chunk the stall is
// bounded by one chunk's unmap. 1 GiB: VRAM that an earlier process used is cleared as it is mapped
// again, at ~35 GB/s — 121 ms per 4 GiB chunk on a box whose last tenant left 90 GiB dirty
// (profiles/r4r_sweep_chunks.txt) — and a claim-time probe that arrives mid-chunk waits for it.
constexpr uint64_t kSweepChunk = 1ull << 30;

// The part of a window that lies in one chunk of the buffer; tested as one pattern pass.
struct SweepPiece {
  size_t chunk = 0;      // index of the buffer chunk
  uint64_t in = 0;       // byte offset inside that chunk
  uint64_t bytes = 0;    // a multiple of 16, never 0
  uint64_t first16 = 0;  // the piece's first 16-byte chunk, counted from the window's start
  uint32_t seed = 0;     // of its pattern: it depends on the piece's MiB of the buffer
};

struct SweepWindow {
  uint64_t offset = 0, bytes = 0;  // as tested: wrapped, 16-byte aligned, clipped to the span
  std::vector<SweepPiece> pieces;  // in address order; their bytes add up to ``bytes``
};

// The window [offset, offset + bytes) of a buffer of ``span`` bytes made of ``chunk``-byte pieces
// (a multiple of 16; the last one holds what is left of the span): the offset wraps modulo the span
// and is rounded down to 16, the length is clipped to the end of the span and rounded down to 16.
inline SweepWindow sweep_window(uint64_t span, uint64_t chunk, uint64_t offset, uint64_t bytes) {
  SweepWindow w;
  if (span == 0 || chunk == 0) return w;
  const uint64_t a16 = ~static_cast<uint64_t>(15);
  w.offset = (offset % span) & a16;
  w.bytes = std::min<uint64_t>(bytes, span - w.offset) & a16;
  const uint64_t end = w.offset + w.bytes;
  for (uint64_t pos = w.offset; pos < end;) {
    SweepPiece p;
    p.chunk = static_cast<size_t>(pos / chunk);
    p.in = pos % chunk;
    const uint64_t clen = std::min<uint64_t>(chunk, span - p.chunk * chunk);  // the last chunk is short
    p.bytes = std::min<uint64_t>(end - pos, clen - p.in) & a16;
    if (p.bytes == 0) break;
    p.first16 = (pos - w.offset) / 16;
    p.seed = 0x5CAB0000u ^ static_cast<uint32_t>(pos >> 20);
    w.pieces.push_back(p);
    pos += p.bytes;
  }
  return w;
}

}  // namespace
