// The split of an HBM sweep window over the sweep buffer's chunks (native/src/probe/sweep_window.h)
// against a brute-force reference that places every byte of the buffer, over an exhaustive grid of
// small synthetic buffers (256-byte chunks), then the production 1 GiB chunk at hand-picked seams.
#include <cstdint>
#include <sstream>
#include <vector>

#include "../src/probe/sweep_window.h"
#include "testing.h"

namespace {

struct Where {
  uint64_t chunk, in;
  bool operator==(const Where& o) const { return chunk == o.chunk && in == o.in; }
};

// Reference, part one: where every byte of the buffer lives, found by stepping a (chunk,
// offset-in-chunk) pair along the span — no division by the chunk size.
std::vector<Where> byte_map(uint64_t span, uint64_t chunk) {
  std::vector<Where> at;
  Where w{0, 0};
  for (uint64_t pos = 0; pos < span; ++pos) {
    at.push_back(w);
    if (++w.in == chunk) w = Where{w.chunk + 1, 0};
  }
  return at;
}

// Everything the issue asks of one split; throws with the case in the message. ``at``: byte_map.
void check_case(const std::vector<Where>& at, uint64_t span, uint64_t chunk, uint64_t offset, uint64_t bytes) {
  try {
    const SweepWindow w = sweep_window(span, chunk, offset, bytes);
    // reference, part two: the wrapped, aligned, clipped window by its definition
    uint64_t ref_offset = offset % span;
    ref_offset -= ref_offset % 16;
    uint64_t ref_bytes = bytes < span - ref_offset ? bytes : span - ref_offset;
    ref_bytes -= ref_bytes % 16;
    EXPECT_EQ(w.offset, ref_offset);
    EXPECT_EQ(w.bytes, ref_bytes);
    EXPECT_TRUE(w.offset % 16 == 0 && w.bytes % 16 == 0 && w.offset + w.bytes <= span);
    uint64_t next16 = 0, covered = 0;  // covered: bytes of the window the pieces have tiled so far
    for (const SweepPiece& p : w.pieces) {
      EXPECT_TRUE(p.bytes > 0);  // no zero-length piece
      EXPECT_EQ(p.bytes % 16, uint64_t{0});
      EXPECT_EQ(p.in % 16, uint64_t{0});
      EXPECT_EQ(p.first16, next16);  // the relative chunk numbers are contiguous
      next16 += p.bytes / 16;
      // inside one chunk, and inside what that chunk really holds: the last one is short
      const uint64_t chunks = (span + chunk - 1) / chunk;
      EXPECT_TRUE(p.chunk < chunks);
      const uint64_t real = p.chunk + 1 < chunks ? chunk : span - (chunks - 1) * chunk;
      EXPECT_TRUE(p.in + p.bytes <= real);
      EXPECT_EQ(p.seed, 0x5CAB0000u ^ static_cast<uint32_t>((p.chunk * chunk + p.in) >> 20));
      // byte k of the piece is byte covered + k of the window: the pieces tile it exactly, in order
      EXPECT_TRUE(covered + p.bytes <= ref_bytes);
      for (uint64_t k = 0; k < p.bytes; ++k) EXPECT_TRUE((Where{p.chunk, p.in + k}) == at[ref_offset + covered + k]);
      covered += p.bytes;
    }
    EXPECT_EQ(covered, ref_bytes);
    // consecutive pieces sit in consecutive chunks: a window is one address range
    for (size_t i = 1; i < w.pieces.size(); ++i) {
      EXPECT_EQ(w.pieces[i].chunk, w.pieces[i - 1].chunk + 1);
      EXPECT_EQ(w.pieces[i].in, uint64_t{0});
    }
  } catch (const gtest_lite::Failure& f) {
    std::ostringstream os;
    os << f.what() << " [span " << span << ", chunk " << chunk << ", offset " << offset << ", bytes " << bytes << "]";
    throw gtest_lite::Failure(os.str());
  }
}

}  // namespace

TEST(probe_sweep_window_matches_brute_force_on_small_buffers) {
  const uint64_t chunk = 256;
  // one chunk, a whole number of chunks, a last chunk of 16 bytes, of all but 16, and spans that are
  // no multiple of 16 (the production span is 2 MiB granular; the clipping must hold anyway)
  for (uint64_t span : {16u, 48u, 255u, 256u, 272u, 496u, 512u, 520u, 776u, 1024u, 1040u}) {
    const std::vector<Where> at = byte_map(span, chunk);
    size_t cases = 0;
    for (uint64_t offset = 0; offset < 2 * span + chunk; offset += (offset % 16 == 0 ? 1 : (offset % 16 == 1 ? 7 : 8)))
      for (uint64_t bytes = 0; bytes <= span + 2 * chunk; bytes += (bytes % 16 == 0 ? 8 : (bytes % 16 == 8 ? 7 : 1))) {
        check_case(at, span, chunk, offset, bytes);
        ++cases;
      }
    EXPECT_TRUE(cases > 100);
  }
  // other chunk sizes, the degenerate one included (every 16 bytes a seam)
  for (uint64_t c : {16u, 48u, 1024u})
    for (uint64_t span : {c, c + 16, 3 * c, 3 * c + 40, 5 * c - 16}) {
      const std::vector<Where> at = byte_map(span, c);
      for (uint64_t offset = 0; offset < 2 * span; offset += 8)
        for (uint64_t bytes = 0; bytes <= span + c; bytes += 24) check_case(at, span, c, offset, bytes);
    }
}

TEST(probe_sweep_window_of_nothing) {
  EXPECT_TRUE(sweep_window(0, 256, 0, 1024).pieces.empty());
  EXPECT_EQ(sweep_window(0, 256, 0, 1024).bytes, uint64_t{0});
  EXPECT_TRUE(sweep_window(1024, 256, 512, 15).pieces.empty());
  EXPECT_TRUE(sweep_window(8, 256, 0, 1024).pieces.empty());  // a span below one 16-byte chunk
}

namespace {

void expect_piece(const SweepPiece& p, size_t chunk, uint64_t in, uint64_t bytes, uint64_t first16, uint32_t seed) {
  EXPECT_EQ(p.chunk, chunk);
  EXPECT_EQ(p.in, in);
  EXPECT_EQ(p.bytes, bytes);
  EXPECT_EQ(p.first16, first16);
  EXPECT_EQ(p.seed, seed);
}

}  // namespace

TEST(probe_sweep_window_production_chunk_hand_cases) {
  const uint64_t G = 1ull << 30, M = 1ull << 20;
  EXPECT_EQ(kSweepChunk, G);
  const uint64_t span = 16 * G - 6 * M;  // 16 chunks, the last one 6 MiB short
  const uint32_t base = 0x5CAB0000u;     // seed: base ^ (the piece's first MiB of the buffer)
  {  // ends exactly on the first seam: one piece, nothing of chunk 1
    const SweepWindow w = sweep_window(span, kSweepChunk, G - 2 * M, 2 * M);
    EXPECT_EQ(w.offset, G - 2 * M);
    EXPECT_EQ(w.bytes, 2 * M);
    EXPECT_EQ(w.pieces.size(), size_t{1});
    expect_piece(w.pieces[0], 0, G - 2 * M, 2 * M, 0, base ^ 1022u);
  }
  {  // starts exactly on it
    const SweepWindow w = sweep_window(span, kSweepChunk, G, 2 * M);
    EXPECT_EQ(w.pieces.size(), size_t{1});
    expect_piece(w.pieces[0], 1, 0, 2 * M, 0, base ^ 1024u);
  }
  {  // starts one 16-byte chunk before the seam (and at an unaligned offset: rounded down)
    const SweepWindow w = sweep_window(span, kSweepChunk, G - 16 + 9, M);
    EXPECT_EQ(w.offset, G - 16);
    EXPECT_EQ(w.bytes, M);
    EXPECT_EQ(w.pieces.size(), size_t{2});
    expect_piece(w.pieces[0], 0, G - 16, 16, 0, base ^ 1023u);
    expect_piece(w.pieces[1], 1, 0, M - 16, 1, base ^ 1024u);
  }
  {  // crosses two seams
    const SweepWindow w = sweep_window(span, kSweepChunk, G - M, G + 2 * M);
    EXPECT_EQ(w.bytes, G + 2 * M);
    EXPECT_EQ(w.pieces.size(), size_t{3});
    expect_piece(w.pieces[0], 0, G - M, M, 0, base ^ 1023u);
    expect_piece(w.pieces[1], 1, 0, G, M / 16, base ^ 1024u);
    expect_piece(w.pieces[2], 2, 0, M, (M + G) / 16, base ^ 2048u);
  }
  {  // offset >= span wraps: span + (1 GiB - 1 MiB) is the straddle of the first seam
    const SweepWindow w = sweep_window(span, kSweepChunk, span + G - M, 2 * M);
    EXPECT_EQ(w.offset, G - M);
    EXPECT_EQ(w.bytes, 2 * M);
    EXPECT_EQ(w.pieces.size(), size_t{2});
    expect_piece(w.pieces[0], 0, G - M, M, 0, base ^ 1023u);
    expect_piece(w.pieces[1], 1, 0, M, M / 16, base ^ 1024u);
  }
  {  // reaches into the short last chunk
    const SweepWindow w = sweep_window(span, kSweepChunk, 15 * G - M, 4 * M);
    EXPECT_EQ(w.bytes, 4 * M);
    EXPECT_EQ(w.pieces.size(), size_t{2});
    expect_piece(w.pieces[0], 14, G - M, M, 0, base ^ (15u * 1024u - 1u));
    expect_piece(w.pieces[1], 15, 0, 3 * M, M / 16, base ^ (15u * 1024u));
  }
  {  // asks for 4 MiB one MiB before the end: clipped to the short chunk's real length
    const SweepWindow w = sweep_window(span, kSweepChunk, span - M, 4 * M);
    EXPECT_EQ(w.offset, span - M);
    EXPECT_EQ(w.bytes, M);
    EXPECT_EQ(w.pieces.size(), size_t{1});
    expect_piece(w.pieces[0], 15, G - 7 * M, M, 0, base ^ static_cast<uint32_t>((span - M) >> 20));
  }
  {  // the whole span in one window: 16 pieces, the last one short
    const SweepWindow w = sweep_window(span, kSweepChunk, 0, ~0ull);
    EXPECT_EQ(w.bytes, span);
    EXPECT_EQ(w.pieces.size(), size_t{16});
    expect_piece(w.pieces[15], 15, 0, G - 6 * M, 15 * G / 16, base ^ (15u * 1024u));
  }
}
