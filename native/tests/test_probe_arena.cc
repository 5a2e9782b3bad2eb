// The probe's arena layout (native/src/probe/arena.h) against the closed form of the sizes the
// probe has always used: regions 4 KiB-aligned, disjoint, in order, counters right behind the GEMM
// region, nothing reserved for the low-precision phase unless a dtype is asked for.
#include <cstddef>
#include <cstdint>

#include "../src/probe/arena.h"
#include "testing.h"

static size_t al(size_t x) { return (x + 4095) & ~static_cast<size_t>(4095); }

// 2 counters per HBM pattern (4), element + ABFT + census-bad, two CU maps of 2048 bits
static const size_t kCounters = 2 * 4 + 3 + 2 * (2048 / 64);

TEST(probe_arena_layout_matches_closed_form) {
  EXPECT_EQ(static_cast<size_t>(kResSlots), kCounters);
  for (int gemm_n : {256, 512, 2048, 4096})
    for (uint64_t n16 : {uint64_t{1}, uint64_t{65536}, uint64_t{1} << 26})
      for (bool do_mfma : {false, true})
        for (int mask : {0, 1, 7}) {
          const ArenaLayout l = ArenaLayout::make(n16, gemm_n, do_mfma, mask);
          const size_t n = static_cast<size_t>(gemm_n), n0 = 256;
          const size_t sz_a0 = al(n0 * n0 * 2), sz_c0 = al(n0 * n0 * 4), sz_a = al(n * n * 2), sz_c = al(n * n * 4),
                       sz_v = al(6 * n * 8);
          const size_t gemm_bytes = do_mfma ? 2 * sz_a0 + 2 * sz_c0 + 2 * sz_a + sz_c + sz_v : 0;
          const size_t hbm_region = al(n16 * 16);
          const size_t region = hbm_region + gemm_bytes;
          const size_t lowp_off = region + al(kCounters * 8);
          EXPECT_EQ(l.hbm, size_t{0});
          EXPECT_EQ(l.cnt, region);
          EXPECT_EQ(l.lowp_cnt, lowp_off);
          if (do_mfma) {  // the order launch_mfma_phase has always carved them in
            EXPECT_EQ(l.a0, hbm_region);
            EXPECT_EQ(l.b0, l.a0 + sz_a0);
            EXPECT_EQ(l.c0, l.b0 + sz_a0);
            EXPECT_EQ(l.r0, l.c0 + sz_c0);
            EXPECT_EQ(l.a, l.r0 + sz_c0);
            EXPECT_EQ(l.b, l.a + sz_a);
            EXPECT_EQ(l.c, l.b + sz_a);
            EXPECT_EQ(l.v, l.c + sz_c);
            EXPECT_EQ(l.v + sz_v, l.cnt);
          }
          const size_t offs[] = {l.hbm, l.a0, l.b0, l.c0, l.r0, l.a, l.b, l.c, l.v, l.cnt, l.lowp_cnt, l.lowp_region, l.need};
          for (size_t i = 0; i < sizeof offs / sizeof *offs; ++i) {
            EXPECT_EQ(offs[i] % 4096, size_t{0});
            if (i) EXPECT_TRUE(offs[i - 1] <= offs[i]);  // in order; equal only for an empty region
          }
          if (mask == 0) {
            EXPECT_EQ(l.need, lowp_off);  // no lowp constant in it
            EXPECT_EQ(l.lowp_region, l.need);
          } else {
            // per dtype: element, ABFT and census-bad counters and a CU map; 8-bit operands
            const size_t lowp_cnt_bytes = al(3 * (3 + 2048 / 64) * 8);
            const size_t lowp_region = 2 * al(n0 * n0) + 2 * al(n0 * n0 / 32) + 2 * al(n0 * n0 * 4) + 2 * al(n * n) +
                                       2 * al(n * n / 32) + al(n * n * 4) + al(6 * n * 4);
            EXPECT_EQ(l.lowp_region, lowp_off + lowp_cnt_bytes);
            EXPECT_EQ(l.need, lowp_off + lowp_cnt_bytes + lowp_region);
            EXPECT_EQ(lowp::region_bytes(n), lowp_region);
          }
        }
}

TEST(probe_arena_without_mfma_has_no_gemm_region) {
  const ArenaLayout l = ArenaLayout::make(65536, 4096, false, 0);
  EXPECT_EQ(l.cnt, size_t{1} << 20);
  EXPECT_EQ(l.a0, l.cnt);
  EXPECT_EQ(l.v, l.cnt);
  EXPECT_EQ(l.need, (size_t{1} << 20) + 4096);
}
