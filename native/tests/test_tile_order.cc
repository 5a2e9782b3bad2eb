// The probe GEMM's workgroup -> tile mapping (native/src/probe/tile_order.h), exhaustively on the
// host: every blockIdx of every grid up to 16x16 tiles must reach a distinct in-range tile for
// every group size, also with a short last group and a grid that is no multiple of the 8 XCDs.
#include <vector>

#include "../src/probe/tile_order.h"
#include "testing.h"

TEST(xcd_remap_is_a_permutation) {
  for (int nwg = 1; nwg <= 600; ++nwg) {
    std::vector<int> seen(static_cast<size_t>(nwg), 0);
    for (int b = 0; b < nwg; ++b) {
      const int wg = xcd_remap(b, nwg);
      EXPECT_TRUE(wg >= 0 && wg < nwg);
      ++seen[static_cast<size_t>(wg)];
    }
    for (int w = 0; w < nwg; ++w) EXPECT_EQ(seen[static_cast<size_t>(w)], 1);
  }
}

TEST(xcd_remap_keeps_an_xcd_contiguous) {
  // blockIdx b runs on XCD b % 8: its successive blocks take consecutive logical tiles
  for (int nwg : {8, 15, 16, 21, 256, 600})
    for (int b = 0; b + 8 < nwg; ++b) EXPECT_EQ(xcd_remap(b + 8, nwg), xcd_remap(b, nwg) + 1);
}

TEST(block_to_tile_is_a_bijection) {
  const int groups[] = {0, 1, 2, 3, 4, 5, 8, 9, 16, 17};
  for (int tiles_m = 1; tiles_m <= 16; ++tiles_m)
    for (int tiles_n = 1; tiles_n <= 16; ++tiles_n)
      for (int group_m : groups) {
        const int nwg = tiles_m * tiles_n;
        std::vector<int> seen(static_cast<size_t>(nwg), 0);
        for (int b = 0; b < nwg; ++b) {
          int tm = -1, tn = -1;
          grouped_tile(xcd_remap(b, nwg), tiles_m, tiles_n, group_m, &tm, &tn);
          EXPECT_TRUE(tm >= 0 && tm < tiles_m);
          EXPECT_TRUE(tn >= 0 && tn < tiles_n);
          ++seen[static_cast<size_t>(tm * tiles_n + tn)];
        }
        for (int t = 0; t < nwg; ++t) EXPECT_EQ(seen[static_cast<size_t>(t)], 1);
      }
}

TEST(grouped_order_walks_a_group_column_major) {
  // 5x3 tiles in groups of 4: a full group of 4 rows, then a short one of 1 row
  int tm, tn;
  grouped_tile(0, 5, 3, 4, &tm, &tn);
  EXPECT_TRUE(tm == 0 && tn == 0);
  grouped_tile(1, 5, 3, 4, &tm, &tn);
  EXPECT_TRUE(tm == 1 && tn == 0);
  grouped_tile(4, 5, 3, 4, &tm, &tn);
  EXPECT_TRUE(tm == 0 && tn == 1);
  grouped_tile(12, 5, 3, 4, &tm, &tn);
  EXPECT_TRUE(tm == 4 && tn == 0);
  grouped_tile(14, 5, 3, 4, &tm, &tn);
  EXPECT_TRUE(tm == 4 && tn == 2);
  grouped_tile(7, 5, 3, 1, &tm, &tn);  // row-major
  EXPECT_TRUE(tm == 2 && tn == 1);
}
