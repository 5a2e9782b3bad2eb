// Workgroup -> output tile mapping of the probe's GEMM kernels (gemm_bf16.h): pure integer functions,
// shared by the kernels and the host unit test (native/tests/test_tile_order.cc).
#pragma once

#if defined(__HIPCC__)
#define TILE_ORDER_FN __host__ __device__ __forceinline__
#else
#define TILE_ORDER_FN inline
#endif

// Bijective XCD-aware remap (cdna_hip_programming.md §5 "XCD swizzle must be bijective"):
// consecutive logical tiles land on the same XCD (shared L2) under round-robin dispatch.
TILE_ORDER_FN int xcd_remap(int orig, int nwg) {
  int q = nwg / 8, r = nwg % 8, xcd = orig % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
}

// Tile order inside each XCD's contiguous range of wg (xcd_remap): row-major (group_m <= 1) walks
// whole tile rows, so the tiles an XCD runs at once share one or two A panels but need a B panel
// each; grouped (group_m rows at a time, column-major inside a group) makes them a group_m x k
// block that shares both, less operand traffic into the XCD's 4 MB L2 per K-step. Bijective, also
// when the last group has fewer than group_m rows.
TILE_ORDER_FN void grouped_tile(int wg, int tiles_m, int tiles_n, int group_m, int* tile_m, int* tile_n) {
  if (group_m > 1) {
    const int per_group = group_m * tiles_n, first_m = (wg / per_group) * group_m;
    const int rest = tiles_m - first_m, gm = rest < group_m ? rest : group_m, r = wg % per_group;
    *tile_m = first_m + r % gm;
    *tile_n = r / gm;
  } else {
    *tile_m = wg / tiles_n;
    *tile_n = wg % tiles_n;
  }
}
