// fa_bf16_geometry.hpp — the launch geometry of the bfloat16 widen-and-sum (fa_fold_bf16, DESIGN.md
// section 20).  Host-only, on fa_geometry.hpp alone, so that a CPU box can build it; fa_geometry.hpp
// itself is unchanged.
#pragma once

#include "fa_geometry.hpp"

namespace fa {

// One wave-chunk of a bfloat16 row is 64 lanes x 16 B = 512 columns (1 KiB, as the fp32 fold's chunk
// of 256).  A lane keeps 8 fp32 sums per chunk (twice the fp32 fold's 4), so a wave holds at most
// kBf16MaxV chunks of a piece (32 sum registers): pieces of <= kBf16PieceChunks chunks = 16 KiB of
// every row.  The block keeps the fold's 64 KiB of client rows in flight: D = 64 / (V * W) rows.
constexpr int kBf16W = 4, kBf16MaxV = 4, kBf16InFlight = 64;
constexpr int kBf16PieceChunks = kBf16W * kBf16MaxV;
constexpr int64_t kBf16Chunk = 512;

// plan_q8_window's rule on 512-column chunks: ~0.75 blocks per CU (forced: fa_set_reduce_grid), a few
// more blocks (up to rows_grid_max) for a window just past one round of full pieces, the narrowest
// piece (V chunks per wave) that covers the block's share.  Wider windows are swept piece after
// piece by the kernel (equal interleaved pieces, derived from the grid as fold_kernel_rows does).
inline Plan plan_bf16_window(int64_t ncols, int cus, int forced = 0) {
  const int64_t chunks = ceil_div(ncols, kBf16Chunk);
  int64_t grid = forced > 0 ? forced : natural_grid(cus);
  if (forced <= 0 && chunks > grid * kBf16PieceChunks && chunks <= rows_grid_max(cus) * kBf16PieceChunks)
    grid = ceil_div(chunks, kBf16PieceChunks);
  if (grid > chunks) grid = chunks;
  if (grid < 1) grid = 1;
  const int64_t share = ceil_div(chunks, grid);  // chunks per block
  int v = 1;
  while (v < kBf16MaxV && share > v * kBf16W) v *= 2;
  return Plan{kFamFoldRows, v, kBf16W, kBf16InFlight / (v * kBf16W), 0, 0, false, grid};
}

}  // namespace fa
