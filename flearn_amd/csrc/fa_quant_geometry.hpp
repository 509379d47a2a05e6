// fa_quant_geometry.hpp — the launch geometry of the int8 dequantize-and-sum (fa_deq_fold_q8,
// DESIGN.md section 17).  Host-only, on fa_geometry.hpp alone, so that a CPU box can build it
// (tests/quant_geometry_probe.cpp); fa_geometry.hpp itself is unchanged.
#pragma once

#include "fa_geometry.hpp"

namespace fa {

// One wave-chunk of a code row is 64 lanes x 16 B = 1024 columns = one scale block (FA_Q8_BLOCK).
// A lane keeps 16 fp32 sums per chunk (four times the fp32 fold's 4), and 16 centre values beside
// them, so a wave holds at most kQ8MaxV chunks of a piece: pieces of <= kQ8PieceChunks chunks.
// The block keeps the fold's 64 KiB of client rows in flight: D = 64 / (V * W) rows.
constexpr int kQ8W = 4, kQ8MaxV = 2, kQ8InFlight = 64;
constexpr int kQ8PieceChunks = kQ8W * kQ8MaxV;
constexpr int64_t kQ8Block = 1024;

// plan_fold_window's rule on 1024-column chunks: ~0.75 blocks per CU (forced: fa_set_reduce_grid),
// a few more blocks (up to rows_grid_max) for a window just past one round of full pieces, the
// narrowest piece (V chunks per wave) that covers the block's share.  Wider windows are swept
// piece after piece by the kernel (equal interleaved pieces, derived from the grid as
// fold_kernel_rows does).
inline Plan plan_q8_window(int64_t ncols, int cus, int forced = 0) {
  const int64_t chunks = ceil_div(ncols, kQ8Block);
  int64_t grid = forced > 0 ? forced : natural_grid(cus);
  if (forced <= 0 && chunks > grid * kQ8PieceChunks && chunks <= rows_grid_max(cus) * kQ8PieceChunks)
    grid = ceil_div(chunks, kQ8PieceChunks);
  if (grid > chunks) grid = chunks;
  if (grid < 1) grid = 1;
  const int64_t share = ceil_div(chunks, grid);  // chunks per block
  int v = 1;
  while (v < kQ8MaxV && share > v * kQ8W) v *= 2;
  return Plan{kFamFoldRows, v, kQ8W, kQ8InFlight / (v * kQ8W), 0, 0, false, grid};
}

}  // namespace fa
