// fa_quant4_geometry.hpp — the launch geometry of the int4 dequantize-and-sum (fa_deq_fold_q4,
// DESIGN.md section 18).  Host-only, on fa_geometry.hpp alone, as fa_quant_geometry.hpp; both of
// those are unchanged.  Restated by tests/quant4_ref.py.
#pragma once

#include "fa_geometry.hpp"

namespace fa {

// One wave-chunk of a code row is 64 lanes x 16 B = 2048 columns = 16 scale blocks (FA_Q4_CHUNK,
// FA_Q4_BLOCK).  A lane keeps 32 fp32 sums per chunk (twice the int8 kernel's 16) and 32 centre
// values beside them, so a wave holds at most kQ4MaxV chunks of a piece: pieces of
// <= kQ4PieceChunks chunks.  The block keeps the fold's 64 KiB of client rows in flight:
// D = 64 / (V * W) rows.
constexpr int kQ4W = 4, kQ4MaxV = 1, kQ4InFlight = 64;
constexpr int kQ4PieceChunks = kQ4W * kQ4MaxV;
constexpr int64_t kQ4Chunk = 2048;
// The kernel is bound by instruction issue, not by HBM, and its 204 VGPRs leave room for two
// resident blocks per CU (two waves per SIMD): the grid fills them.  Measured on 100 x 25.6 M
// (profiles/quant4/bench_quant4.json): 192 blocks, plan_q8_window's 0.75 per CU, 0.58 ms; 256 0.47;
// 512 0.42; 768 0.41.
constexpr int kQ4BlocksPerCU = 2;

// plan_q8_window's rule on 2048-column chunks with two differences in the grid: kQ4BlocksPerCU blocks
// per CU instead of ~0.75 (forced: fa_set_reduce_grid), and no few-more-blocks clause — plan_q8_window
// widens its grid up to rows_grid_max for a window just past one round of full pieces; at two blocks
// per CU the grid is already past rows_grid_max, so that clause could never apply and is gone.  The
// rest is the rule: never more blocks than chunks, the narrowest shipped piece (V chunks per wave)
// that covers the block's share, wider shares swept piece after piece by the kernel.
inline Plan plan_q4_window(int64_t ncols, int cus, int forced = 0) {
  const int64_t chunks = ceil_div(ncols, kQ4Chunk);
  int64_t grid = forced > 0 ? forced : (int64_t)cus * kQ4BlocksPerCU;
  if (grid > chunks) grid = chunks;
  if (grid < 1) grid = 1;
  const int64_t share = ceil_div(chunks, grid);  // chunks per block
  int v = 1;
  while (v < kQ4MaxV && share > v * kQ4W) v *= 2;
  return Plan{kFamFoldRows, v, kQ4W, kQ4InFlight / (v * kQ4W), 0, 0, false, grid};
}

}  // namespace fa
