// fa_quant1_geometry.hpp — the launch geometry of the 1-bit sign-and-scale sum (fa_deq_fold_q1,
// DESIGN.md section 21).  Host-only, on fa_geometry.hpp alone, as fa_quant4_geometry.hpp; that one
// is unchanged.  Restated by tests/quant1_ref.py.
#pragma once

#include "fa_geometry.hpp"

namespace fa {

// One wave-chunk of a code row is 64 lanes x 4 B = 2048 columns = 16 scale blocks (FA_Q1_CHUNK,
// FA_Q1_BLOCK): the int4 round's row and plan arithmetic.  A lane keeps 32 fp32 sums per chunk and
// 32 centre values beside them, so a wave holds kQ1MaxV chunk of a piece: pieces of
// <= kQ1PieceChunks chunks.
constexpr int kQ1W = 4, kQ1MaxV = 1;
constexpr int kQ1PieceChunks = kQ1W * kQ1MaxV;
constexpr int64_t kQ1Chunk = 2048;
// The pipeline depth.  A row is 256 B per wave, so the family's "64 KiB of client rows in flight"
// would be 64 rows per wave; what bounds D here is load latency on one side (a row's 32 columns
// are 82 VALU instructions, so D rows cover D x 82 issue slots) and two VGPRs per slot on the
// other.  FA_Q1_DEPTH rebuilds the unit at another depth for the measurement
// (tools/bench_quant1.py --lib).  Measured on 100 x 25.6 M (profiles/quant1/depth_and_grid.txt), ms
// at 2 / 3 blocks per CU: D = 8 (150 VGPRs, 3 waves per SIMD) 0.287 / 0.272; D = 16 (183 VGPRs, 2
// waves) 0.283 / 0.284; D = 32 (244 VGPRs) 0.307 / 0.309.  Depth buys nothing past 8 and costs the
// third resident wave; a chain of 25-row chunks (rows < 2 D run the drain) is 0.479 ms at D = 8
// against 0.549 at 16.
#ifndef FA_Q1_DEPTH
#define FA_Q1_DEPTH 8
#endif
constexpr int kQ1Depth = FA_Q1_DEPTH;
// Blocks per CU.  The kernel is bound by instruction issue like q4, whose two blocks per CU were the
// start; at D = 8 three blocks are resident (three waves per SIMD) and the grid fills them: 256
// blocks 0.359 ms, 512 0.287, 768 0.272.
constexpr int kQ1BlocksPerCU = 3;

// plan_q4_window's rule with this unit's constants: kQ1BlocksPerCU blocks per CU (forced:
// fa_set_reduce_grid), never more blocks than chunks, the narrowest shipped piece (V chunks per
// wave) that covers the block's share, wider shares swept piece after piece by the kernel.
inline Plan plan_q1_window(int64_t ncols, int cus, int forced = 0) {
  const int64_t chunks = ceil_div(ncols, kQ1Chunk);
  int64_t grid = forced > 0 ? forced : (int64_t)cus * kQ1BlocksPerCU;
  if (grid > chunks) grid = chunks;
  if (grid < 1) grid = 1;
  const int64_t share = ceil_div(chunks, grid);  // chunks per block
  int v = 1;
  while (v < kQ1MaxV && share > v * kQ1W) v *= 2;
  return Plan{kFamFoldRows, v, kQ1W, kQ1Depth, 0, 0, false, grid};
}

}  // namespace fa
