// fa_mx_geometry.hpp — the launch geometry of the Microscaling dequantize-and-sum (fa_deq_fold_mx,
// DESIGN.md section 22).  Host-only, on fa_geometry.hpp alone, as fa_quant1_geometry.hpp; that one
// is unchanged.
#pragma once

#include "fa_geometry.hpp"

namespace fa {

// One wave-chunk of a code row is 64 lanes x 32 columns = 2048 columns = 64 scale bytes for both
// element types (FA_MX_CHUNK, FA_MX_BLOCK): 1 KiB of FP4 codes, 2 KiB of FP8 codes.  A lane keeps 32
// fp32 sums per chunk and 32 centre values beside them, so a wave holds kMxMaxV chunk of a piece:
// pieces of <= kMxPieceChunks chunks.
constexpr int kMxW = 4, kMxMaxV = 1;
constexpr int kMxPieceChunks = kMxW * kMxMaxV;
constexpr int64_t kMxChunk = 2048;
// The pipeline depth, per element type: a slot is 4 code VGPRs and a scale byte for FP4, 8 and a
// byte for FP8.  FA_MX_DEPTH4 / FA_MX_DEPTH8 rebuild the unit at another depth for the measurement
// (tools/bench_mx.py --lib).  Measured on 100 x 25.6 M (profiles/mx/depth_and_grid.txt), ms at 2 / 3
// blocks per CU: FP4 D = 8 (186 VGPRs) 0.376 / 0.388, D = 16 (226 VGPRs) 0.379 / 0.398; FP8 D = 8
// (220 VGPRs) 0.582 / 0.585, D = 4 (184 VGPRs) 0.583 / 0.663.  Every build holds two waves per SIMD,
// so depth past 8 buys nothing, and a chain of 25-row chunks (rows < 2 D run the drain) is 0.574 ms
// at FP4 D = 8 against 0.616 at 16.
#ifndef FA_MX_DEPTH4
#define FA_MX_DEPTH4 8
#endif
#ifndef FA_MX_DEPTH8
#define FA_MX_DEPTH8 8
#endif
constexpr int kMxDepth4 = FA_MX_DEPTH4, kMxDepth8 = FA_MX_DEPTH8;
// Blocks per CU: both instantiations hold two waves per SIMD, that is two resident blocks of four
// waves per CU, and the grid fills exactly those: 512 blocks 0.376 ms (FP4) / 0.582 (FP8), 768 0.388 /
// 0.585, 1024 0.388 / 0.590.
constexpr int kMxBlocksPerCU = 2;

// plan_q1_window's rule with this unit's constants: kMxBlocksPerCU blocks per CU (forced:
// fa_set_reduce_grid), never more blocks than chunks, the narrowest shipped piece (V chunks per
// wave) that covers the block's share, wider shares swept piece after piece by the kernel.
inline Plan plan_mx_window(int64_t ncols, int cus, int elem, int forced = 0) {
  const int64_t chunks = ceil_div(ncols, kMxChunk);
  int64_t grid = forced > 0 ? forced : (int64_t)cus * kMxBlocksPerCU;
  if (grid > chunks) grid = chunks;
  if (grid < 1) grid = 1;
  const int64_t share = ceil_div(chunks, grid);  // chunks per block
  int v = 1;
  while (v < kMxMaxV && share > v * kMxW) v *= 2;
  return Plan{kFamFoldRows, v, kMxW, elem == 4 ? kMxDepth4 : kMxDepth8, 0, 0, false, grid};
}

}  // namespace fa
