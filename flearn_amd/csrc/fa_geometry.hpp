// fa_geometry.hpp — which kernel instantiation runs for a shape, and on what grid: the reduces, the
// folds, the trimmed sums, the Gram matrix, the norm-clipped rounds and their Gaussian noise.
//
// And one numerics decision on a launch constant: whether the epilogues' reciprocal quotient is exact
// for a weight sum (recip_quot_exact).
//
// Plain C++17, pure integer decisions: no HIP, no globals, no device queries.  fa_reduce.hip asks
// these functions for a Plan and turns it into a launch; tests/geometry_probe.cpp asks them on a
// CPU box (tests/test_geometry_plan.py).  Measured with tools/tune_reduce.hip on MI355X
// (DESIGN.md §4); every rule carries the measurement behind it.
#pragma once

#include <stdint.h>
#include <string.h>

#include <initializer_list>

#include "flearn_amd.h"

namespace fa {

enum Family { kFamRows, kFamNarrow, kFamRowmajor, kFamSplitn, kFamBalanced, kFamRowsH16, kFamFoldRows, kFamFoldElem };

// One launch: the kernel family, the template arguments its dispatch varies, and the grid.
struct Plan {
  int family;
  int V, W, D;    // quads (float16: octs) per lane and piece, waves per block, rows in flight
  int KG, EPIB;   // row-major: pieces per group, epilogue slots batched per lane
  bool wide16;    // row-major: 4 waves x 16 KiB pieces instead of 8 waves x 8 KiB
  int64_t grid;
};

// fp32 client stacks.  Fewer blocks than CUs stream best: ~192 blocks on 256 CUs,
// each keeping ~64 KiB of client rows in flight, equal interleaved pieces of the window.
//   * several pieces per block (k >= 2): reduce_kernel_rowmajor, 8 waves x 8 KiB per piece,
//     rows swept once per group of KG pieces (fp32 sums only: f64 sums need 2x the registers);
//   * one piece per block: reduce_kernel_rows; the piece width and pipeline depth follow the
//     share s (KiB of every row per block): the narrowest piece that covers s, D = 64/(V*W) rows
//     deep.  Plain mean: 4 waves x up to 16 KiB per row; fused optimizer epilogues: 8 waves x up
//     to 8 KiB (half the per-lane state work at every piece end, twice the waves to overlap it).
constexpr double kRowsBlocksPerCU = 0.75;
constexpr int kPieceChunks = 64;  // max KiB of a row per block and piece (= W * Vmax)

// 8-byte kinds (f64 / i64 buckets: BN counters, float64 state; small): 4 quads per thread,
// one row at a time, round-balanced grid
constexpr int kBalancedV = 4, kBalancedU = 1;

// Split-N geometry (tools/tune_splitn.py, profiles/r02/tune_splitn): one 1-KiB chunk of every row
// per block, kSplitW client splits (one per wave), each a rolling pipeline kSplitD rows deep.
// 1000 x 44,416 fp32: 28.7 us vs 50.2 us sequential; 4000 x 44,416: 111 vs 184 us; but
// 1000 x 1 M (3907 chunks): 738 vs 572 us — so the split form is used only for windows of fewer
// 1-KiB chunks than CUs, and with at least 2 * kSplitW clients.  And at most kSplitMaxN clients:
// a reordered fp32 sum differs from the sequential one by about the sequential sum's own rounding
// error, which grows like sqrt(N), and the contract is <= 1e-6 per tensor.  The exact CPU
// restatement of both orders (tests/splitn_error.py, profiles/r03/splitn_error.json; LeNet5
// tensors, 3 seeds x 3 weight kinds x 2 data kinds) puts the worst tensor at 6.2e-7 for N = 256,
// 7.4e-7 at 512, 2.5e-6 at 1024 (a 6-element bias, MOON weights), 1.3e-6 at 2048 — so 256.
// Columns whose terms nearly cancel are re-summed in order by the kernel's guard.
constexpr int kSplitW = 4, kSplitD = 8, kSplitMaxN = 256;

// The epilogues divide an fp32 sum x by the launch's weight sum d in double.  For a d with a short
// significand the quotient's two-fma form on r = RN(1/d) (fa_numerics.hpp: quot) is RN(x / d) for
// every fp32 x — proved in DESIGN.md §2 under exactly these conditions, so all three are kept
// although longer denominators passed the exhaustive CPU run too:
//   * d finite and non-zero;
//   * 2^-100 <= |d| <= 2^100 (no product, remainder or correction leaves the normal double range
//     for any fp32 x, subnormal x included);
//   * d's significand has at most 27 significant bits: the low 26 bits of the mantissa field are 0.
// Integer sample counts and unit weights summed (100.0, 3.0, ..., up to 2^27) qualify; 0.001 does
// not and keeps the IEEE divide.
inline bool recip_quot_exact(double d) {
  uint64_t u;
  memcpy(&u, &d, sizeof u);
  const int exp = (int)((u >> 52) & 0x7ff) - 1023;  // finite non-zero normal: -1022 .. 1023
  if (exp < -100 || exp > 100) return false;        // also 0, subnormals, infinities and NaN
  if (exp == 100 && (u & 0xfffffffffffffull) != 0) return false;  // |d| <= 2^100
  return (u & ((1ull << 26) - 1)) == 0;
}

// 1-KiB row pieces of a window of `ncols` elements, `per` of them in a 16-B load
inline int64_t row_chunks(int64_t ncols, int per = 4) { return ((ncols + per - 1) / per + 63) / 64; }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int64_t natural_grid(int cus) { return (int64_t)(cus * kRowsBlocksPerCU + 0.5); }

// The widest grid of one-piece blocks (reduce_kernel_rows) the geometry below uses: 13/16 of the
// CUs (100 x 3.2 M columns on 196 blocks 89.7-90.1%, 100 x 3.5 M on 214 blocks 88.6%)
inline int64_t rows_grid_max(int cus) { return (int64_t)cus * 13 / 16; }

// The grid of one piece per block (fp32 and float16 alike): the forced grid, else ~0.75 blocks
// per CU; never more blocks than chunks.
inline int64_t one_piece_grid(int64_t chunks, int cus, int forced) {
  int64_t grid = forced > 0 ? forced : natural_grid(cus);
  // a window just wider than one round of full pieces: a few more blocks (up to one per CU)
  // instead of a second, nearly empty round
  if (forced <= 0 && chunks > grid * kPieceChunks && chunks <= (int64_t)cus * kPieceChunks)
    grid = ceil_div(chunks, kPieceChunks);
  if (grid < 1) grid = 1;
  if (grid > chunks) grid = chunks;
  return grid;
}

// Row-major geometry for windows of several 64-KiB pieces per block (k >= 2): a grid near `target`
// blocks whose k splits into equal groups of KG in {4, 3, 2} pieces (every step of a group is
// a real piece).  Returns false when no grid in [160, cus] gives such a k.
inline bool rowmajor_geometry(int64_t chunks, int cus, int64_t target, int64_t* grid, int* kg) {
  const int64_t lo = 160 < cus ? 160 : cus, hi = cus;
  for (int64_t d = 0; d <= hi - lo; ++d) {
    for (int sgn = 0; sgn < 2; ++sgn) {
      const int64_t g = sgn ? target - d : target + d;
      if (g < lo || g > hi || (d == 0 && sgn)) continue;
      const int64_t k = ceil_div(chunks, g * kPieceChunks);
      if (k < 2) return false;  // one piece per block: the column-major kernel
      for (int c : {4, 3, 2}) {  // (5 x 8 quads of sums + the pipeline do not fit 256 VGPRs)
        if (k % c == 0) {
          *grid = g;
          *kg = c;
          return true;
        }
      }
    }
  }
  return false;
}

// KG for a forced grid: the group size in {4, 3, 2} that wastes the fewest group slots
inline int kg_for(int64_t k) {
  int best = 4;
  int64_t waste = ceil_div(k, 4) * 4 - k;
  for (int c : {3, 2}) {
    const int64_t wc = ceil_div(k, c) * c - k;
    if (wc < waste) {
      waste = wc;
      best = c;
    }
  }
  return best;
}

// Row-major groups of KG pieces on `grid` blocks: the same 64-KiB pieces either as 8 waves x 8 KiB
// or as 4 waves x 16 KiB.  With several groups per block (k >= 6) 4 waves stream ~1% faster —
// plain mean 100 x 25.6 M: 86.6 vs 85.8% and 85.1 vs 83.7% on two boxes, 100 x 86.6 M: 83.2 vs
// 82.3% (profiles/r02/tune_nsgrid); fused AVGM 100 x 25.6 M: 85.7 vs 84.4%, Adagrad 100 x 86.6 M:
// 85.1 vs 84.1% (profiles/r02/tune_epiw) — with one group (C2, C4) they do not (84.2 vs 85.0%,
// 89.7 vs 89.8%, AVGM 83.2 vs 83.4%).  Yogi's f64 epilogue does not fit 4 x 16 quads of sums at
// KG = 4 (144 spilled VGPRs).
inline Plan rowmajor_plan(int mode, int op, int64_t chunks, int64_t grid, int kg) {
  const int64_t k = ceil_div(chunks, grid * kPieceChunks);
  const bool yogi_f64 = op == FA_OP_YOGI && mode != FA_MODE_W32_DIV32;
  const bool wide16 = k >= 6 && (kg <= 3 || (kg == 4 && !yogi_f64));
  // 4 x 16: fused epilogues batch the state of 4 slots per lane (EPIB 4) instead of 2: one
  // process, 9 interleaved rounds, each variant twice (tools/tune_reduce.hip set "epib4",
  // profiles/r03/tune_epib4/): Adagrad 100 x 86.6 M 5315 -> 5272 us, AVGM 100 x 25.6 M
  // 1599 -> 1595 us, AVGM 100 x 11.7 M 711 -> 707 us; the plain mean has no state (+-0.1%)
  const int epib = wide16 && op != FA_OP_MEAN ? 4 : 2;
  return Plan{kFamRowmajor, wide16 ? 16 : 8, wide16 ? 4 : 8, 1, kg, epib, wide16, grid};
}

inline Plan rows_plan(int v, int w, int64_t grid) {
  return Plan{kFamRows, v, w, kPieceChunks / (v * w), 0, 0, false, grid};
}

// One fp32 stack window (fa_reduce_f32 / fa_reduce_f32_splitn): mode FA_MODE_W32_DIV64 / _DIV32 /
// _W64, op FA_OP_*, n clients, ncols columns, on `cus` CUs; forced: fa_set_reduce_grid (0 = the
// geometry chooses); splitn: the caller allows the reordered sum.
inline Plan plan_f32_window(int mode, int op, int n, int64_t ncols, int cus, int forced, bool splitn) {
  const int64_t chunks = row_chunks(ncols);
  if (splitn && n >= 2 * kSplitW && n <= kSplitMaxN && chunks < cus)  // see kSplitMaxN
    return Plan{kFamSplitn, 0, kSplitW, kSplitD, 0, 0, false, chunks};
  if (mode != FA_MODE_W64) {  // fp32 sums (every flearn weight type but f64)
    if (forced > 0 && chunks > (int64_t)forced * kPieceChunks)
      return rowmajor_plan(mode, op, chunks, forced, kg_for(ceil_div(chunks, (int64_t)forced * kPieceChunks)));
    // Past one round of the grid: row-major groups.  So also where one piece per block would
    // take more than rows_grid_max blocks — two pieces per block on a grid near 13/16 of the
    // CUs instead (100 x 4.19 M columns: 256 one-piece blocks 246 us = 86.0%, 208 blocks x 2
    // pieces 235 us = 90.2%; tools/width_sweep.py, profiles/r06/width/)
    const bool past = chunks > (int64_t)cus * kPieceChunks;
    int64_t g = 0;
    int kg = 0;
    if (forced <= 0 && chunks > rows_grid_max(cus) * kPieceChunks &&
        rowmajor_geometry(chunks, cus, past ? natural_grid(cus) : rows_grid_max(cus), &g, &kg))
      return rowmajor_plan(mode, op, chunks, g, kg);
  }
  int64_t grid = one_piece_grid(chunks, cus, forced);
  int64_t share = ceil_div(chunks, grid);  // chunks per block
  if (share <= 2) {
    // narrow windows (at most two 1-KiB chunks of every row per block: LeNet-sized models, deep
    // client stacks): reduce_kernel_narrow, one single-wave block per chunk, a D-deep pipeline
    // with no drain code and the round's weights broadcast from one VGPR.  A 4- or 8-wave
    // block had work for one or two waves (8-16 KiB in flight per block).  1000 x LeNet5 51.1
    // -> 31.8 us, 2000 clients 98.3 -> 55.6 us, 400 clients 27.5 -> 15.7 us, 100 clients
    // 9.8 -> 7.4 us, 300 x 70,001 -> 17.2 us (tools/tune_reduce.hip sets "deep", "deep2";
    // profiles/r02/tune_deep/).  D: 16 rows below 350 clients (the ramp of a deeper pipeline
    // does not pay off), 32 below 700, else 40 (48-60 lose: fewer waves' worth of latency
    // hiding per row than the issue cost of the extra slots).  Same sums, same order.
    return Plan{kFamNarrow, 1, 1, n < 350 ? 16 : n < 700 ? 32 : 40, 0, 0, false, chunks};
  }
  if (op == FA_OP_MEAN) {
    const int W = 4;
    // A share just past a power of two leaves about half of every pipeline slot empty (the
    // piece is V*W KiB wide, `share` KiB of it real, D = 64/(V*W) rows deep).  Where a grid of
    // at most rows_grid_max blocks makes the share a whole power of two, take that grid: plain
    // mean 100 x 1.6 M columns 95.1 -> 90.3-90.8 us, 100 x 800 K 48.6 -> 46.5 us; shares >= 60% full
    // (100 x 2.4 M, 1.2 M, 600 K, 200 K) lose with it, and so do the fused epilogues
    // (tools/width_sweep.py, profiles/r06/width/)
    if (forced <= 0) {
      int64_t cap = W;
      while (cap < share) cap *= 2;
      const int64_t g2 = ceil_div(chunks, cap / 2);
      if (cap > W && share * 5 < cap * 3 && g2 <= rows_grid_max(cus)) {
        grid = g2;
        share = ceil_div(chunks, grid);
      }
    }
    int v = 1;  // the narrowest piece that covers the share, at most 16 KiB per wave
    while (v < 16 && share > v * W) v *= 2;
    return rows_plan(v, W, grid);
  }
  // shares of at most 8 KiB on 4 waves: with 8 waves one quad per lane (V = 1, 8 rows deep)
  // compiles into register copies — 240 VGPRs, scratch spills and ~1,290 v_mov_b64 per
  // kernel, for every epilogue — and 100 x 200 K FedAVGM took 45 us, 3x the plain mean
  if (share <= 4) return rows_plan(1, 4, grid);
  if (share <= 8) return rows_plan(2, 4, grid);
  // a share just past 16 or 32 KiB: the grid that makes it a whole 16 / 32 KiB piece, on 4
  // waves (the mean's rule; 8 waves lose there): FedAVGM 100 x 1.6 M 85.0 -> 88.4-88.6%,
  // 100 x 800 K 83.0 -> 85.8-86.0%; shares of 9-16 KiB stay on 8 waves (100 x 400 K: 77.9%
  // against 75.6-75.9% filled on 4; tools/width_sweep.py, profiles/r06/width/fused_*)
  if (forced <= 0 && share > 16) {
    const int64_t cap = share <= 32 ? 32 : 64;
    const int64_t g2 = ceil_div(chunks, cap / 2);
    if (share * 5 < cap * 3 && g2 <= rows_grid_max(cus)) return rows_plan(ceil_div(chunks, g2) <= 16 ? 4 : 8, 4, g2);
  }
  return rows_plan(share <= 16 ? 2 : share <= 32 ? 4 : 8, 8, grid);
}

// Wide fp32 windows as several launches over consecutive column windows of the same stack
// (round 5, tools/probe_slabs.py --windows, profiles/r05/c5/: same stack, same allocation,
// interleaved rounds, two allocations each).  Each window gets its own row-major geometry (grid,
// KG, groups per block), and these splits measured faster than one launch: fused epilogues at
// 16 M+ columns in 3 windows — FedOPT-Adagrad 100 x 86.6 M 5282/5270 -> 5190/5211 us, FedAVGM
// 100 x 86.6 M 5260/5249 -> 5177/5183, FedAVGM 100 x 25.6 M 1561/1564 -> 1542/1544 (2 windows:
// 1574/1572, slower); plain means of 8-16 M columns in 2 — 100 x 11.7 M 666/665 -> 660/661,
// 1000 x 11.7 M 6481/6486 -> 6441/6437 (3 windows: 6545).  The plain mean of 25.6 M (NS) stays
// one launch (2 windows 0.2-0.4% slower), as does 86.6 M (no consistent gain).  Per column the
// sums and epilogue are unchanged: bit-identical results.  Not with a forced grid (ABI 7), and
// fp32 sums only.
inline int window_count(int op, int64_t ncols) {
  if (op != FA_OP_MEAN) return ncols >= ((int64_t)16 << 20) ? 3 : 1;
  return (ncols >= ((int64_t)8 << 20) && ncols < ((int64_t)16 << 20)) ? 2 : 1;
}

// Columns per window of a split into `count`: whole 1-KiB chunks of a row (16-B aligned starts)
inline int64_t window_width(int64_t ncols, int count) {
  return count <= 1 ? ncols : ceil_div(ncols, count) / 256 * 256 + 256;
}

// float16 client stacks (fa_reduce_f16): the one-piece geometry above for an fp32 window of the
// same BYTE width — ~0.75 blocks per CU (up to one per CU instead of a nearly empty second round),
// 4 waves, the narrowest piece (V KiB per wave) that covers the block's share, D = 64/(V*W) rows
// deep, at most 16 (~64 KiB of client rows in flight per block).  Wider windows are swept piece
// after piece (column-major), D = 1.  vmax follows the sums' registers per oct: 4 VGPRs (f16 sums)
// 16, 8 (fp32 sums) 8, 16 (f64 sums) 4.  A window of at most one chunk per block runs as
// single-wave blocks, 16 rows deep.  forced: fa_set_reduce_grid (0 = the geometry chooses); V, W
// and D follow from the share on that grid by the same rule, and a share past the widest piece is
// swept in rounds as on the natural grid.
inline Plan plan_f16_window(int vmax, int64_t ncols, int cus, int forced = 0) {
  const int64_t chunks = row_chunks(ncols, 8);
  const int64_t grid = one_piece_grid(chunks, cus, forced);
  const int64_t share = ceil_div(chunks, grid);  // chunks per block
  const int w = share <= 1 ? 1 : 4;
  int v = 1;
  while (v < vmax && share > v * w) v *= 2;
  const int d = v * w >= kPieceChunks ? 1 : (kPieceChunks / (v * w) > 16 ? 16 : kPieceChunks / (v * w));
  return Plan{kFamRowsH16, v, w, d, 0, 0, false, grid};
}

// 8-byte kinds: one block per chunk up to the resident slots (CUs x the kernel's occupancy)
inline int64_t balanced_grid(int64_t chunks, int64_t slots) {
  const int64_t grid = chunks < slots ? chunks : slots;
  return grid > 0 ? grid : 1;
}

// One chunk of a streamed round (fa_fold): acc_kind FA_ACC_*, the window's columns, on `cus` CUs;
// forced: fa_set_reduce_grid (0 = the geometry chooses).
//   * fp32 client rows (FA_ACC_F32 / _F32_W64): fold_kernel_rows on the one-piece sizing rules of
//     the plain mean — 4 waves, ~0.75 blocks per CU, the narrowest piece (V KiB per wave) that
//     covers the block's share, D = 64/(V*W) rows in flight (V*W*D = 64 KiB per block).  A window
//     just past one round of full pieces takes a few more blocks, up to rows_grid_max (13/16 of the
//     CUs), instead of a nearly empty second round; wider windows are swept piece after piece
//     (column-major, 64-KiB pieces, D = 1) on the natural grid.  The chunk's client count does not
//     enter: the kernel's ramp and drain are correct for any K against D.
//   * 8-byte kinds (FA_ACC_F64 / _I64): fold_kernel_elem, grid-stride, one column per lane, at
//     most 4 blocks per CU.
constexpr int kFoldW = 4;
inline Plan plan_fold_window(int acc_kind, int64_t ncols, int cus, int forced = 0) {
  if (acc_kind == FA_ACC_F64 || acc_kind == FA_ACC_I64) {
    const int64_t blocks = ceil_div(ncols, 256), cap = forced > 0 ? forced : (int64_t)cus * 4;
    return Plan{kFamFoldElem, 1, 4, 1, 0, 0, false, blocks < 1 ? 1 : (blocks < cap ? blocks : cap)};
  }
  const int64_t chunks = row_chunks(ncols);
  int64_t grid = forced > 0 ? forced : natural_grid(cus);
  if (forced <= 0 && chunks > grid * kPieceChunks && chunks <= rows_grid_max(cus) * kPieceChunks)
    grid = ceil_div(chunks, kPieceChunks);
  if (grid > chunks) grid = chunks;
  if (grid < 1) grid = 1;
  const int64_t share = ceil_div(chunks, grid);  // chunks per block
  int v = 1;  // the narrowest piece that covers the share; past one round: full 64-KiB pieces
  while (v < kPieceChunks / kFoldW && share > v * kFoldW) v *= 2;
  return Plan{kFamFoldRows, v, kFoldW, kPieceChunks / (v * kFoldW), 0, 0, false, grid};
}

// Coordinate-wise trimmed sums (fa_trim_sum): a lane sorts its column's clients in registers, so the
// kernel is instantiated per padded depth NP, the smallest of 4, 8, ..., 128 that holds n_clients.
// A block of kTrimW waves owns pieces of 64 * kTrimW consecutive columns (one dword per lane and
// row) and strides over the window's pieces by the grid; the grid is the pieces, at most the
// blocks resident at once: CUs x the waves per SIMD the instantiation's registers allow
// (trim_waves_per_simd, from the compiled VGPR counts in DESIGN.md section 12).
constexpr int kTrimW = 4;
constexpr int kTrimMaxClients = FA_TRIM_MAX_CLIENTS;

struct TrimPlan {
  int np;          // sort slots per lane (0: n_clients out of range)
  int64_t pieces;  // 64 * kTrimW-column pieces of the window
  int64_t grid;
};

inline int trim_np(int n) {
  if (n < 1 || n > kTrimMaxClients) return 0;
  int np = 4;
  while (np < n) np *= 2;
  return np;
}

// waves per SIMD (= 4-wave blocks per CU) each instantiation is compiled for and reaches: 226
// VGPRs at NP = 128, 111 at 64, 53 or fewer below (512 / VGPRs, at most 8); with 3 and 5 the two
// deep ones spill 10 and 1 registers
constexpr int trim_waves_per_simd(int np) { return np >= 128 ? 2 : np >= 64 ? 4 : 8; }

inline TrimPlan plan_trim_window(int n_clients, int64_t n_cols, int cus, int forced_grid) {
  const int np = trim_np(n_clients);
  const int64_t pieces = ceil_div(n_cols, 64 * kTrimW);
  int64_t grid = forced_grid > 0 ? forced_grid : (int64_t)cus * trim_waves_per_simd(np ? np : 4);
  if (grid > pieces) grid = pieces;
  if (grid < 1) grid = 1;
  return TrimPlan{np, pieces, grid};
}

// 8-byte kinds (trim_kernel_elem): grid-stride, one column per lane, at most 4 blocks per CU
inline int64_t trim_elem_grid(int64_t n_cols, int cus, int forced_grid) {
  const int64_t blocks = ceil_div(n_cols, 256), cap = forced_grid > 0 ? forced_grid : (int64_t)cus * 4;
  return blocks < 1 ? 1 : (blocks < cap ? blocks : cap);
}

// The client Gram matrix (fa_gram_f32): G = Y Y^T over a column window, on
// v_mfma_f32_32x32x2_f32.  The kernel is instantiated per padded depth NP, the smallest multiple of
// the 32-row MFMA tile that holds n_clients (32, 64, 96, 128).  A block of 4 waves owns one
// contiguous share of the window, in whole LDS chunks of Kc columns (Kc by NP so that the
// double-buffered tile fills the LDS: gram_kc), the chunks spread evenly over the grid (block b:
// chunks [b * chunks / grid, (b + 1) * chunks / grid)); one block per CU at most, since one tile
// pair takes most of a CU's LDS.  Every kGramLc columns (whole chunks) the MFMA accumulators (the
// inner chain) are added into a second fp32 tile in registers and cleared, so the longest sequence
// of fp32 roundings behind one entry of a block's partial is chain = Lc + ceil(share / Lc): at most
// Lc products in the inner chain, then one add per inner tile.  (A wave sums only its 1/KS of each
// chunk's columns, and the KS waves' tiles are added at the block's end: Lc / KS + ceil(share / Lc)
// + KS - 1 roundings, which is below `chain` for KS in {2, 4}.)  The natural grid keeps
// chain <= 8192 for windows up to 2^25 columns on 64 CUs or more (share <= 2^19 + Kc).
constexpr int kGramMaxClients = FA_GRAM_MAX_CLIENTS;
constexpr int kGramTile = 32;
constexpr int kGramLc = 1024;

struct GramPlan {
  int np;           // padded clients (0: n_clients out of range)
  int kc;           // columns per LDS chunk
  int lc;           // columns per inner chain
  int64_t chunks;   // Kc-column chunks of the window
  int64_t grid;     // blocks = partial tiles in the workspace
  int64_t share;    // the widest block's columns (whole chunks)
  int64_t chain;    // lc + ceil(share / lc)
  int64_t workspace_bytes;  // grid * np * np * 4
};

inline int gram_np(int n) {
  if (n < 1 || n > kGramMaxClients) return 0;
  return (n + kGramTile - 1) / kGramTile * kGramTile;
}

// NP * Kc = 16 Ki floats (96: 12 Ki): two [NP][Kc + 4] fp32 tiles are 132-135 KiB (96: 99) of LDS
constexpr int gram_kc(int np) { return np <= 32 ? 512 : np <= 64 ? 256 : 128; }

inline GramPlan plan_gram_window(int n_clients, int64_t n_cols, int cus, int forced_grid) {
  const int np = gram_np(n_clients);
  const int kc = gram_kc(np ? np : kGramTile);
  const int64_t chunks = ceil_div(n_cols < 1 ? 1 : n_cols, kc);
  int64_t grid = forced_grid > 0 ? forced_grid : cus;
  if (grid > chunks) grid = chunks;
  if (grid < 1) grid = 1;
  const int64_t share = ceil_div(chunks, grid) * kc;
  return GramPlan{np, kc, kGramLc, chunks, grid, share, kGramLc + ceil_div(share, kGramLc),
                  grid * (int64_t)(np ? np : kGramTile) * (np ? np : kGramTile) * 4};
}

// Norm-clipped rounds (fa_rownorm2_f32 / fa_clip_sum_f32).  Both kernels sweep
// the window as fold_kernel_rows does: kFoldW waves, the narrowest piece (V KiB per wave) that covers
// the block's share, D = 64/(V*W) rows in flight.  The clip sum takes plan_fold_window(FA_ACC_F32)
// as it is.  The norms take the same sizing on at most kRownormGridCap blocks (one fp32 partial per
// client and block in the workspace), and the plan, not the kernel, cuts the pieces: `pc` 1-KiB
// chunks per piece, block b sweeping pieces b, b + grid, ..., never more blocks than pieces.
// chain: the longest sequence of fp32 roundings behind one client's partial — V fused multiply-adds
// per element slot of a lane's quads and 2 adds joining the 4 slots, kRownormWaveAdds adds of the
// wave's fixed tree (4 DPP steps inside a row of 16 lanes, then the 4 rows in order), one add per
// piece of the block into the wave's running sum, and W - 1 adds of the waves' sums at the block's
// end.  All terms are squares, so |d2 - d2_ref| <= (gamma(chain) + grid * 2^-52) * d2_ref.
constexpr int kClipMaxClients = FA_CLIP_MAX_CLIENTS;
constexpr int kRownormGridCap = 512;
constexpr int kRownormWaveAdds = 7;

struct RownormPlan {
  int V, W, D;      // quads per lane and piece (0: n_clients out of range), waves, rows in flight
  int64_t chunks;   // 1-KiB chunks of the window
  int64_t pc;       // chunks per piece (<= W * V)
  int64_t pieces;
  int64_t grid;     // blocks = partial rows in the workspace
  int64_t per_block;  // the most pieces one block sweeps
  int64_t chain;
  int64_t workspace_bytes;  // grid * n_clients * 4
};

inline RownormPlan plan_rownorm_window(int n_clients, int64_t n_cols, int cus, int forced_grid) {
  const bool ok = n_clients >= 1 && n_clients <= kClipMaxClients;
  const int64_t chunks = row_chunks(n_cols < 1 ? 1 : n_cols);
  int64_t grid = forced_grid > 0 ? forced_grid : natural_grid(cus);
  if (forced_grid <= 0 && chunks > grid * kPieceChunks && chunks <= rows_grid_max(cus) * kPieceChunks)
    grid = ceil_div(chunks, kPieceChunks);
  if (grid > kRownormGridCap) grid = kRownormGridCap;
  if (grid > chunks) grid = chunks;
  if (grid < 1) grid = 1;
  const int64_t share = ceil_div(chunks, grid);
  int v = 1;
  while (v < kPieceChunks / kFoldW && share > v * kFoldW) v *= 2;
  const int64_t k = ceil_div(chunks, grid * kFoldW * v);  // rounds
  const int64_t pc = ceil_div(chunks, grid * k);
  const int64_t pieces = ceil_div(chunks, pc);
  if (grid > pieces) grid = pieces;
  const int64_t per_block = ceil_div(pieces, grid);
  return RownormPlan{ok ? v : 0, kFoldW, kPieceChunks / (v * kFoldW), chunks, pc, pieces, grid, per_block,
                     v + 2 + kRownormWaveAdds + per_block + kFoldW - 1, grid * (ok ? n_clients : 0) * 4};
}

// What fa_rownorm_workspace returns: enough for any device and any forced grid (a launch has at most
// min(kRownormGridCap, chunks) blocks)
inline int64_t rownorm_workspace_bytes(int n_clients, int64_t n_cols) {
  int64_t blocks = n_cols > (int64_t)kRownormGridCap * 256 ? kRownormGridCap : row_chunks(n_cols < 1 ? 1 : n_cols);
  if (blocks > kRownormGridCap) blocks = kRownormGridCap;
  return blocks * n_clients * 4;
}

// Gaussian noise on an fp32 accumulator (fa_gauss_add_f32): gauss_add_kernel
// is grid-stride over the window's 16-B quads, one quad per lane and step, kNoiseBlock lanes per
// block.  The grid is the blocks that cover the quads once, at most kNoiseBlocksPerCU per CU (the
// kernel's registers leave every wave slot of a CU usable: 8 four-wave blocks) or the forced grid.
// A column's noise is a function of its absolute index alone, so the results do not depend on the
// grid.  steps: the grid-stride steps of the busiest lane.
constexpr int kNoiseBlock = 256;
constexpr int kNoiseBlocksPerCU = 8;

struct NoisePlan {
  int64_t quads;   // 16-B quads of the window, a ragged last one included
  int64_t blocks;  // kNoiseBlock-lane blocks that cover them once
  int64_t grid;
  int64_t steps;
};

inline NoisePlan plan_gauss_add(int64_t n_cols, int cus, int forced_grid) {
  const int64_t quads = n_cols > 0 ? n_cols / 4 + (n_cols % 4 != 0) : 0;  // (no n_cols + 3: it may be INT64_MAX)
  int64_t blocks = quads / kNoiseBlock + (quads % kNoiseBlock != 0);
  if (blocks < 1) blocks = 1;
  const int64_t cap = forced_grid > 0 ? forced_grid : (int64_t)cus * kNoiseBlocksPerCU;
  int64_t grid = blocks < cap ? blocks : cap;
  if (grid < 1) grid = 1;
  return NoisePlan{quads, blocks, grid, ceil_div(blocks, grid)};
}

// The sorting network of trim_kernel_rows: Batcher's odd-even merge sort on NP = 2^q slots, as
// layers (p, k) for p = 1, 2, ..., NP/2 and k = p, p/2, ..., 1, each of up to NP/2 independent
// compare-exchanges.  Candidate m in [0, NP/2) of layer (p, k) is the pair (a, a + k) with
// a = k % p + 2k * (m / k) + m % k; it is part of the network (`on`) when both slots exist and lie
// in the same 2p-block.  1,471 exchanges at NP = 128 (bitonic: 1,792).
struct TrimPair {
  int a, b;
  bool on;
};
constexpr TrimPair trim_net_pair(int np, int p, int k, int m) {
  const int a = k % p + 2 * k * (m / k) + m % k, b = a + k;
  return TrimPair{a, b, b < np && a / (2 * p) == b / (2 * p)};
}

}  // namespace fa
