// fa_gramwide.hpp — the client Gram matrix of 129 .. 1024 clients (fa_gram_f32_wide, DESIGN.md
// section 24): panel_pair_kernel, one block per (column slice, pair of 128-row panels), and
// panel_finish_kernel, which sums the slices' partial tiles in float64.  Included by fa_gramwide.hip
// and by tools/tune_gramwide.hip.  In a namespace of its own, as fa_trimwide.hpp: gram_kernel_tile
// (fa_gram.hpp) stays the kernel of up to 128 clients.
#pragma once

#include <type_traits>

#include "fa_gramwide_geometry.hpp"
#include "fa_numerics.hpp"

namespace fa {
namespace gramwide {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPanel = kGramWidePanel, kKc = kGramWideKc, kLc = kGramLc;
constexpr int kPitch = kKc + 4;             // floats; 4 mod 64: conflict-free b128 reads, as gram_kernel_tile's
constexpr int kTileFloats = kPanel * kPitch;  // one operand tile [128][Kc + 4]: 34 KiB, 4 of them 136 KiB
constexpr int kRpw = kPanel / 4;            // rows per wave and panel: wave, wave + 4, ...
static_assert(kKc == 64, "one row of a chunk is one dword per lane of a wave");
static_assert(kLc % kKc == 0 && (4 * kTileFloats / 4) % 256 == 0, "whole chunks per inner chain; an even clear");

// The order in which the grid's blocks take the (slice, pair) units (measured against each other by
// tools/tune_gramwide.hip)
enum : int {
  kSliceMajorXcd = 0,  // slice-major, and the blocks one XCD receives (every 8th) take consecutive units
  kSliceMajor = 1,     // unit = block: the pairs of a slice on consecutive blocks, spread over the XCDs
  kPairMajor = 2,      // shipped: the slices of a pair on consecutive blocks
};

__device__ __forceinline__ void unit_of(int b, int grid, int pairs, int order, int& slice, int& pair) {
  if (order == kPairMajor) {
    const int slices = grid / pairs;
    pair = b / slices;
    slice = b % slices;
    return;
  }
  int v = b;
  if (order == kSliceMajorXcd) {  // block b runs on XCD b % 8: XCD x takes the units [x * grid / 8 ..), in order
    const int x = b & 7, base = grid >> 3, rem = grid & 7;
    v = x * base + (x < rem ? x : rem) + (b >> 3);
  }
  slice = v / pairs;
  pair = v % pairs;
}

// How a block spreads a pair's 32 x 32 tiles over its 4 waves.  An off-diagonal pair has all 16
// tiles: wave a takes the tiles (a, 0..3), one A read feeding 4 B reads, so every SIMD issues the same
// number of MFMAs on 4 independent accumulators.  A diagonal pair (I == J) has the 10 upper tiles of
// one panel, numbered (0,0), (0,1), ..., (0,3), (1,1), ...: waves 0 and 1 take 3 each, waves 2 and 3
// take 2.  An even split of 10 tiles over 4 waves would cut a tile's columns between two waves, as
// gram_kernel_tile<128> does, and an entry's arithmetic would then depend on the kind of pair it
// falls into; a permutation of the rows moves entries from one kind to the other, so everywhere an
// entry is one k-ordered chain over the whole chunk, and the diagonal pairs (at most 8 of 36) run at
// 3 tiles' time for 2.5 tiles' work per wave.
template <bool DIAG>
struct PairShape {
  static constexpr int TPW = DIAG ? 3 : 4;
};

// One chunk of one wave's rows of a panel into registers: row wave + 4 i through its own
// range-checked descriptor whose range is the chunk's valid bytes, so a ragged window end loads 0 and
// no address past the window is formed into a fetch; one 256-B row piece per wave instruction.  Rows
// >= rows (the panel's real rows) are not loaded (wave-uniform) and stay zero in LDS.
__device__ __forceinline__ void panel_load(float (&st)[kRpw], const char* p, int64_t row_bytes, int wave, int rows,
                                           uint32_t bytes, int lane) {
  asm volatile("" : "+s"(rows));  // as gram_load: the conditions are made per chunk, not kept across the loop
#pragma unroll
  for (int i = 0; i < kRpw; ++i) {
    if (wave + 4 * i < rows)
      st[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(row_rsrc(p, bytes), lane * 4, 0, 0));
    p += 4 * row_bytes;
    asm volatile("" : "+s"(p));
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <bool CEN>
__device__ __forceinline__ void panel_stage(float* __restrict__ tile, const float (&st)[kRpw], float cs, int wave,
                                            int rows, int lane) {
  asm volatile("" : "+s"(rows));
#pragma unroll
  for (int i = 0; i < kRpw; ++i)
    if (wave + 4 * i < rows) tile[(wave + 4 * i) * kPitch + lane] = CEN ? st[i] - cs : st[i];
}

// One (slice, pair) unit.  lds: 2 buffers of [A tile][B tile] (a diagonal pair uses A alone), zeroed
// by the caller; rows_a / rows_b: the panels' real rows (1 .. 128).  Per chunk the 4 waves load the
// panels' rows into registers while the previous chunk is multiplied, then write them, centred, into
// the other buffer; one barrier per chunk.  For the tile (a, b) lane l reads 16 B of row 32 a + (l & 31)
// of A and of row 32 b + (l & 31) of B at column 8 g + 4 (l >> 5) of the chunk and issues 4
// MFMAs, element s of both reads being step s: the same columns in both operands, in an order fixed
// by the plan.  After kLc columns of the slice the inner accumulators are added into the outer fp32
// tile and cleared.  Tiles of padded rows only (a >= tiles_a or b >= tiles_b) are neither multiplied
// nor stored.  The block stores its tiles to `out` ([128][128] floats, row from the A panel; C/D map:
// col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  No atomics.
template <bool DIAG, bool CEN>
__device__ __forceinline__ void pair_body(float* __restrict__ lds, const float* __restrict__ pa,
                                          const float* __restrict__ pb, const float* __restrict__ pc, int64_t stride,
                                          int rows_a, int rows_b, int64_t ncols, int64_t cb, int64_t ce,
                                          float* __restrict__ out) {
  using S = PairShape<DIAG>;
  const int tid = (int)threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_a = (rows_a + kGramTile - 1) / kGramTile, tiles_b = (rows_b + kGramTile - 1) / kGramTile;

  // the wave's tiles: diagonal, numbers first .. first + 2 (waves 2, 3: + 1) of the upper tiles; else (wave, t)
  int ta[S::TPW], tb[S::TPW], aoff[S::TPW], boff[S::TPW];
  unsigned act = 0;  // bit t: the tile has real rows on both sides
#pragma unroll
  for (int t = 0; t < S::TPW; ++t) {
    int a = wave, b = t;
    if constexpr (DIAG) {
      int rem = (wave < 2 ? 3 * wave : 2 + 2 * wave) + t;
      a = 0;
      while (a < 3 && rem >= 4 - a) {  // (waves 2 and 3: t == 2 names no tile and stays inactive)
        rem -= 4 - a;
        ++a;
      }
      b = a + rem;
    }
    ta[t] = a;
    tb[t] = b;
    aoff[t] = (32 * a + (lane & 31)) * kPitch + 4 * half;
    boff[t] = (DIAG ? 0 : kTileFloats) + (32 * b + (lane & 31)) * kPitch + 4 * half;
    if (a < tiles_a && b < tiles_b && !(DIAG && wave >= 2 && t == 2)) act |= 1u << t;
  }
  act = __builtin_amdgcn_readfirstlane(act);
  f32x16 inner[S::TPW], outer[S::TPW];
#pragma unroll
  for (int t = 0; t < S::TPW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) inner[t][r] = outer[t][r] = 0.f;

  const int64_t row_bytes = stride * 4;
  float sa[kRpw], sb[DIAG ? 1 : kRpw], cs = 0.f;
  auto fetch = [&](int64_t c) {
    const int64_t c0 = c * kKc;
    const uint32_t bytes = (uint32_t)(ncols - c0 < kKc ? ncols - c0 : kKc) * 4u;
    panel_load(sa, reinterpret_cast<const char*>(pa + c0) + wave * row_bytes, row_bytes, wave, rows_a, bytes, lane);
    if constexpr (!DIAG)
      panel_load(sb, reinterpret_cast<const char*>(pb + c0) + wave * row_bytes, row_bytes, wave, rows_b, bytes, lane);
    if constexpr (CEN)
      cs = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(row_rsrc(pc + c0, bytes), lane * 4, 0, 0));
  };
  auto stage = [&](float* buf) {
    panel_stage<CEN>(buf, sa, cs, wave, rows_a, lane);
    if constexpr (!DIAG) panel_stage<CEN>(buf + kTileFloats, sb, cs, wave, rows_b, lane);
  };
  // one chunk's products; FULL: every tile of the wave is real, no condition in the stream of MFMAs
  auto multiply = [&](const float* cur, auto full) {
#pragma unroll
    for (int g = 0; g < kKc / 8; ++g) {
#pragma unroll
      for (int t = 0; t < S::TPW; ++t) {
        if constexpr (!decltype(full)::value)
          if (!(act >> t & 1)) continue;
        const f32x4 a = *reinterpret_cast<const f32x4*>(cur + aoff[t] + 8 * g);
        const f32x4 b = *reinterpret_cast<const f32x4*>(cur + boff[t] + 8 * g);
#pragma unroll
        for (int s = 0; s < 4; ++s) inner[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], inner[t], 0, 0, 0);
      }
    }
  };

  fetch(cb);
  stage(lds);
  __syncthreads();
  int run = 0;  // columns of the slice in the inner chain
  for (int64_t c = cb; c < ce; ++c) {
    const float* cur = lds + ((c - cb) & 1) * (2 * kTileFloats);
    float* nxt = lds + (((c - cb) & 1) ^ 1) * (2 * kTileFloats);
    const bool more = c + 1 < ce;
    if (more) fetch(c + 1);
    if (act == (1u << S::TPW) - 1)
      multiply(cur, std::true_type{});
    else
      multiply(cur, std::false_type{});
    run += kKc;
    if (run >= kLc || !more) {
#pragma unroll
      for (int t = 0; t < S::TPW; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          outer[t][r] += inner[t][r];
          inner[t][r] = 0.f;
        }
      }
      run = 0;
    }
    if (more) stage(nxt);
    // one barrier per chunk: `nxt` was last read before the previous barrier, `cur` is next
    // written after this one
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < S::TPW; ++t) {
    if (act >> t & 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * ta[t] + (r & 3) + 8 * (r >> 2) + 4 * half, col = 32 * tb[t] + (lane & 31);
        out[row * kPanel + col] = outer[t][r];
      }
    }
  }
}

// fp32 rows, 129 <= n <= 1024 clients in `panels` panels, 256 threads, grid = slices * pairs blocks
// (plan_gram_wide).  Block b takes the unit unit_of(b) names: the chunks [cb, ce) of the window for
// the panel pair (I, J), and stores its partial to slot slice * pairs + pair of `partials`.
template <bool CEN>
__global__ __launch_bounds__(256) void panel_pair_kernel(const float* __restrict__ stack, int64_t stride, int n,
                                                         const float* __restrict__ center, int64_t col0, int64_t ncols,
                                                         int64_t chunks, int slices, int panels, int order,
                                                         float* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float lds[4 * kTileFloats];
  for (int i = (int)threadIdx.x; i < 4 * kTileFloats / 4; i += 256)
    reinterpret_cast<f32x4*>(lds)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int pairs = panels * (panels + 1) / 2;
  int slice, pair;
  unit_of((int)blockIdx.x, (int)gridDim.x, pairs, order, slice, pair);
  int I = 0, J = pair;  // pair number -> (I, J), I <= J
  while (J >= panels - I) {
    J -= panels - I;
    ++I;
  }
  J += I;
  const int rows_a = n - kPanel * I < kPanel ? n - kPanel * I : kPanel;
  const int rows_b = n - kPanel * J < kPanel ? n - kPanel * J : kPanel;
  const int64_t cb = (int64_t)slice * chunks / slices, ce = ((int64_t)slice + 1) * chunks / slices;
  const float* pa = stack + (int64_t)kPanel * I * stride + col0;
  const float* pb = stack + (int64_t)kPanel * J * stride + col0;
  const float* pc = CEN ? center + col0 : nullptr;
  float* out = partials + ((int64_t)slice * pairs + pair) * (kPanel * kPanel);
  __syncthreads();  // the zeros are in place
  if (I == J)
    pair_body<true, CEN>(lds, pa, pb, pc, stride, rows_a, rows_b, ncols, cb, ce, out);
  else
    pair_body<false, CEN>(lds, pa, pb, pc, stride, rows_a, rows_b, ncols, cb, ce, out);
}

// G[i][j] (float64, [n][n]) = the slices' partials of the entry, converted and added in slice order;
// the entry is read at (min(i, j), max(i, j)) — the pair (I <= J) that holds it, and inside a
// diagonal pair the upper triangle — so G[i][j] and G[j][i] are the same bits.
__global__ __launch_bounds__(256) void panel_finish_kernel(const float* __restrict__ partials, int slices, int panels,
                                                           int n, double* __restrict__ gram_out) {
  const int idx = (int)(blockIdx.x * 256 + threadIdx.x);
  if (idx >= n * n) return;
  const int i = idx / n, j = idx % n, lo = i < j ? i : j, hi = i < j ? j : i;
  const int I = lo / kPanel, J = hi / kPanel, pairs = panels * (panels + 1) / 2;
  const int pair = I * panels - I * (I - 1) / 2 + (J - I);
  const float* p = partials + (int64_t)pair * (kPanel * kPanel) + (lo % kPanel) * kPanel + hi % kPanel;
  double s = 0.0;
  for (int b = 0; b < slices; ++b) s += (double)p[(int64_t)b * pairs * (kPanel * kPanel)];
  gram_out[idx] = s;
}

}  // namespace gramwide
}  // namespace fa
