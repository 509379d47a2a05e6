// fa_sparse.hpp — top-k sparse uploads (fa_sparse_fold_f32): the ordered fp32
// sum of client rows that hold (column, value) pairs instead of N x P codes, in work proportional to
// the pairs.  Two kernels, no atomics across waves, no scratch, the same bits under every grid:
//   * bounds_kernel: one thread per (row, window boundary) binary-searches the row's ascending
//     columns for the first pair at or past the boundary and writes int32 [N][nwin + 1];
//   * window_fold_kernel: each WAVE owns one window of WC consecutive accumulator columns in an LDS
//     tile of its own, fills it with the round's start (the carried sums, wsum times the centre, or
//     +0.0), walks the rows in list order adding each row's pairs of the window into the tile, and
//     stores the tile once.
// A row's columns are strictly ascending, so no two lanes of one step (or of one row) touch one tile
// address; a wave's LDS operations complete in issue order, so rows need no barrier between them.
// Nothing a client sends can move an access: pair loads go through a range-checked row descriptor, a
// lane acts only on a pair inside its segment whose column is inside its window, and the store's
// descriptor ends with the window.  Unsorted or duplicate columns give a meaningless sum, not a fault.
// Included by fa_sparse.hip only.  The kernels live in fa::sparse: the inventories pin the kernels of
// fa, fa::clip and their siblings.
#pragma once

#include "fa_numerics.hpp"

namespace fa {
namespace sparse {

typedef vec4<float>::type XV;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kPadCol = 0xFFFFFFFFu;  // a padding pair's column: past every boundary

// bounds[row][b] = the first pair of `row` whose column is >= min(col0 + b * WC, col0 + ncols),
// b = 0 .. nwin.  A binary search over the row's kpairs pairs (padding pairs hold kPadCol, so a
// boundary never passes them): every probe is inside the row whatever the columns hold.
__global__ __launch_bounds__(256) void bounds_kernel(const uint32_t* __restrict__ pairs, int64_t stride_pairs,
                                                     int kpairs, int n, int64_t col0, int64_t ncols, int wc,
                                                     int64_t nwin, int* __restrict__ bounds) {
  const int64_t per = nwin + 1;
  const int64_t total = (int64_t)n * per;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t row = t / per, b = t - row * per;
    const int64_t rel = b * wc < ncols ? b * wc : ncols;
    const uint64_t target = (uint64_t)(col0 + rel);
    const uint32_t* r = pairs + row * stride_pairs * 2;
    int lo = 0, hi = kpairs;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if ((uint64_t)r[2 * (int64_t)mid] < target) lo = mid + 1; else hi = mid;
    }
    bounds[t] = lo;
  }
}

// One step of one row: the lane's pair p (pair `at + lane` of the row, read as 0 past the row) goes
// into the tile when it lies inside the segment (`at + lane < hi`) and its column inside the window.
// acc = fl32(acc + fl32(a * v)): a multiply and an add, never contracted (-ffp-contract=off).
__device__ __forceinline__ void add_pair(float* tile, u32x2 p, int at, int hi, int lane, uint32_t w0, uint32_t wcols,
                                         float a) {
  const uint32_t rel = p[0] - w0;
  const uint32_t bits = p[1];  // a copy: a bit_cast of the vector element itself reads the vector's first bytes
  if (at + lane < hi && rel < wcols) tile[rel] = tile[rel] + a * __builtin_bit_cast(float, bits);
}

// fa_sparse_fold_f32's second launch.  Block = W waves; wave `wv` of block b sweeps windows
// b * W + wv, + gridDim.x * W, ...  Per window:
//   init   the tile's quads through a range-checked descriptor (columns past the window read 0):
//          acc_in, else fl32(wsum * center), else +0.0;
//   rows   in batches of 64: lane r of the wave loads row (base + r)'s two bounds and its weight — one
//          gathered load per 64 rows, the next batch's issued before this one's rows run — and a row's
//          values reach the scalar unit by readlane, so all control flow is wave-uniform.  Inside a
//          batch the rows' first 64 pairs are loaded D rows ahead in registers (fa_clip.hpp's
//          rows_each: ramp, steady state, drain); a segment longer than 64 pairs takes its further
//          steps four at a time, loads first;
//   store  the tile's quads, 16 B per lane, through a descriptor that ends with the window.
template <int WC, int D, int W>
__global__ __launch_bounds__(64 * W) void window_fold_kernel(const uint32_t* __restrict__ pairs, int64_t stride_pairs,
                                                             int kpairs, int n, const float* __restrict__ weights,
                                                             const float* __restrict__ center, float wsum,
                                                             const float* acc_in, float* acc_out, int64_t col0,
                                                             int64_t ncols, int64_t nwin,
                                                             const int* __restrict__ bounds) {
  static_assert(WC % 256 == 0 && D >= 1 && D <= 16, "a tile is whole steps of 64 quads");
  __shared__ float tiles[W][WC];
  const int lane = (int)threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  float* tile = tiles[wv];
  const int64_t per = nwin + 1;
  const uint32_t row_bytes = (uint32_t)kpairs * 8u;
  for (int64_t w = (int64_t)blockIdx.x * W + wv; w < nwin; w += (int64_t)gridDim.x * W) {
    const int64_t cb = w * WC;  // the window's first column of the launch's [0, ncols)
    const int wcols_i = ncols - cb < WC ? (int)(ncols - cb) : WC;
    const uint32_t wcols = (uint32_t)wcols_i;
    const uint32_t w0 = (uint32_t)(col0 + cb);  // bucket-global, as the pairs' columns are
    // ---- init
    if (acc_in != nullptr) {
      const __amdgpu_buffer_rsrc_t ra = col_rsrc<const float>(acc_in, cb / 4, wcols_i);
#pragma unroll 4
      for (int q = lane; q < WC / 4; q += 64) *reinterpret_cast<XV*>(tile + 4 * q) = buf_load_tquad<float>(ra, q);
    } else if (center != nullptr) {
      const __amdgpu_buffer_rsrc_t rg = col_rsrc<const float>(center + col0, cb / 4, wcols_i);
#pragma unroll 4
      for (int q = lane; q < WC / 4; q += 64) *reinterpret_cast<XV*>(tile + 4 * q) = wsum * buf_load_tquad<float>(rg, q);
    } else {
#pragma unroll 4
      for (int q = lane; q < WC / 4; q += 64) *reinterpret_cast<XV*>(tile + 4 * q) = XV{0.f, 0.f, 0.f, 0.f};
    }
    // ---- rows
    auto batch_load = [&](int base, int& lo, int& hi, float& a) {
      const int r = base + lane;
      lo = hi = 0;
      a = 0.f;
      if (r < n) {
        const int* b = bounds + (int64_t)r * per + w;
        lo = b[0];
        hi = b[1];
        a = weights[r];
      }
    };
    int nlo, nhi;
    float na;
    batch_load(0, nlo, nhi, na);
    for (int base = 0; base < n; base += 64) {
      const int vlo = nlo, vhi = nhi;
      const float va = na;
      if (base + 64 < n) batch_load(base + 64, nlo, nhi, na);
      const int cnt = n - base < 64 ? n - base : 64;
      const char* pn = reinterpret_cast<const char*>(pairs) + (int64_t)base * stride_pairs * 8;  // the next row to load
      u32x2 x[D];
#define FA_SPARSE_LOAD(slot, r)                                                                       \
  {                                                                                                   \
    const int lo_ = __builtin_amdgcn_readlane(vlo, r);                                                \
    x[slot] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(row_rsrc(pn, row_bytes), \
                                                                             (lo_ + lane) * 8, 0, 2)); \
    pn += stride_pairs * 8;                                                                           \
    asm volatile("" : "+s"(pn));                                                                      \
  }
      auto use = [&](int r, u32x2 first) {
        const int lo = __builtin_amdgcn_readlane(vlo, r), hi = __builtin_amdgcn_readlane(vhi, r);
        const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, va), r));
        add_pair(tile, first, lo, hi, lane, w0, wcols, a);
        if (hi - lo > 64) {  // a dense row: the further steps, four loads in flight
          const __amdgpu_buffer_rsrc_t rr =
              row_rsrc(reinterpret_cast<const char*>(pairs) + (int64_t)(base + r) * stride_pairs * 8, row_bytes);
          for (int at = lo + 64; at < hi; at += 256) {
            u32x2 y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
              y[j] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rr, (at + 64 * j + lane) * 8, 0, 2));
#pragma unroll
            for (int j = 0; j < 4; ++j) add_pair(tile, y[j], at + 64 * j, hi, lane, w0, wcols, a);
          }
        }
      };
#pragma unroll
      for (int d = 0; d < D; ++d)
        if (d < cnt) FA_SPARSE_LOAD(d, d)
      int i = 0;
      for (; i + 2 * D <= cnt; i += D) {  // steady state: every refill (row i + d + D) is a real row
#pragma unroll
        for (int d = 0; d < D; ++d) {
          use(i + d, x[d]);
          __builtin_amdgcn_sched_barrier(0);  // consume slot d, then refill it
          FA_SPARSE_LOAD(d, i + d + D)
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {  // drain: fewer than 2*D rows left
        if (i + d < cnt) {
          use(i + d, x[d]);
          if (i + d + D < cnt) FA_SPARSE_LOAD(d, i + d + D)
        }
      }
#pragma unroll
      for (int d = 0; d < D; ++d)
        if (i + D + d < cnt) use(i + D + d, x[d]);
#undef FA_SPARSE_LOAD
    }
    // ---- store
    const __amdgpu_buffer_rsrc_t ro = col_rsrc<float>(acc_out, cb / 4, wcols_i);
#pragma unroll 4
    for (int q = lane; q < WC / 4; q += 64) buf_store_tquad<float>(ro, q, *reinterpret_cast<const XV*>(tile + 4 * q));
  }
}

}  // namespace sparse
}  // namespace fa
