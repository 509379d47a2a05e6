// fa_tune_device.hpp — device code only the tuning tools launch; TOOL, not product.
//
// Included by tools/tune_reduce.hip and tools/tune_rows.hip.  The product header
// (flearn_amd/csrc/fa_device.hpp) holds what fa_reduce.hip launches; the kernels here are earlier
// geometries that lost their measurements (profiles/HISTORY.md §4) and stay as baselines of the
// sweeps: the sub-tile kernels on one-shot and column-blocked grids, their buffer-descriptor form,
// and the row-pointer reduce that claims one piece at a time.
#pragma once

#include "../flearn_amd/csrc/fa_device.hpp"

namespace fa {

// Buffer-descriptor form of a sub-tile (4-byte elements).  Per client row the block builds a
// buffer resource whose base is the row's first quad of this sub-tile and whose num_records is
// the sub-tile's valid byte count; lane offsets (VGPR) are the same for every row and slot v's
// 4-KiB step rides in soffset.  Slots past the valid range are dropped by the hardware range
// check (they return 0, generate no memory request and need no branch), so a partial sub-tile
// issues exactly the loads of its valid quads with the same instruction stream as a full one.
template <class P, typename T, int OP, int V, int U, bool NT>
__device__ __forceinline__ void reduce_subtile_buf(const float* __restrict__ base, int64_t stride,
                                                   int n, const typename P::w_t* __restrict__ w,
                                                   int64_t qt, int nvalid_quads, const Epi<T>& e) {
  typedef typename P::acc_t A;
  typedef typename vec4<float>::type XV;
  typedef typename vec4<A>::type AV;
  const char* tile0 = reinterpret_cast<const char*>(base + qt * 4);
  const uint32_t bytes = (uint32_t)nvalid_quads * 16u;
  const int64_t row_bytes = stride * 4;
  const int voff = (int)threadIdx.x * 16;
  AV acc[V];
  {
    const __amdgpu_buffer_rsrc_t r = row_rsrc(tile0, bytes);
    const typename P::w_t w0 = w[0];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const XV x = buf_load_quad<NT>(r, voff, v * kThreads * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[v][j] = P::mul(w0, x[j]);
    }
  }
  int i = 1;
  for (; i + U <= n; i += U) {
    XV x[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const __amdgpu_buffer_rsrc_t r = row_rsrc(tile0 + (int64_t)(i + u) * row_bytes, bytes);
#pragma unroll
      for (int v = 0; v < V; ++v) x[u][v] = buf_load_quad<NT>(r, voff, v * kThreads * 16);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const typename P::w_t wu = w[i + u];
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[v][j] = add<A>(acc[v][j], P::mul(wu, x[u][v][j]));
    }
  }
  for (; i < n; ++i) {
    const __amdgpu_buffer_rsrc_t r = row_rsrc(tile0 + (int64_t)i * row_bytes, bytes);
    const typename P::w_t wi = w[i];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const XV x = buf_load_quad<NT>(r, voff, v * kThreads * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[v][j] = add<A>(acc[v][j], P::mul(wi, x[j]));
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v)
    if (v * kThreads + (int)threadIdx.x < nvalid_quads)
      finish_quad<T, OP, A>(e, (qt + (int64_t)v * kThreads + threadIdx.x) * 4, 4, acc[v]);
}

// reduce_range_subtile (sub-tile starting at quad qt, limited to quads < qlim) through buffer
// descriptors where BUF is set.
template <class P, typename T, int OP, int V, int U, bool NT, bool BUF>
__device__ __forceinline__ void tune_range_subtile(const typename P::x_t* __restrict__ base, int64_t stride, int n,
                                                   const typename P::w_t* __restrict__ w, int64_t qt,
                                                   int64_t qlim, int64_t ncols, const Epi<T>& e) {
  if constexpr (BUF) {
    static_assert(sizeof(typename P::x_t) == 4, "buffer path is for 4-byte elements");
    constexpr int kSub = kThreads * V;
    const int64_t q0 = qt + threadIdx.x;
    const int64_t qfull = ncols / 4;  // complete quads in the window
    const int64_t end = qt + kSub < qlim ? qt + kSub : qlim;  // this sub-tile's quads [qt, end)
    const int64_t full_end = end < qfull ? end : qfull;
    if (full_end > qt) reduce_subtile_buf<P, T, OP, V, U, NT>(base, stride, n, w, qt, (int)(full_end - qt), e);
    // the window's ragged last quad (ncols % 4 != 0), if it falls in this sub-tile
    if (qfull < end && qfull >= qt && q0 == qt + (qfull - qt) % kThreads)
      reduce_ragged<P, T, OP>(base, stride, n, w, qfull, qfull + 1, ncols, e);
  } else {
    reduce_range_subtile<P, T, OP, V, U, NT>(base, stride, n, w, qt, qlim, ncols, e);
  }
}

// reduce_kernel_balanced's grid over the buffer-descriptor sub-tile.
template <class P, typename T, int OP, int V, int U, bool NT>
__global__ __launch_bounds__(kThreads) void reduce_kernel_balanced_buf(
    const typename P::x_t* __restrict__ stack, int64_t stride, int n,
    const typename P::w_t* __restrict__ w, int64_t col0, int64_t ncols, Epi<T> e) {
  const int64_t nquads = (ncols + 3) / 4;
  const int64_t nchunks = (nquads + 63) / 64;
  const int64_t b = blockIdx.x, g = gridDim.x;
  const int64_t per = nchunks / g, extra = nchunks % g;
  const int64_t c0 = b * per + (b < extra ? b : extra);
  const int64_t c1 = c0 + per + (b < extra ? 1 : 0);
  const int64_t qlim = c1 * 64 < nquads ? c1 * 64 : nquads;
  const typename P::x_t* base = stack + col0;
  for (int64_t qt = c0 * 64; qt < qlim; qt += kThreads * V)
    tune_range_subtile<P, T, OP, V, U, NT, true>(base, stride, n, w, qt, qlim, ncols, e);
}

// One sub-tile per block (grid = number of sub-tiles): the simple mapping.
template <class P, typename T, int OP, int V, int U, bool NT, bool BUF = false>
__global__ __launch_bounds__(kThreads) void reduce_kernel(
    const typename P::x_t* __restrict__ stack, int64_t stride, int n,
    const typename P::w_t* __restrict__ w, int64_t col0, int64_t ncols, Epi<T> e) {
  const int64_t qt = (int64_t)blockIdx.x * (kThreads * V);
  const int64_t nquads = (ncols + 3) / 4;
  tune_range_subtile<P, T, OP, V, U, NT, BUF>(stack + col0, stride, n, w, qt,
                                              qt + kThreads * V < nquads ? qt + kThreads * V : nquads, ncols, e);
}

// Column-blocked client stack: element (n, c) lives at ((c / B) * N + n) * B + c % B with
// B = kThreads*V*4 columns (one tile).  Tile b's N rows are one contiguous N*B*4-byte region, so
// a block streams its whole tile linearly (rows B*4 bytes apart) — the access pattern of a plain
// streaming read.  One tile per block; the window is the whole (padded) bucket.
template <class P, typename T, int OP, int V, int U, bool NT>
__global__ __launch_bounds__(kThreads) void reduce_kernel_blocked(
    const typename P::x_t* __restrict__ stack, int n, const typename P::w_t* __restrict__ w,
    int64_t ncols, Epi<T> e) {
  constexpr int64_t B = (int64_t)kThreads * V * 4;
  const int64_t tile = blockIdx.x;
  const typename P::x_t* base = stack + tile * (int64_t)n * B;
  Epi<T> et = e;
  if (et.out32) et.out32 += tile * B;
  if (et.out64) et.out64 += tile * B;
  if constexpr (OP != FA_OP_MEAN) {
    if (et.prev) et.prev += tile * B;
    if (et.h) et.h += tile * B;
    et.v += tile * B;
  }
  const int64_t cols = ncols - tile * B < B ? ncols - tile * B : B;
  tune_range_subtile<P, T, OP, V, U, NT, (sizeof(typename P::x_t) == 4)>(base, B, n, w, 0, (cols + 3) / 4, cols, et);
}

// Row-pointer reduce, one claimed piece at a time (the form before reduce_kernel_segrows_rm's
// row-major groups; profiles/HISTORY.md §4 row-pointer findings 2-4): pieces come largest first;
// block b starts with piece b and then claims the next unclaimed one from a device counter.
// Wide pieces go through the row pipeline D rows deep, narrow ones (<= W KiB of a row) through a
// one-quad-per-lane sweep V*D rows deep.  The counter must be 0 at launch.
template <class P, typename T, int OP, int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void reduce_kernel_segrows(const float* const* __restrict__ rows, int n,
                                                                const typename P::w_t* __restrict__ w,
                                                                const fa_piece* __restrict__ pieces,
                                                                int64_t npieces, int* __restrict__ next, Epi<T> e) {
  typedef typename P::acc_t A;
  typedef typename vec4<A>::type AV;
  __shared__ int s_next;
  int64_t p = blockIdx.x;
  while (p < npieces) {
    int claimed = 0;
    if (threadIdx.x == 0) claimed = (int)gridDim.x + atomicAdd(next, 1);
    const fa_piece pc = pieces[p];
    const float* const* rp = rows + (int64_t)pc.seg * n;
    // a segment's ragged last quad rides in the vector path: the range check is per dword
    // (`bytes` = exactly the piece's columns), its missing elements load as 0 and are not stored
    const int nq = (pc.n_cols + 3) >> 2;
    const uint32_t bytes = (uint32_t)pc.n_cols * 4u;
    const PtrRows row{rp, pc.seg_off * 4};
    if (nq > 64 * W) {
      AV acc[V];
      rows_sweep<P, V, D, W, NT>(row, bytes, n, w, acc);
      finish_piece<T, OP, A, V, 64 * W, (V >= 2 ? 2 : V)>(e, pc.col / 4, pc.n_cols, acc);
    } else if (nq > 0) {
      AV acc[1];
      rows_sweep<P, 1, V * D, W, NT>(row, bytes, n, w, acc);
      finish_piece<T, OP, A, 1, 64 * W, 1>(e, pc.col / 4, pc.n_cols, acc);
    }
    if (threadIdx.x == 0) s_next = claimed;
    __syncthreads();
    p = s_next;
    __syncthreads();  // s_next is rewritten in the next iteration
  }
}

}  // namespace fa
