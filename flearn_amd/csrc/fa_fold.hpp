// fa_fold.hpp — streamed rounds (fa_fold / fa_fold_finish): the carried-sum row sweep, the fold
// kernels, the finish kernel, and the standalone update (apply_kernel, fa_opt_apply).  Included by
// fa_rows.hip and, through fa_device.hpp, by the tuning tools.
#pragma once

#include "fa_numerics.hpp"

namespace fa {

// ---------------------------------------------------------------------------------------------
// Streamed rounds (fa_fold / fa_fold_finish): a round aggregated in chunks of K clients.  The
// reference's sum is a running one (acc = a0*x0; acc += a_n*x_n in list order, strategy.py:123-126),
// so a typed accumulator carried from one chunk's launch to the next holds, after the last chunk,
// exactly the bits the single launch's register sum held; the divide and the server update
// (strategy.py:127-129, avgm.py / opt.py / dyn.py) need the whole weight list and run once, in
// fold_finish_kernel, through the same epi_compute the fused epilogues call.
// ---------------------------------------------------------------------------------------------

// rows_sweep for a sum that may be carried in.  first (block-uniform): no sum yet, row 0's product
// initialises it (so -0.0 survives) and the pipeline starts at row 1, exactly rows_sweep; else acc
// holds the carried sum and every row 0..n-1 is added to it.  The pipeline's slot d holds row
// i + d from the first row s on; n may be smaller than D (chunks are short): the ramp loads only
// real rows and the drain's branches are wave-uniform.  Rows are loaded in strictly increasing
// order through all three phases, so the row address is ONE running scalar pointer (opaque to the
// compiler, as in reduce_kernel_narrow: written as tile0 + (i + d + D) * row_bytes in the unrolled
// loops, every d * row_bytes was kept in a scalar register pair and D = 16 spilled 30 of them).
template <class P, int V, int D, int W, bool NT>
__device__ __forceinline__ void rows_fold_sweep(const char* tile0, int64_t row_bytes, uint32_t bytes, int n,
                                                const typename P::w_t* __restrict__ w,
                                                typename vec4<typename P::acc_t>::type (&acc)[V], bool first) {
  typedef typename vec4<float>::type XV;
  const int voff = (int)threadIdx.x * 16;
  const int s = first ? 1 : 0;
  const char* pn = tile0 + (int64_t)s * row_bytes;  // the next row to load
#define FA_FOLD_LOAD(slot)                                                                        \
  {                                                                                               \
    const __amdgpu_buffer_rsrc_t r_ = row_rsrc(pn, bytes);                                        \
    _Pragma("unroll") for (int v = 0; v < V; ++v) x[slot][v] = buf_load_quad<NT>(r_, voff + v * 64 * W * 16, 0); \
    pn += row_bytes;                                                                              \
    asm volatile("" : "+s"(pn));                                                                  \
  }
  XV x[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (s + d < n) FA_FOLD_LOAD(d)
  if (first) {
    const __amdgpu_buffer_rsrc_t r = row_rsrc(tile0, bytes);
    const typename P::w_t w0 = w[0];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = quad_mul<P>(w0, buf_load_quad<NT>(r, voff + v * 64 * W * 16, 0));
  }
  int i = s;
  for (; i + 2 * D <= n; i += D) {  // steady state: every refill (row i + d + D) is a real row
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const typename P::w_t wi = w[i + d];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = quad_axpy<P>(acc[v], wi, x[d][v]);
      __builtin_amdgcn_sched_barrier(0);  // consume slot d, then refill it (see rows_sweep)
      FA_FOLD_LOAD(d)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {  // drain: fewer than 2*D rows left
    if (i + d < n) {
      const typename P::w_t wi = w[i + d];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = quad_axpy<P>(acc[v], wi, x[d][v]);
      if (i + d + D < n) FA_FOLD_LOAD(d)
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (i + D + d < n) {
      const typename P::w_t wi = w[i + D + d];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = quad_axpy<P>(acc[v], wi, x[d][v]);
    }
  }
#undef FA_FOLD_LOAD
}

// fa_fold for fp32 client rows (FA_ACC_F32 / FA_ACC_F32_W64): reduce_kernel_rows' work split (equal
// interleaved pieces of pc <= W*V 1-KiB chunks, block b sweeping pieces b, b+grid, ...), per-row
// range-checked descriptors, the window's ragged last quad covered by the range.  The piece's
// carried sums are loaded once before the sweep and stored once after it, whole 16-B units per
// lane through descriptors whose range is the piece's columns (lanes past the end load 0 and
// their stores are dropped).  acc_out may be acc_in: a lane reads its quads before it writes them
// and no other lane touches them.  acc_in == NULL: the chunk is the round's first.
template <class P, int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void fold_kernel_rows(const float* __restrict__ stack, int64_t stride, int n,
                                                           const typename P::w_t* __restrict__ w,
                                                           const typename P::acc_t* acc_in,
                                                           typename P::acc_t* acc_out, int64_t col0, int64_t ncols) {
  static_assert(sizeof(typename P::x_t) == 4, "row pipeline is for 4-byte elements");
  typedef typename P::acc_t A;
  typedef typename vec4<A>::type AV;
  const int64_t nquads = (ncols + 3) / 4;
  const int64_t chunks = (nquads + 63) / 64;
  const int64_t g = gridDim.x;
  const int64_t k = (chunks + g * W * V - 1) / (g * W * V);  // rounds
  const int64_t pc = (chunks + g * k - 1) / (g * k);         // chunks per piece (<= W*V)
  const int64_t pieces = (chunks + pc - 1) / pc;
  const bool first = acc_in == nullptr;
  for (int64_t p = blockIdx.x; p < pieces; p += g) {
    const int64_t qb = p * pc * 64;
    const int64_t qe = qb + pc * 64 < nquads ? qb + pc * 64 : nquads;
    const int64_t cend = qe * 4 < ncols ? qe * 4 : ncols;
    const int cols = cend > qb * 4 ? (int)(cend - qb * 4) : 0;
    if (cols <= 0) continue;
    AV acc[V];
    if (!first) {
      const __amdgpu_buffer_rsrc_t ra = col_rsrc<const A>(acc_in, qb, cols);
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = buf_load_tquad<A>(ra, (int)threadIdx.x + v * 64 * W);
    }
    rows_fold_sweep<P, V, D, W, NT>(reinterpret_cast<const char*>(stack + col0 + qb * 4), stride * 4,
                                    (uint32_t)cols * 4u, n, w, acc, first);
    const __amdgpu_buffer_rsrc_t ro = col_rsrc<A>(acc_out, qb, cols);
#pragma unroll
    for (int v = 0; v < V; ++v) buf_store_tquad<A>(ro, (int)threadIdx.x + v * 64 * W, acc[v]);
  }
}

// fa_fold for the 8-byte kinds (FA_ACC_F64 / FA_ACC_I64: float64 buffers, BN counters; small
// buckets): one column per lane at a time, grid-stride, rows in list order.
template <class P>
__global__ __launch_bounds__(kThreads) void fold_kernel_elem(const typename P::x_t* __restrict__ stack, int64_t stride,
                                                             int n, const typename P::w_t* __restrict__ w,
                                                             const typename P::acc_t* acc_in,
                                                             typename P::acc_t* acc_out, int64_t col0, int64_t ncols) {
  typedef typename P::acc_t A;
  for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * kThreads) {
    const typename P::x_t* x = stack + col0 + c;
    A acc;
    int i = 0;
    if (acc_in) {
      acc = acc_in[c];
    } else {
      acc = P::mul(w[0], x[0]);
      i = 1;
    }
    for (; i < n; ++i) acc = add<A>(acc, P::mul(w[i], x[(int64_t)i * stride]));
    acc_out[c] = acc;
  }
}

// fa_fold_finish: the divide and the optional server update over a finished accumulator, one quad
// per lane; the arithmetic and the stores are finish_quad's (epi_compute / update), the ones the
// fused epilogues run.  acc is 16-B aligned: an 8-byte quad is read as two 16-B halves.
template <typename A, typename T, int OP>
__global__ __launch_bounds__(kThreads) void fold_finish_kernel(const A* __restrict__ acc, int64_t n, Epi<T> e) {
  const int64_t c = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (c >= n) return;
  const int valid = (int)((n - c) < 4 ? (n - c) : 4);
  typename vec4<A>::type a;
  if (valid == 4) {
    if constexpr (sizeof(A) == 4) {
      a = *reinterpret_cast<const typename vec4<A>::type*>(acc + c);
    } else {
      typedef A a2 __attribute__((ext_vector_type(2)));
      const a2 lo = *reinterpret_cast<const a2*>(acc + c), hi = *reinterpret_cast<const a2*>(acc + c + 2);
      a = typename vec4<A>::type{lo[0], lo[1], hi[0], hi[1]};
    }
  } else {
    a = load_quad_guarded(acc + c, valid);
  }
  finish_quad<T, OP, A>(e, c, valid, a);
}

// Standalone update (client_receive form): g read from memory instead of reduced.
template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void apply_kernel(const T* __restrict__ glob, int64_t n,
                                                         Epi<T> e) {
  const int64_t c = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (c >= n) return;
  const int valid = (int)((n - c) < 4 ? (n - c) : 4);
  typename vec4<T>::type g = load_quad_guarded(glob + c, valid);
  finish_quad<T, OP, T>(e, c, valid, g);  // denom == 1: T(g)/1 == g exactly
}

}  // namespace fa
