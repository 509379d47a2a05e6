// fa_segrows.hpp — the row-pointer side: the segmented reduce over per-client tensors where they
// lie (reduce_kernel_segrows_rm) and the gather kernels that copy them into a stack.  Included by
// fa_rows.hip only among the product's units (gather_rows_f64_kernel is no template and may be
// defined once per library) and, through fa_device.hpp, by the tuning tools.
#pragma once

#include "fa_numerics.hpp"

namespace fa {

// Segmented row-pointer reduce (fa_reduce_f32_rows): uploads that are separate device tensors
// per (client, key) are read where they lie — no pack copy.  Work = pieces (fa_rows_plan): each
// is a column range of ONE segment, so every row of a piece is one contiguous range of one
// tensor and gets one buffer descriptor; client order and epilogue are the row pipeline's.
//   * a claim is a GROUP of KG wide pieces (the leading pieces[0].aux entries of the
//     largest-first table) swept together row by row — step (row i, piece j), j fastest, one step
//     (V*W KiB) in flight, like reduce_kernel_rowmajor — so the blocks stay on neighbouring client
//     rows as the stack kernel's do; the row pointer of the step after the next one is fetched
//     while the next is in flight (every index is static: j is unrolled);
//   * scheduling: block b starts with claim b and then takes the next unclaimed one from a device
//     counter.  Blocks finish within about one small piece of each other whatever the mix of
//     tensor sizes — a static split of 100 ResNet-sized uploads left a ~10% tail
//     (tools/tune_rows.py);
//   * claims past the groups are the narrow pieces (<= W KiB of a row: BN vectors, biases), one at
//     a time.  They are latency-bound, not bandwidth-bound, and take a one-quad-per-lane sweep DN
//     rows deep, so a 64-element tensor of 100 clients costs ~7 HBM round trips instead of ~50.
// The counter must be 0 at launch (the host clears it on the stream before each launch).
// TR (tools/tune_rows.hip): wave 0 of every block stamps the 100-MHz wall clock at each claim it
// starts (e.trace[block * 32 + 1 + c], c < 30) and at its exit (slot 0), claim count in slot 31.
// XLS: the epilogue's f64 stores as whole cache lines (buf_store_tquad XL, 2 KiB of LDS per wave),
// as rowmajor_group does for fused epilogues at KG <= 3 (DESIGN.md §4 finding 22).
// Dead ends, measured and removed (profiles/HISTORY.md §4, "row-pointer" findings):
//   * one claimed piece at a time, column-major (kept in tools/fa_tune_device.hpp): finding 4;
//   * two or more steps in flight: finding 8;
//   * static groups in lockstep, claiming only the narrow pieces: finding 9;
//   * a one-dword translation prefetch some steps ahead: finding 11;
//   * the group's row pointers staged in LDS: §10 item 4.
template <class P, typename T, int OP, int V, int W, int KG, int DN, bool NT, bool TR = false, bool XLS = false>
__global__ __launch_bounds__(64 * W) void reduce_kernel_segrows_rm(const float* const* __restrict__ rows, int n,
                                                                   const typename P::w_t* __restrict__ w,
                                                                   const fa_piece* __restrict__ pieces,
                                                                   int64_t npieces, int* __restrict__ next, Epi<T> e) {
  typedef typename P::acc_t A;
  typedef typename vec4<A>::type AV;
  typedef typename vec4<float>::type XV;
  __shared__ int s_next;
  const int64_t nwide = npieces > 0 ? pieces[0].aux : 0;
  const int64_t groups = (nwide + KG - 1) / KG;
  const int64_t claims = groups + (npieces - nwide);
  const int voff = (int)threadIdx.x * 16;
  int64_t t = blockIdx.x;
  int nclaim = 0;
  const int64_t nbase = gridDim.x;  // claims are numbered from the grid's size on
#define FA_SRM_CLAIM() ((int)nbase + atomicAdd(next, 1))
  while (t < claims) {
    // the next claim: a group (hundreds of us) claims during its last row, so an idle block can
    // take what is left meanwhile (claiming at the start reserved work behind a long group while
    // blocks that had drawn short pieces ran dry: tools/tune_rows.py --trace); a narrow piece
    // claims at its start, which hides the atomic behind its short sweep
    int claimed = 0;
    if (t >= groups && threadIdx.x == 0) claimed = FA_SRM_CLAIM();
    if constexpr (TR) {
      if (threadIdx.x == 0 && nclaim < 30) e.trace[blockIdx.x * 32 + 1 + nclaim] = wall_clock64();
      ++nclaim;
    }
    if (t < groups) {
      const float* const* rp[KG];
      int64_t ob[KG], col[KG];
      int cols[KG];
      uint32_t bytes[KG];
#pragma unroll
      for (int j = 0; j < KG; ++j) {
        const int64_t pi = t * KG + j;
        const fa_piece pc = pi < nwide ? pieces[pi] : fa_piece{0, 0, 0, 0, 0};
        rp[j] = rows + (int64_t)pc.seg * n;  // a missing piece keeps segment 0's pointers, 0 bytes
        ob[j] = pc.seg_off * 4;
        col[j] = pc.col;
        cols[j] = pc.n_cols;
        bytes[j] = (uint32_t)pc.n_cols * 4u;
      }
      // row pointer of step (i, j); rows clamped (a step past the end is never loaded)
#define FA_SRM_PTR(i, j) (reinterpret_cast<const char*>(rp[j][(i) < n ? (i) : n - 1]) + ob[j])
#define FA_SRM_LOAD(p, j)                                                                              \
  {                                                                                                    \
    const __amdgpu_buffer_rsrc_t r_ = row_rsrc((p), bytes[j]);                                         \
    _Pragma("unroll") for (int v = 0; v < V; ++v) x[v] = buf_load_quad<NT>(r_, voff + v * 64 * W * 16, 0); \
  }
      AV acc[KG][V];
      XV x[V];
      // the first step.  (A one-trip loop on purpose: written as a plain statement the sweep is
      // scheduled differently — same registers, other instruction order — and every measurement
      // of this kernel was taken on the code this form compiles to.)
      for (int d = 0; d < 1; ++d) FA_SRM_LOAD(FA_SRM_PTR(d, 0), 0);
      const char* pn = FA_SRM_PTR(1 / KG, 1 % KG);  // the pointer of the next step to load
      // after consuming step (i, j): load the next step, then fetch the pointer of the one after it
#define FA_SRM_REFILL(i, j)                                        \
  __builtin_amdgcn_sched_barrier(0);                               \
  if ((i) + ((j) + 1) / KG < n) {                                  \
    FA_SRM_LOAD(pn, ((j) + 1) % KG);                               \
    pn = FA_SRM_PTR((i) + ((j) + 2) / KG, ((j) + 2) % KG);         \
  }                                                                \
  __builtin_amdgcn_sched_barrier(0);
      {  // row 0: the products initialise the sums (peeled: a select between the first product
         // and the running sum kept both alive for every slot and spilled KG >= 3)
        const typename P::w_t w0 = w[0];
        if (n == 1 && threadIdx.x == 0) claimed = FA_SRM_CLAIM();
#pragma unroll
        for (int j = 0; j < KG; ++j) {
#pragma unroll
          for (int v = 0; v < V; ++v) acc[j][v] = quad_mul<P>(w0, x[v]);
          FA_SRM_REFILL(0, j)
        }
      }
      for (int i = 1; i < n; ++i) {
        if (i == n - 1 && threadIdx.x == 0) claimed = FA_SRM_CLAIM();
        const typename P::w_t wi = w[i];
#pragma unroll
        for (int j = 0; j < KG; ++j) {
#pragma unroll
          for (int v = 0; v < V; ++v) acc[j][v] = quad_axpy<P>(acc[j][v], wi, x[v]);
          FA_SRM_REFILL(i, j)
        }
      }
#undef FA_SRM_REFILL
#undef FA_SRM_LOAD
#undef FA_SRM_PTR
#pragma unroll
      for (int j = 0; j < KG; ++j) finish_piece<T, OP, A, V, 64 * W, (V >= 2 ? 2 : V), XLS>(e, col[j] / 4, cols[j], acc[j]);
    } else {
      const fa_piece pc = pieces[nwide + (t - groups)];
      const float* const* rp = rows + (int64_t)pc.seg * n;
      const uint32_t bytes = (uint32_t)pc.n_cols * 4u;
      const PtrRows row{rp, pc.seg_off * 4};
      if (((pc.n_cols + 3) >> 2) > 64 * W) {  // a wide piece the groups did not take
        AV acc[V];
        rows_sweep<P, V, 1, W, NT>(row, bytes, n, w, acc);
        finish_piece<T, OP, A, V, 64 * W, (V >= 2 ? 2 : V), XLS>(e, pc.col / 4, pc.n_cols, acc);
      } else if (pc.n_cols > 0) {
        AV acc[1];
        rows_sweep<P, 1, DN, W, NT>(row, bytes, n, w, acc);
        finish_piece<T, OP, A, 1, 64 * W, 1, XLS>(e, pc.col / 4, pc.n_cols, acc);
      }
    }
    if (threadIdx.x == 0) s_next = claimed;
    __syncthreads();
    t = s_next;
    __syncthreads();
  }
#undef FA_SRM_CLAIM
  if constexpr (TR) {
    if (threadIdx.x == 0) {
      e.trace[blockIdx.x * 32] = wall_clock64();
      e.trace[blockIdx.x * 32 + 31] = (unsigned long long)nclaim;
    }
  }
}

// fa_gather_rows: block (s, i) copies client i's tensor of segment s into its stack row.
template <typename E>
__global__ __launch_bounds__(kThreads) void gather_rows_kernel(E* __restrict__ stack, int64_t stride, int n,
                                                               const E* const* __restrict__ rows,
                                                               const int64_t* __restrict__ segs, int nseg, int i0) {
  const int s = blockIdx.x, i = i0 + (int)blockIdx.y;  // i0: client tile (grid.y <= 65535)
  const int64_t col = segs[s], len = segs[nseg + s];
  const E* src = rows[(int64_t)s * n + i];
  E* dst = stack + (int64_t)i * stride + col;
  for (int64_t k = threadIdx.x; k < len; k += kThreads) dst[k] = src[k];
}

// fa_gather_rows_f64: the same into a float64 stack, segment s's source converted by kind
// (segs[2*nseg + s]: FA_SRC_F64 copy, FA_SRC_I64 int64 -> double rounded to nearest, FA_SRC_F32).
__global__ __launch_bounds__(kThreads) void gather_rows_f64_kernel(double* __restrict__ stack, int64_t stride, int n,
                                                                   const void* const* __restrict__ rows,
                                                                   const int64_t* __restrict__ segs, int nseg, int i0) {
  const int s = blockIdx.x, i = i0 + (int)blockIdx.y;
  const int64_t col = segs[s], len = segs[nseg + s], kind = segs[2 * nseg + s];
  const void* src = rows[(int64_t)s * n + i];
  double* dst = stack + (int64_t)i * stride + col;
  if (kind == FA_SRC_I64) {
    const int64_t* x = static_cast<const int64_t*>(src);
    for (int64_t k = threadIdx.x; k < len; k += kThreads) dst[k] = (double)x[k];
  } else if (kind == FA_SRC_F32) {
    const float* x = static_cast<const float*>(src);
    for (int64_t k = threadIdx.x; k < len; k += kThreads) dst[k] = (double)x[k];
  } else {
    const double* x = static_cast<const double*>(src);
    for (int64_t k = threadIdx.x; k < len; k += kThreads) dst[k] = x[k];
  }
}

}  // namespace fa
