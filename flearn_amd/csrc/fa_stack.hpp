// fa_stack.hpp — the kernels that reduce a contiguous client stack: balanced sub-tiles (the 8-byte
// kinds), the row pipeline (reduce_kernel_rows), the narrow window, the row-major groups and the
// opt-in split-N order.  Included by fa_reduce.hip and, through fa_device.hpp, by the tuning tools.
#pragma once

#include "fa_numerics.hpp"

namespace fa {

// Sub-tile kinds for reduce_subtile.
enum Part : int {
  kFull = 0,   // all V quads of every thread complete and inside the window (the hot path)
  kMasked = 1  // only slots v < nv are this block's; nv is WAVE-uniform (scalar branches)
};

// One sub-tile of the client stack for this thread: quads q0 + v*kThreads (v < V) of every row,
// all N rows in list order, then the fused epilogue.
// kMasked: slots v >= nv are outside this block's range.  Their loads are NOT skipped (an `if`
// around a load becomes exec-masked control flow and the compiler drains vmcnt at every join,
// serialising the row's loads); they re-read slot nv-1's address instead — an L1/L2 hit inside
// the same wave, no extra HBM traffic — and only the final stores are predicated.
template <class P, typename T, int OP, int V, int U, bool NT, int PART>
__device__ __forceinline__ void reduce_subtile(const typename P::x_t* __restrict__ base,
                                               int64_t stride, int n,
                                               const typename P::w_t* __restrict__ w, int64_t q0,
                                               int nv, const Epi<T>& e) {
  typedef typename P::x_t X;
  typedef typename P::acc_t A;
  typedef typename vec4<X>::type XV;
  typedef typename vec4<A>::type AV;
  // this lane's quad in slot 0, and each slot's offset from it (wave-uniform: nv is uniform)
  const X* lane = base + q0 * 4;
  int off[V];
#pragma unroll
  for (int v = 0; v < V; ++v) off[v] = ((PART == kFull || v < nv) ? v : nv - 1) * kThreads * 4;
  AV acc[V];
  {
    const typename P::w_t w0 = w[0];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const XV x = load_quad<X, NT>(lane + off[v]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[v][j] = P::mul(w0, x[j]);
    }
  }
  int i = 1;
  for (; i + U <= n; i += U) {
    XV x[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const X* row = lane + (int64_t)(i + u) * stride;
#pragma unroll
      for (int v = 0; v < V; ++v) x[u][v] = load_quad<X, NT>(row + off[v]);
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
    const X* row = lane + (int64_t)i * stride;
    const typename P::w_t wi = w[i];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const XV x = load_quad<X, NT>(row + off[v]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[v][j] = add<A>(acc[v][j], P::mul(wi, x[j]));
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v)
    if (PART == kFull || v < nv) finish_quad<T, OP, A>(e, (q0 + (int64_t)v * kThreads) * 4, 4, acc[v]);
}

// The window's ragged end (at most one wave per launch): one quad at a time, element-guarded.
template <class P, typename T, int OP>
__device__ __attribute__((noinline)) void reduce_ragged(const typename P::x_t* __restrict__ base,
                                                        int64_t stride, int n,
                                                        const typename P::w_t* __restrict__ w,
                                                        int64_t q0, int64_t qlim, int64_t ncols,
                                                        const Epi<T>& e) {
  typedef typename P::x_t X;
  typedef typename vec4<typename P::acc_t>::type AV;
#pragma unroll 1
  for (int64_t q = q0; q < qlim; q += kThreads) {
    const int64_t c = q * 4;
    const int valid = (int)((ncols - c) < 4 ? (ncols - c) : 4);
    AV acc;
    {
      const typename vec4<X>::type x = load_quad_guarded(base + c, valid);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = P::mul(w[0], x[j]);
    }
#pragma unroll 1
    for (int i = 1; i < n; ++i) {
      const typename vec4<X>::type x = load_quad_guarded(base + (int64_t)i * stride + c, valid);
      const typename P::w_t wi = w[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = add<typename P::acc_t>(acc[j], P::mul(wi, x[j]));
    }
    finish_quad<T, OP, typename P::acc_t>(e, c, valid, acc);
  }
}

// Sub-tile starting at quad qt, limited to quads < qlim (the block's range, <= the window).
template <class P, typename T, int OP, int V, int U, bool NT>
__device__ __forceinline__ void reduce_range_subtile(const typename P::x_t* __restrict__ base,
                                                     int64_t stride, int n,
                                                     const typename P::w_t* __restrict__ w,
                                                     int64_t qt, int64_t qlim, int64_t ncols,
                                                     const Epi<T>& e) {
  constexpr int kSub = kThreads * V;
  const int64_t q0 = qt + threadIdx.x;
  const int64_t qfull = ncols / 4;  // complete quads in the window
  if (qt + kSub <= qlim && qt + kSub <= qfull) {
    reduce_subtile<P, T, OP, V, U, NT, kFull>(base, stride, n, w, q0, V, e);
    return;
  }
  // slot v of wave wv covers quads [qt + v*kThreads + 64*wv, +64): count the complete ones
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x) / 64;
  const int64_t wbase = qt + 64 * wv;
  const int64_t lim = qlim < qfull ? qlim : qfull;
  int nv = 0;
  while (nv < V && wbase + (int64_t)nv * kThreads + 64 <= lim) ++nv;
  if (nv > 0) reduce_subtile<P, T, OP, V, U, NT, kMasked>(base, stride, n, w, q0, nv, e);
  // the rest of this wave's slots (only at the window's ragged end: lim < qlim)
  const int64_t qr = q0 + (int64_t)nv * kThreads;
  if (qr < qlim) reduce_ragged<P, T, OP>(base, stride, n, w, qr, qlim, ncols, e);
}

// Balanced grid.  Work unit: a CHUNK of 64 quads (1 KiB of one fp32 row = one wave-wide dwordx4
// instruction).  The host sizes the grid as k full waves of resident blocks (k = rounds) so that
// every block owns an equal share +-1 chunk of the window, preferably <= one sub-tile: all
// blocks of a round finish together (no tail of late blocks) and, because neighbouring blocks own
// neighbouring column ranges and sweep the rows in lockstep, the chip streams each client row
// almost sequentially — the access pattern of a plain linear read.
template <class P, typename T, int OP, int V, int U, bool NT>
__global__ __launch_bounds__(kThreads) void reduce_kernel_balanced(
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
    reduce_range_subtile<P, T, OP, V, U, NT>(base, stride, n, w, qt, qlim, ncols, e);
}

// Row-pipelined grid.  Built for deep, narrow windows (many clients, few columns: the per-rank
// column shards of a multi-GPU aggregation, e.g. 800 clients x 365 K columns), where the
// sub-tile kernels run out of column parallelism and a batch of rows that is issued, drained
// and re-issued keeps only half its bytes in flight on average.  Here:
//   * a block is W waves; lane l owns quads l, l+64W, ..., l+(V-1)*64W of the block's piece of
//     every row (V*W KiB contiguous per row), so each wave instruction reads 1 KiB of one row;
//   * rows are a rolling register pipeline D rows deep (rows_sweep): row i+D is loaded right
//     after row i is consumed, so D*V loads stay in flight per lane for the whole sweep
//     (s_waitcnt vmcnt((D-1)*V) in the steady state, no drain per batch);
//   * loads go through per-row buffer descriptors whose range check covers the window's end, so
//     a partial last piece needs no per-lane branches (the slot offset rides in voffset, which
//     the range check always covers) and the window's ragged last quad (ncols % 4) is read in
//     the same instructions (the range check is per dword).
// The summation order (client list order, first product initialises the sum) is unchanged.
template <class P, typename T, int OP, int V, int D, int W, bool NT>
__device__ __forceinline__ void rows_piece(const float* __restrict__ stack, int64_t stride, int n,
                                           const typename P::w_t* __restrict__ w, int64_t col0,
                                           int64_t ncols, const Epi<T>& e, int64_t qb,
                                           int64_t qend) {
  // the piece is quads [qb, qend), qend - qb <= 64*W*V; its columns, the window's ragged last
  // quad (ncols % 4 != 0) included: the raw-buffer range check is per dword on gfx950
  // (tools/probe_oob.py), so the missing elements of that quad load as 0 and are never stored
  typedef typename P::acc_t A;
  typedef typename vec4<A>::type AV;
  const int64_t cend = qend * 4 < ncols ? qend * 4 : ncols;
  const int cols = cend > qb * 4 ? (int)(cend - qb * 4) : 0;
  if (cols > 0) {
    AV acc[V];
    rows_sweep<P, V, D, W, NT>(StackRows{reinterpret_cast<const char*>(stack + col0 + qb * 4), stride * 4},
                               (uint32_t)cols * 4u, n, w, acc);
    finish_piece<T, OP, A, V, 64 * W, (V >= 2 ? 2 : V)>(e, qb, cols, acc);
  }
}

// Split-N reduce (fa_reduce_f32_splitn) for windows too narrow to fill the chip with one
// sequential sweep per column (LeNet5-sized models of many clients: 44 K columns x 1000 rows is
// 174 one-KiB row chunks for 256 CUs, each walking 1000 rows).  Here the CLIENTS are split too:
//   * a block owns one 1-KiB chunk of the window (64 quads) and W client splits: wave v sums the
//     contiguous rows [v*n/W, (v+1)*n/W) in list order (the split's first product initialises its
//     sum) through the row pipeline (rows_sweep, D rows in flight; the split index is made
//     wave-uniform with readfirstlane so every row keeps ONE scalar buffer descriptor);
//   * the W partial sums of a quad are staged in LDS and combined by a FIXED binary tree in
//     split order, ((p0+p1)+(p2+p3))+..., one barrier per level;
//   * then the epilogue of the row pipeline (divide, optional optimizer update, stores).
// Deterministic (the tree does not depend on scheduling) but NOT the reference's sequential
// order: opt-in, checked at <= 1e-6 normwise relative error per tensor (tests/test_gpu_splitn.py)
// — except columns whose terms nearly cancel (sum of |products| > 2 |sum|, or a non-finite
// sum): those are re-summed in list order by wave 0 (the cancellation guard below), bit-exact.
// oracle.c_reduce_splitn restates this exact order and guard (the tests pin it bit for bit).
// Needs n >= W (every split non-empty; the host falls back to the sequential kernel otherwise).
template <class P, typename T, int OP, int W, int D, bool NT>
__global__ __launch_bounds__(64 * W) void reduce_kernel_splitn(const float* __restrict__ stack, int64_t stride, int n,
                                                               const typename P::w_t* __restrict__ w, int64_t col0,
                                                               int64_t ncols, Epi<T> e) {
  typedef typename P::acc_t A;
  typedef typename vec4<A>::type AV;
  __shared__ AV part[W][64];
  __shared__ AV apart[W][64];  // the splits' sums of |product|: the cancellation guard
  const int lane = (int)threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);  // the split: wave-uniform
  // the chunk's columns, its last quad possibly partial: the raw buffer range check is per dword
  // on gfx950 (tools/probe_oob.py, profiles/r02/oob.json), so `bytes` = exactly the chunk's
  // columns and the missing elements of a ragged last quad load as 0 and are never stored
  const int64_t qb = (int64_t)blockIdx.x * 64;  // first quad of the chunk
  const int64_t cleft = ncols - qb * 4;
  const int tcols = cleft <= 0 ? 0 : (cleft < 256 ? (int)cleft : 256);
  const int nq = (tcols + 3) / 4;  // quads, the last possibly partial
  // split wv: contiguous rows [r0, r1)
  const int r0 = (int)((int64_t)wv * n / W);
  const int r1 = (int)((int64_t)(wv + 1) * n / W);
  typedef typename vec4<float>::type XV;
  const char* tile00 = reinterpret_cast<const char*>(stack + col0 + qb * 4);
  const uint32_t bytes = (uint32_t)tcols * 4u;
  const int voff = lane * 16;
  AV acc = {A(0), A(0), A(0), A(0)}, aacc = {A(0), A(0), A(0), A(0)};
  auto absq = [](AV v) { return AV{v[0] < A(0) ? -v[0] : v[0], v[1] < A(0) ? -v[1] : v[1],
                                   v[2] < A(0) ? -v[2] : v[2], v[3] < A(0) ? -v[3] : v[3]}; };
  if (nq > 0) {
    // this split's rows through a D-deep rolling pipeline with NO guarded loads: a slot past the
    // split's end re-reads its last row (a cache hit) and the product is discarded by a select,
    // so the loads stay unconditional and the ramp is not serialised by waitcnt merges.  Each
    // product p = fl(w*x) feeds the running sum (acc + p: the same rounding as acc + w*x, no
    // contraction) and the running sum of |p|
    const char* tile0 = tile00 + (int64_t)r0 * stride * 4;
    const int64_t row_bytes = stride * 4;
    const int cnt = r1 - r0;  // >= 1
    const typename P::w_t* ws = w + r0;
    XV x[D];
#pragma unroll
    for (int d = 0; d < D; ++d)
      x[d] = buf_load_quad<NT>(row_rsrc(tile0 + (int64_t)(d < cnt ? d : cnt - 1) * row_bytes, bytes), voff, 0);
    acc = quad_mul<P>(ws[0], x[0]);
    aacc = absq(acc);
    {
      const int r = D < cnt ? D : cnt - 1;
      x[0] = buf_load_quad<NT>(row_rsrc(tile0 + (int64_t)r * row_bytes, bytes), voff, 0);
    }
#pragma unroll
    for (int d = 1; d < D; ++d) {  // rows 1..D-1
      const AV p = quad_mul<P>(ws[d < cnt ? d : 0], x[d]);
      acc = d < cnt ? acc + p : acc;
      aacc = d < cnt ? aacc + absq(p) : aacc;
      __builtin_amdgcn_sched_barrier(0);
      const int r = d + D < cnt ? d + D : cnt - 1;
      x[d] = buf_load_quad<NT>(row_rsrc(tile0 + (int64_t)r * row_bytes, bytes), voff, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    for (int base = D; base < cnt; base += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int i = base + d;
        const AV p = quad_mul<P>(ws[i < cnt ? i : 0], x[d]);
        acc = i < cnt ? acc + p : acc;
        aacc = i < cnt ? aacc + absq(p) : aacc;
        __builtin_amdgcn_sched_barrier(0);
        const int r = i + D < cnt ? i + D : cnt - 1;
        x[d] = buf_load_quad<NT>(row_rsrc(tile0 + (int64_t)r * row_bytes, bytes), voff, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  part[wv][lane] = acc;
  apart[wv][lane] = aacc;
  __syncthreads();
#pragma unroll
  for (int h = 1; h < W; h *= 2) {  // fixed tree over the splits, one level per barrier
    if ((wv % (2 * h)) == 0 && wv + h < W) {
      part[wv][lane] = part[wv][lane] + part[wv + h][lane];
      apart[wv][lane] = apart[wv][lane] + apart[wv + h][lane];
    }
    __syncthreads();
  }
  if (wv == 0) {
    // cancellation guard: a column whose sum is not at least half its sum of |products|
    // (!(S_abs <= 2|S|): also NaN / inf) takes the reference's sequential sum instead — a
    // reordered sum of nearly cancelling terms can lie arbitrarily far (relatively) from the
    // sequential one; every other column is within the reordering's rounding error of it
    AV r = part[0][lane];
    const AV aa = apart[0][lane];
    bool flag[4], any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const A ab = r[k] < A(0) ? -r[k] : r[k];
      flag[k] = !(aa[k] <= A(2) * ab) || !(ab <= A(3.0e38));
      any |= flag[k];
    }
    if (__builtin_amdgcn_ballot_w64(any && lane < nq) != 0) {  // (wave-uniform)
      AV seq[1];
      rows_sweep<P, 1, 16, 1, NT>(StackRows{tile00, stride * 4}, bytes, n, w, seq);
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = flag[k] ? seq[0][k] : r[k];
    }
    const AV rr[1] = {r};
    finish_piece<T, OP, A, 1, 64, 1>(e, qb, tcols, rr);
  }
}

// Work split: the window's 1-KiB chunks are cut into equal pieces of pc <= W*V chunks, as many
// as make k whole rounds of the grid (pc = ceil(chunks / (k * grid))), so every block sweeps k
// pieces (the last one or two blocks one fewer) and the launch has no tail round.
// Block b takes pieces b, b+grid, b+2*grid, ...: at any moment the grid's pieces form one
// contiguous stretch of each row (a linear-read access pattern).  Dead ends (profiles/HISTORY.md):
// k consecutive pieces per block instead (tune_reduce set "il"); consecutive piece slots for the
// blocks that share an XCD (set "misc").
template <class P, typename T, int OP, int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void reduce_kernel_rows(const float* __restrict__ stack,
                                                             int64_t stride, int n,
                                                             const typename P::w_t* __restrict__ w,
                                                             int64_t col0, int64_t ncols, Epi<T> e) {
  static_assert(sizeof(typename P::x_t) == 4, "row pipeline is for 4-byte elements");
  const int64_t nquads = (ncols + 3) / 4;
  const int64_t chunks = (nquads + 63) / 64;
  const int64_t g = gridDim.x;
  const int64_t k = (chunks + g * W * V - 1) / (g * W * V);  // rounds
  const int64_t pc = (chunks + g * k - 1) / (g * k);         // chunks per piece (<= W*V)
  const int64_t pieces = (chunks + pc - 1) / pc;
  for (int64_t p = blockIdx.x; p < pieces; p += g) {
    const int64_t qs = p * pc * 64;
    rows_piece<P, T, OP, V, D, W, NT>(stack, stride, n, w, col0, ncols, e, qs,
                                      qs + pc * 64 < nquads ? qs + pc * 64 : nquads);
  }
}

// Narrow windows, deep pipeline (at most two 1-KiB row chunks per block: LeNet-sized models, deep
// client stacks).  Block b owns chunks [b*W, b*W + W), one per wave, lane l one quad.  Only D rows
// per wave bound the bytes in flight here (a wave's vmcnt counts at most 63 loads), so D goes up
// to 60 and the pipeline has no drain code: the sweep runs whole D-row rounds; in the last two a
// refill past the last row re-loads row n-1 (an L2 hit) and a product past it is dropped by a
// select.  The row address
// advances by the stride through one running scalar pointer (opaque to the compiler: written as
// row(i + d) in the unrolled loop, every d * stride was kept in a scalar register pair and
// spilled).  Same sums, same order as reduce_kernel_rows.
template <class P, typename T, int OP, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void reduce_kernel_narrow(const float* __restrict__ stack, int64_t stride,
                                                               int n, const typename P::w_t* __restrict__ w,
                                                               int64_t col0, int64_t ncols, Epi<T> e) {
  static_assert(sizeof(typename P::x_t) == 4 && D <= 63, "4-byte rows; vmcnt counts 63 loads");
  typedef typename P::acc_t A;
  typedef typename vec4<A>::type AV;
  typedef typename vec4<float>::type XV;
  const int64_t nquads = (ncols + 3) / 4;
  const int64_t qb = (int64_t)blockIdx.x * 64 * W;
  const int64_t qe = qb + 64 * W < nquads ? qb + 64 * W : nquads;
  const int64_t cend = qe * 4 < ncols ? qe * 4 : ncols;
  if (cend <= qb * 4) return;
  const int cols = (int)(cend - qb * 4);
  const uint32_t bytes = (uint32_t)cols * 4u;
  const int voff = (int)threadIdx.x * 16;
  const int64_t rb = stride * 4;
  const char* base = reinterpret_cast<const char*>(stack + col0 + qb * 4);
  const char* lastp = base + (int64_t)(n - 1) * rb;
  const char* p = base + rb;  // the next row to load (row 1)
#define FA_NW_LOAD(dst, CLAMP)                                                         \
  {                                                                                      \
    const char* q_ = p;                                                                  \
    if (CLAMP) q_ = p <= lastp ? p : lastp;                                              \
    dst = buf_load_quad<NT>(row_rsrc(q_, bytes), voff, 0);                               \
    p += rb;                                                                             \
    asm volatile("" : "+s"(p));                                                          \
  }
  // the weights of a round ride in one VGPR (lane l: row i + l), loaded a round ahead through a
  // range-checked descriptor and broadcast with readlane: a scalar load per row, waited for right
  // before its product, put a scalar-cache round trip on every row of the serial chain
  typedef typename P::w_t WT;
  const __amdgpu_buffer_rsrc_t wr = row_rsrc(w, (uint32_t)n * (uint32_t)sizeof(WT));
  const int lane = (int)threadIdx.x & 63;
  auto wload = [&](int first) {  // lane l of every wave: w[first + l] (0 past the end)
    if constexpr (sizeof(WT) == 4)
      return __builtin_bit_cast(WT, __builtin_amdgcn_raw_buffer_load_b32(wr, (lane + first) * 4, 0, 0));
    else
      return __builtin_bit_cast(WT, __builtin_amdgcn_raw_buffer_load_b64(wr, (lane + first) * 8, 0, 0));
  };
  auto wlane = [](WT v, int l) {
    if constexpr (sizeof(WT) == 4) {
      return __builtin_bit_cast(WT, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
    } else {
      const long long b = __builtin_bit_cast(long long, v);
      const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
      return __builtin_bit_cast(WT, (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
    }
  };
  WT wcur = wload(1);
  XV x[D];
#pragma unroll
  for (int d = 0; d < D; ++d) FA_NW_LOAD(x[d], true);
  AV acc = quad_mul<P>(w[0], buf_load_quad<NT>(row_rsrc(base, bytes), voff, 0));
  int i = 1;
  // steady rounds: every consumed row and every refill row is real
  for (; i + 2 * D <= n; i += D) {
    const WT wnext = wload(i + D);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      acc = quad_axpy<P>(acc, wlane(wcur, d), x[d]);
      __builtin_amdgcn_sched_barrier(0);
      FA_NW_LOAD(x[d], false);
      __builtin_amdgcn_sched_barrier(0);
    }
    wcur = wnext;
  }
  // the last (at most two) rounds: refills clamped to row n-1, products past it dropped
  for (; i < n; i += D) {
    const WT wnext = wload(i + D);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const AV t = quad_axpy<P>(acc, wlane(wcur, d), x[d]);
      acc = i + d < n ? t : acc;
      __builtin_amdgcn_sched_barrier(0);
      FA_NW_LOAD(x[d], true);
      __builtin_amdgcn_sched_barrier(0);
    }
    wcur = wnext;
  }
#undef FA_NW_LOAD
  const AV accs[1] = {acc};
  finish_piece<T, OP, A, 1, 64 * W, 1>(e, qb, cols, accs);
}

// piece j of the group starting at slot g0: quads [qb, qb + bytes/16) of every row (interleaved
// over the grid as in reduce_kernel_rows); the window's ragged last quad included (per-dword range
// check: its missing elements load as 0 and are never stored); bytes 0: every access dropped
__device__ __forceinline__ void rowmajor_piece_geom(int64_t g0, int j, int64_t k, int64_t pc, int64_t pieces,
                                                    int64_t nquads, int64_t ncols, int64_t* qb, uint32_t* bytes) {
  const int64_t pj = blockIdx.x + (g0 + j) * (int64_t)gridDim.x;
  int64_t q = pj * pc * 64;
  const int64_t qe = q + pc * 64 < nquads ? q + pc * 64 : nquads;
  const int64_t ce = qe * 4 < ncols ? qe * 4 : ncols;
  const int64_t left = ce - q * 4;
  const uint32_t b = (pj < pieces && g0 + j < k && left > 0) ? (uint32_t)left * 4u : 0u;
  *qb = b ? q : 0;
  *bytes = b;
}

// One group of a row-major block: KG of the block's pieces (slots g0 .. g0+KG-1, interleaved
// over the grid as in reduce_kernel_rows), all rows swept once, then the group epilogue.
// XL: whole-line f64 state / result stores (buf_store_tquad).
// Dead ends, measured and removed (profiles/HISTORY.md §4): the next group's first loads issued
// before this group's epilogue stores (finding 24); the last pieces' sums parked in LDS so that XL
// fits KG = 4 (finding 23); a per-quad epilogue through finish_quad (finding 10).
// EARLY / RQ: the group's tail (below); chosen per launch by the kernel.
template <class P, typename T, int OP, int V, int D, int W, int KG, bool NT, int EPIB, bool TR, bool XL,
          bool EARLY = false, int RQ = 0>
__device__ __forceinline__ void rowmajor_group(const char* __restrict__ base, int64_t row_bytes, int n,
                                               const typename P::w_t* __restrict__ w, int64_t g0, int64_t k,
                                               int64_t pc, int64_t pieces, int64_t nquads, int64_t ncols,
                                               int gi, const Epi<T>& e,
                                               typename vec4<float>::type (&x)[D][V]) {
  static_assert(KG % D == 0, "pipeline depth must divide the group size");
  typedef typename P::acc_t A;
  typedef typename vec4<A>::type AV;
  int voff = (int)threadIdx.x * 16;
  // the early tail's copy of the sweep derives its lane offsets per group: shared with the other
  // copy across the kernel, one of them was spilled to scratch and reloaded inside the last row
  if constexpr (EARLY) asm volatile("" : "+v"(voff));
  int64_t qb[KG];
  uint32_t bytes[KG];  // 4 x the piece's columns; 0: every access of this slot is dropped
#pragma unroll
  for (int j = 0; j < KG; ++j) rowmajor_piece_geom(g0, j, k, pc, pieces, nquads, ncols, &qb[j], &bytes[j]);
  AV acc[KG][V];
  // step s = (i, j), i = s / KG, j = s % KG; slot = j % D
#define FA_RM_LOAD(slot, row, j)                                                                      \
  {                                                                                                   \
    const __amdgpu_buffer_rsrc_t r_ = row_rsrc(base + qb[j] * 16 + (int64_t)(row) * row_bytes, bytes[j]); \
    _Pragma("unroll") for (int v = 0; v < V; ++v) x[slot][v] = buf_load_quad<NT>(r_, voff + v * 64 * W * 16, 0); \
  }
#pragma unroll
  for (int d = 0; d < D; ++d) FA_RM_LOAD(d, 0, d);
  // row 0: products initialise the sums
#pragma unroll
  for (int j = 0; j < KG; ++j) {
    const typename P::w_t w0 = w[0];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[j][v] = quad_mul<P>(w0, x[j % D][v]);
    __builtin_amdgcn_sched_barrier(0);
    if (j + D < KG) {
      FA_RM_LOAD(j % D, 0, j + D);
    } else if (n > 1) {
      FA_RM_LOAD(j % D, 1, j + D - KG);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  int i = 1;
  for (; i + 1 < n; ++i) {  // rows with a successor: every refill is a real step
    const typename P::w_t wi = w[i];
#pragma unroll
    for (int j = 0; j < KG; ++j) {
#pragma unroll
      for (int v = 0; v < V; ++v) acc[j][v] = quad_axpy<P>(acc[j][v], wi, x[j % D][v]);
      __builtin_amdgcn_sched_barrier(0);
      if (j + D < KG) {
        FA_RM_LOAD(j % D, i, j + D);
      } else {
        FA_RM_LOAD(j % D, i + 1, j + D - KG);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // The group's tail: the last row and the epilogue.  EARLY (the plain fp32 mean into out32 alone,
  // at least two rows; RQ: quot's form): in the last row a piece's sums are final once its step is
  // consumed, and the next piece's loads are issued right after — so pieces 0 .. KG-2 are divided
  // under those loads, in place (the fp32 results replace the sums: no registers added), and only
  // the last piece's divide runs with nothing in flight.  Two quads at a time between scheduling
  // barriers, as the sweep pins its steps.  The same arithmetic per element as finish_piece's; the
  // stores stay at the group's end (findings 14 and 24: stores inside the read stream lose).
  // The tail is a template argument and not a branch here: with two tails behind one sweep the
  // register allocator spilled the sweep's lane offsets to scratch (DESIGN.md §4 finding 28).
  static_assert(!EARLY || (OP == FA_OP_MEAN && sizeof(A) == 4), "early quotients: the plain fp32 mean");
  constexpr int kQB = V >= 2 ? 2 : 1;  // quads divided between two scheduling barriers
  if (i < n) {  // last row: refills only inside the row
    const typename P::w_t wi = w[i];
#pragma unroll
    for (int j = 0; j < KG; ++j) {
#pragma unroll
      for (int v = 0; v < V; ++v) acc[j][v] = quad_axpy<P>(acc[j][v], wi, x[j % D][v]);
      if (j + D < KG) FA_RM_LOAD(j % D, i, j + D);
      if constexpr (EARLY) {
        if (j + 1 < KG) {
#pragma unroll
          for (int v0 = 0; v0 < V; v0 += kQB) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int v = v0; v < v0 + kQB; ++v)
#pragma unroll
              for (int c = 0; c < 4; ++c) acc[j][v][c] = (A)quot<T, A, RQ>(e, acc[j][v][c]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
#undef FA_RM_LOAD
  if constexpr (TR) {
    if (threadIdx.x == 0 && gi < 7) e.trace[blockIdx.x * 16 + 1 + 2 * gi] = wall_clock64();
  }
  if constexpr (EARLY) {  // (the kernel sends n == 1 to the other tail)
#pragma unroll
    for (int j = 0; j + 1 < KG; ++j) {  // these hold their fp32 results
      const __amdgpu_buffer_rsrc_t r32 = col_rsrc<float>(e.out32, qb[j], (int)(bytes[j] / 4));
#pragma unroll
      for (int v = 0; v < V; ++v) buf_store_tquad<float>(r32, (int)threadIdx.x + v * 64 * W, acc[j][v]);
    }
    if (bytes[KG - 1] > 0) {
      const EpiRsrc<T, OP> r(e, qb[KG - 1], (int)(bytes[KG - 1] / 4));
      finish_piece_rq<T, OP, A, V, 64 * W, EPIB, XL, RQ>(e, r, acc[KG - 1]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < KG; ++j) finish_piece<T, OP, A, V, 64 * W, EPIB, XL>(e, qb[j], (int)(bytes[j] / 4), acc[j]);
  }
  if constexpr (TR) {
    if (threadIdx.x == 0 && gi < 7) e.trace[blockIdx.x * 16 + 2 + 2 * gi] = wall_clock64();
  }
}

// A block's groups, under the tail the launch takes (wave-uniform; rowmajor_group): early quotients
// for the plain fp32 mean of two or more rows into out32 alone, where the host chose the reciprocal
// form (e.rq).  Measured on 100 x 25.6 M (tools/tune_reduce.hip set "quot", DESIGN.md §4 finding
// 28): early reciprocal quotients -5..-6 us a launch; early IEEE divides +2.6 us (13 f64
// instructions an element outlast the loads they sit under), so those launches keep the tail at the
// group's end.  KG = 4 stands at 488 of the 512 registers with one sweep and a second copy of it
// spilled: it keeps one tail too.
// ED = false (tools/tune_reduce.hip only): every quotient at the group's end, as before finding 28.
template <class P, typename T, int OP, int V, int D, int W, int KG, bool NT, int EPIB, bool TR, bool XL, bool ED>
__device__ __forceinline__ void rowmajor_groups(const char* __restrict__ base, int64_t row_bytes, int n,
                                                const typename P::w_t* __restrict__ w, int64_t k, int64_t pc,
                                                int64_t pieces, int64_t nquads, int64_t ncols, const Epi<T>& e,
                                                typename vec4<float>::type (&x)[D][V]) {
  typedef typename P::acc_t A;
  int gi = 0;
#define FA_RM_GROUPS(EARLY, RQ)                                                                               \
  for (int64_t g0 = 0; g0 < k; g0 += KG)                                                                      \
    rowmajor_group<P, T, OP, V, D, W, KG, NT, EPIB, TR, XL, EARLY, RQ>(base, row_bytes, n, w, g0, k, pc, pieces, \
                                                                       nquads, ncols, gi++, e, x);
  if constexpr (ED && OP == FA_OP_MEAN && kHasRecipQuot<T, A> && KG <= 3) {
    if (n >= 2 && e.out64 == nullptr && e.rq == 1) {
      FA_RM_GROUPS(true, 1)
      return;
    }
#ifdef FA_TUNE_QUOT_MUL
    if (n >= 2 && e.out64 == nullptr && e.rq == 2) {
      FA_RM_GROUPS(true, 2)
      return;
    }
#endif
  }
  FA_RM_GROUPS(false, 0)
#undef FA_RM_GROUPS
}

// Row-major variant for blocks that own several pieces (k > 1: C2-C5-sized buckets).  The
// column-major walk (reduce_kernel_rows: piece after piece, all rows each) starts every round of
// pieces with the blocks out of step, and rounds after the first measured ~8% slower per row on
// 100-client buckets (tune/trace_*).  Here a block sweeps the rows ONCE for a group of up to KG
// pieces: step s = (row i, piece j) with j fastest, KG accumulators per lane, and the same
// rolling register pipeline D steps deep (D divides KG, so every slot index is static).  The
// whole grid then moves through the client rows together.  Per element the sum is still rows
// 0..N-1 in order.
// TR (tools/tune_reduce.hip set "timeline"): wave 0 of every block stamps the 100-MHz wall clock
// at its start and at each group's sweep end and epilogue end into e.trace[block * 16 + slot].
// EPIB: slots per lane whose state the piece epilogue loads at once (finish_piece's B).
// XL: whole-line f64 state / result stores; by default where they cost no spills: the fused ops at
// KG <= 3 (at KG = 4 the LDS regrouping pushes the kernel past 256 + 256 registers; finding 22).
template <class P, typename T, int OP, int V, int D, int W, int KG, bool NT, int EPIB = (V >= 2 ? 2 : V),
          bool TR = false, bool XL = (sizeof(T) == 8 && OP != FA_OP_MEAN && KG <= 3)>
__global__ __launch_bounds__(64 * W) void reduce_kernel_rowmajor(const float* __restrict__ stack,
                                                                 int64_t stride, int n,
                                                                 const typename P::w_t* __restrict__ w,
                                                                 int64_t col0, int64_t ncols, Epi<T> e) {
  static_assert(sizeof(typename P::x_t) == 4, "row pipeline is for 4-byte elements");
  const int64_t nquads = (ncols + 3) / 4;
  const int64_t chunks = (nquads + 63) / 64;
  const int64_t g = gridDim.x;
  const int64_t k = (chunks + g * W * V - 1) / (g * W * V);  // pieces per block
  const int64_t pc = (chunks + g * k - 1) / (g * k);         // chunks per piece (<= W*V)
  const int64_t pieces = (chunks + pc - 1) / pc;
  const int64_t row_bytes = stride * 4;
  const char* base = reinterpret_cast<const char*>(stack + col0);
  if constexpr (TR) {
    if (threadIdx.x == 0) e.trace[blockIdx.x * 16] = wall_clock64();
  }
  static_assert(EPIB >= 1, "the piece epilogue batches at least one slot");
  typename vec4<float>::type x[D][V];  // the pipeline's slots
  rowmajor_groups<P, T, OP, V, D, W, KG, NT, EPIB, TR, XL, true>(base, row_bytes, n, w, k, pc, pieces, nquads, ncols, e, x);
}

}  // namespace fa
