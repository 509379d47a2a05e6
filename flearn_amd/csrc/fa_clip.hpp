// fa_clip.hpp — norm-clipped rounds (fa_rownorm2_f32 / fa_clip_sum_f32): the
// clients' squared update norms in one pass over the stack, and the sum of the clipped uploads in a
// second one.  Both are fold_kernel_rows' siblings: its work split (pieces of <= W*V 1-KiB chunks),
// its per-row range-checked descriptors (ragged ends load 0), 16 B per lane, non-temporal, and its
// D-deep load pipeline; the piece's centre quads are loaded once and stay in registers.  Included by
// fa_clip.hip only.  The kernels live in fa::clip: the kernel inventory pins the kernels of
// namespace fa itself.
#pragma once

#include "fa_numerics.hpp"

namespace fa {
namespace clip {

typedef vec4<float>::type XV;

// rows_fold_sweep's pipeline for a per-row callback: rows s..n-1 of the piece, in order, slot d
// holding row i + d; use(i, x) consumes row i's quads, want(i) (wave-uniform) says whether row i
// is read at all (a row that is not wanted leaves its slot undefined and `use` must not look at it);
// ramped() runs once after the ramp's loads are issued.  One running scalar row pointer, as there.
template <int V, int D, int W, bool NT, class Want, class Ramped, class Use>
__device__ __forceinline__ void rows_each(const char* tile0, int64_t row_bytes, uint32_t bytes, int s, int n,
                                          Want&& want, Ramped&& ramped, Use&& use) {
  const int voff = (int)threadIdx.x * 16;
  const char* pn = tile0 + (int64_t)s * row_bytes;  // the next row to load
#define FA_CLIP_LOAD(slot, row)                                                                   \
  {                                                                                               \
    if (want(row)) {                                                                              \
      const __amdgpu_buffer_rsrc_t r_ = row_rsrc(pn, bytes);                                      \
      _Pragma("unroll") for (int v = 0; v < V; ++v) x[slot][v] = buf_load_quad<NT>(r_, voff + v * 64 * W * 16, 0); \
    }                                                                                             \
    pn += row_bytes;                                                                              \
    asm volatile("" : "+s"(pn));                                                                  \
  }
  XV x[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (s + d < n) FA_CLIP_LOAD(d, s + d)
  ramped();
  int i = s;
  for (; i + 2 * D <= n; i += D) {  // steady state: every refill (row i + d + D) is a real row
#pragma unroll
    for (int d = 0; d < D; ++d) {
      use(i + d, x[d]);
      __builtin_amdgcn_sched_barrier(0);  // consume slot d, then refill it
      FA_CLIP_LOAD(d, i + d + D)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {  // drain: fewer than 2*D rows left
    if (i + d < n) {
      use(i + d, x[d]);
      if (i + d + D < n) FA_CLIP_LOAD(d, i + d + D)
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (i + D + d < n) use(i + D + d, x[d]);
#undef FA_CLIP_LOAD
}

// v + (v of the lane DPP control CTRL names), every lane of the wave
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false);
  return v + __builtin_bit_cast(float, o);
}

// The wave's sum of v in a fixed order, wave-uniform: pairs, quads, eights and sixteens inside each
// row of 16 lanes (every lane of a row then holds the row's sum), then the four rows in order —
// kRownormWaveAdds = 7 roundings behind the result.
__device__ __forceinline__ float wave_total(float v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
  v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
  v = dpp_add<0x141>(v);  // row_half_mirror: the other quad of the eight
  v = dpp_add<0x140>(v);  // row_mirror: the other eight of the row
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return ((r0 + r1) + r2) + r3;
}

// fa_rownorm2_f32, first kernel: partials[blockIdx.x * n + i] = the block's fp32 sum of
// fl32(x_i - g)^2 over its pieces (pc chunks each, pieces blockIdx.x, + gridDim.x, ...; the host
// launches no more blocks than pieces).  A lane squares its 4*V differences of a row with fused
// multiply-adds (one chain per element slot of its quads), the wave adds its lanes in wave_total's
// order, and lane r & 63 of running sum r >> 6 keeps the wave's sum for row r: two registers for up
// to 128 clients, updated under a lane mask, no atomics.  The W waves' sums are added in wave order
// at the block's end.  center == NULL: an empty descriptor range, g = 0 and fl32(x - 0) = x.
template <int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void rownorm_kernel(const float* __restrict__ stack, int64_t stride, int n,
                                                         const float* __restrict__ center, int64_t col0,
                                                         int64_t ncols, int64_t pc, float* __restrict__ partials) {
  __shared__ float part[W][128];
  const int64_t nquads = (ncols + 3) / 4;
  const int64_t chunks = (nquads + 63) / 64;
  const int64_t pieces = (chunks + pc - 1) / pc;
  const int lane = (int)threadIdx.x & 63;
  float rs0 = 0.f, rs1 = 0.f;
  for (int64_t p = blockIdx.x; p < pieces; p += gridDim.x) {
    const int64_t qb = p * pc * 64;
    const int64_t qe = qb + pc * 64 < nquads ? qb + pc * 64 : nquads;
    const int64_t cend = qe * 4 < ncols ? qe * 4 : ncols;
    const int cols = cend > qb * 4 ? (int)(cend - qb * 4) : 0;
    if (cols <= 0) continue;
    const __amdgpu_buffer_rsrc_t rg = col_rsrc<const float>(center ? center + col0 : nullptr, qb, cols);
    XV g[V];
#pragma unroll
    for (int v = 0; v < V; ++v) g[v] = buf_load_tquad<float>(rg, (int)threadIdx.x + v * 64 * W);
    rows_each<V, D, W, NT>(
        reinterpret_cast<const char*>(stack + col0 + qb * 4), stride * 4, (uint32_t)cols * 4u, 0, n,
        [](int) { return true; }, [] {},
        [&](int i, const XV(&x)[V]) {
          float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
#pragma unroll
          for (int v = 0; v < V; ++v) {
            const XV d = x[v] - g[v];
            q0 = __builtin_fmaf(d[0], d[0], q0);
            q1 = __builtin_fmaf(d[1], d[1], q1);
            q2 = __builtin_fmaf(d[2], d[2], q2);
            q3 = __builtin_fmaf(d[3], d[3], q3);
          }
          const float tot = wave_total((q0 + q1) + (q2 + q3));
          rs0 = lane == i ? rs0 + tot : rs0;
          rs1 = lane == i - 64 ? rs1 + tot : rs1;
        });
  }
  const int wave = (int)threadIdx.x >> 6;
  part[wave][lane] = rs0;
  part[wave][64 + lane] = rs1;
  __syncthreads();
  const int t = (int)threadIdx.x;
  if (t < n) {
    float s = part[0][t];
#pragma unroll
    for (int w = 1; w < W; ++w) s += part[w][t];
    partials[(int64_t)blockIdx.x * n + t] = s;
  }
}

// fa_rownorm2_f32, second kernel: client t's partials summed in float64 in block order
__global__ __launch_bounds__(128) void rownorm_finish_kernel(const float* __restrict__ partials, int grid, int n,
                                                             double* __restrict__ out) {
  const int t = (int)threadIdx.x;
  if (t >= n) return;
  double s = 0.0;
  for (int b = 0; b < grid; ++b) s += (double)partials[(int64_t)b * n + t];
  out[t] = s;
}

// One row under the three-way rule (s wave-uniform): s >= 1 the row itself, 0 < s < 1
// g + s * (x - g) with every operation rounded, else (s <= 0, NaN) the centre, x unread.
// clip_first turns row 0's quads, loaded into the sums' registers, into the first clipped upload;
// clip_add adds a later row.
template <int V>
__device__ __forceinline__ void clip_first(XV (&acc)[V], const XV (&g)[V], float s) {
  if (s >= 1.f) return;
  if (s > 0.f) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = g[v] + s * (acc[v] - g[v]);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = g[v];
  }
}

template <int V>
__device__ __forceinline__ void clip_add(XV (&acc)[V], const XV (&g)[V], float s, const XV (&x)[V]) {
  if (s >= 1.f) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = acc[v] + x[v];
  } else if (s > 0.f) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = acc[v] + (g[v] + s * (x[v] - g[v]));
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = acc[v] + g[v];
  }
}

// fa_clip_sum_f32: fold_kernel_rows' split (equal interleaved pieces of pc <= W*V chunks, derived
// from the grid as there), the first row's clipped upload initialising the sums (an all -0.0 column
// with unit scales stays -0.0), the others added in list order, the sums stored once per piece
// through a range-checked descriptor (lanes past the end are dropped).
template <int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void clip_sum_kernel(const float* __restrict__ stack, int64_t stride, int n,
                                                          const float* __restrict__ center,
                                                          const float* __restrict__ scale, float* acc_out,
                                                          int64_t col0, int64_t ncols) {
  const int64_t nquads = (ncols + 3) / 4;
  const int64_t chunks = (nquads + 63) / 64;
  const int64_t gr = gridDim.x;
  const int64_t k = (chunks + gr * W * V - 1) / (gr * W * V);  // rounds
  const int64_t pc = (chunks + gr * k - 1) / (gr * k);         // chunks per piece (<= W*V)
  const int64_t pieces = (chunks + pc - 1) / pc;
  for (int64_t p = blockIdx.x; p < pieces; p += gr) {
    const int64_t qb = p * pc * 64;
    const int64_t qe = qb + pc * 64 < nquads ? qb + pc * 64 : nquads;
    const int64_t cend = qe * 4 < ncols ? qe * 4 : ncols;
    const int cols = cend > qb * 4 ? (int)(cend - qb * 4) : 0;
    if (cols <= 0) continue;
    const __amdgpu_buffer_rsrc_t rg = col_rsrc<const float>(center + col0, qb, cols);
    XV g[V], acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) g[v] = buf_load_tquad<float>(rg, (int)threadIdx.x + v * 64 * W);
    const char* tile0 = reinterpret_cast<const char*>(stack + col0 + qb * 4);
    const uint32_t bytes = (uint32_t)cols * 4u;
    rows_each<V, D, W, NT>(
        tile0, stride * 4, bytes, 1, n, [&](int i) { return scale[i] > 0.f; },
        [&] {  // row 0, behind the ramp's loads as in rows_fold_sweep
          const float s0 = scale[0];
          if (s0 > 0.f) {
            const __amdgpu_buffer_rsrc_t r = row_rsrc(tile0, bytes);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = buf_load_quad<NT>(r, (int)threadIdx.x * 16 + v * 64 * W * 16, 0);
          }
          clip_first<V>(acc, g, s0);
        },
        [&](int i, const XV(&x)[V]) { clip_add<V>(acc, g, scale[i], x); });
    const __amdgpu_buffer_rsrc_t ro = col_rsrc<float>(acc_out, qb, cols);
#pragma unroll
    for (int v = 0; v < V; ++v) buf_store_tquad<float>(ro, (int)threadIdx.x + v * 64 * W, acc[v]);
  }
}

}  // namespace clip
}  // namespace fa
