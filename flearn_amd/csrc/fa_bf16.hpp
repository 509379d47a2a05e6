// fa_bf16.hpp — bfloat16 uploads (fa_fold_bf16): the weighted fp32 sum of one
// chunk of clients whose rows are bfloat16 bit patterns, widened in registers.  fold_kernel_rows' and
// fa::quant::deq_fold_kernel's sibling with the family's work split (equal interleaved pieces of
// <= W*V chunks derived from the grid, per-row range-checked descriptors so that ragged ends load 0,
// one 16-B non-temporal load per lane and row, a D-deep load pipeline, the piece's sums in registers,
// one range-checked store per piece).  What differs: a 16-B load is 8 columns, so a wave's chunk is
// 512 columns and a lane keeps 8 fp32 sums (two quads) per chunk; there is no scale stream and no
// centre; and widening is exact — a bfloat16 is the high half of the fp32 of the same value, so a
// dword becomes its two columns with one shift (the even column, in the low half) and one mask (the
// odd one).  Included by fa_bf16.hip only.  The kernel lives in fa::bf16: the inventories pin the
// kernels of fa, fa::clip, fa::clipfold and fa::noise.
#pragma once

#include "fa_numerics.hpp"

namespace fa {
namespace bf16 {

typedef vec4<float>::type XV;

constexpr int kChunk = 512;  // columns of one wave-chunk: 64 lanes x 16 B / 2

// The 8 columns of one 16-B load as two fp32 quads in column order: bits << 16, exactly.
__device__ __forceinline__ void widen(u32x4 x, XV& a, XV& b) {
  const u32x4 lo = x << 16, hi = x & 0xFFFF0000u;
  a = __builtin_bit_cast(XV, u32x4{lo[0], hi[0], lo[1], hi[1]});
  b = __builtin_bit_cast(XV, u32x4{lo[2], hi[2], lo[3], hi[3]});
}

// quant::rows_each's pipeline with one stream: rows 0..n-1 of the piece in order, slot d holding row
// i + d's loads x[d][v] (chunk v * W + wave of the piece); use(i, x) consumes row i.  One running
// scalar row pointer; chunks past the piece's end read 0.
template <int V, int D, int W, bool NT, class Use>
__device__ __forceinline__ void rows_each(const char* tile0, int64_t row_bytes, uint32_t bytes, int n, Use&& use) {
  const int voff = (int)threadIdx.x * 16;
  const char* pn = tile0;  // the next row to load
#define FA_BF16_LOAD(slot)                                                                           \
  {                                                                                                  \
    const __amdgpu_buffer_rsrc_t r_ = row_rsrc(pn, bytes);                                           \
    _Pragma("unroll") for (int v = 0; v < V; ++v)                                                    \
      x[slot][v] = __builtin_amdgcn_raw_buffer_load_b128(r_, voff + v * 64 * W * 16, 0, NT ? 2 : 0); \
    pn += row_bytes;                                                                                 \
    asm volatile("" : "+s"(pn));                                                                     \
  }
  u32x4 x[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < n) FA_BF16_LOAD(d)
  int i = 0;
  for (; i + 2 * D <= n; i += D) {  // steady state: every refill (row i + d + D) is a real row
#pragma unroll
    for (int d = 0; d < D; ++d) {
      use(i + d, x[d]);
      __builtin_amdgcn_sched_barrier(0);  // consume slot d, then refill it
      FA_BF16_LOAD(d)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {  // drain: fewer than 2*D rows left
    if (i + d < n) {
      use(i + d, x[d]);
      if (i + d + D < n) FA_BF16_LOAD(d)
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (i + D + d < n) use(i + D + d, x[d]);
#undef FA_BF16_LOAD
}

// fa_fold_bf16.  Per column and row, every operation rounded to fp32 and none contracted:
//   x = float(bits << 16);  acc = acc + weight * x
// acc_in == NULL (wave-uniform) opens the round: the sums start at -0.0, the identity of the fp32
// add (-0.0 + t == t for every t, -0.0 and subnormals included), so row 0's product is the first sum
// bit for bit and every row runs the same code.  Else the piece's carried sums are loaded through a
// range-checked descriptor.  acc_out may be acc_in: a lane reads its quads before it writes them
// and no other lane touches them.  A lane's 8 columns of chunk c are fp32 quads c * 128 + lane * 2
// + 0..1.  The rows' descriptor range is the piece's bytes rounded up to a dword (inside the row:
// strides and window starts are multiples of 8 columns); the store's range is the columns
// themselves, so what a ragged end computes from the half dword past it is dropped.
template <int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void widen_fold_kernel(const uint16_t* __restrict__ stack, int64_t stride, int n,
                                                            const float* __restrict__ weights, const float* acc_in,
                                                            float* acc_out, int64_t col0, int64_t ncols) {
  const int64_t chunks = (ncols + kChunk - 1) / kChunk;
  const int64_t gr = gridDim.x;
  const int64_t k = (chunks + gr * W * V - 1) / (gr * W * V);  // rounds
  const int64_t pc = (chunks + gr * k - 1) / (gr * k);         // chunks per piece (<= W*V)
  const int64_t pieces = (chunks + pc - 1) / pc;
  const bool first = acc_in == nullptr;
  const int q0 = (int)threadIdx.x * 2;  // the lane's first fp32 quad of slot 0: chunk `wave`, 8 columns per lane
  for (int64_t p = blockIdx.x; p < pieces; p += gr) {
    const int64_t cb = p * pc;
    const int64_t ce = cb + pc < chunks ? cb + pc : chunks;
    const int64_t colb = cb * kChunk;
    const int64_t cend = ce * kChunk < ncols ? ce * kChunk : ncols;
    const int cols = cend > colb ? (int)(cend - colb) : 0;
    if (cols <= 0) continue;
    XV acc[V][2];
    if (first) {
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[v][j] = XV{-0.f, -0.f, -0.f, -0.f};
    } else {
      const __amdgpu_buffer_rsrc_t ra = col_rsrc<const float>(acc_in, colb / 4, cols);
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[v][j] = buf_load_tquad<float>(ra, q0 + v * W * 128 + j);
    }
    const char* tile0 = reinterpret_cast<const char*>(stack + col0 + colb);
    const uint32_t bytes = ((uint32_t)cols * 2u + 3u) & ~3u;
    rows_each<V, D, W, NT>(tile0, stride * 2, bytes, n, [&](int i, const u32x4(&x)[V]) {
      const float a = weights[i];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        XV t[2];
        widen(x[v], t[0], t[1]);
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[v][j] = acc[v][j] + a * t[j];
      }
    });
    const __amdgpu_buffer_rsrc_t ro = col_rsrc<float>(acc_out, colb / 4, cols);
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int j = 0; j < 2; ++j) buf_store_tquad<float>(ro, q0 + v * W * 128 + j, acc[v][j]);
  }
}

}  // namespace bf16
}  // namespace fa
