// fa_quant.hpp — int8 block-quantized uploads (fa_deq_fold_q8): the weighted
// fp32 sum of one chunk of clients whose rows are 1-byte codes with one fp32 scale per 1024 columns,
// dequantized in registers.  fold_kernel_rows' / clip_fold_kernel's sibling: their work split
// (equal interleaved pieces of <= W*V chunks, derived from the grid), per-row range-checked
// descriptors (ragged ends load 0), one 16-B non-temporal load per lane and row, a D-deep load
// pipeline, the piece's centre kept in registers, the sums stored once per piece.  Here a 16-B load
// is 16 columns, so a wave's chunk is 1024 columns — one scale block: a row's scale is wave-uniform
// per chunk and travels through the pipeline beside the row's codes (a broadcast vector load, so it
// returns in order with them and is never waited for on its own).  Included by fa_quant.hip only.
// The kernel lives in fa::quant: the inventories pin the kernels of fa, fa::clip, fa::clipfold and
// fa::noise.
#pragma once

#include <type_traits>

#include "fa_numerics.hpp"

namespace fa {
namespace quant {

typedef vec4<float>::type XV;

// The 4 codes of one dword, sign-extended: exact in fp32.
__device__ __forceinline__ XV codes_of(uint32_t w) {
  return XV{(float)(int8_t)(w), (float)(int8_t)(w >> 8), (float)(int8_t)(w >> 16), (float)(int8_t)(w >> 24)};
}

// clip::rows_each's pipeline with a second stream: rows 0..n-1 of the piece in order, slot d holding
// row i + d's code quads x[d][v] and its scales sc[d][v] (chunk v * W + wave of the piece); use(i, x,
// sc) consumes row i.  Two running scalar row pointers.  The scale load's offset sits in the VGPR
// offset (wave * 4) and the instruction offset (v * W * 4): both are range-checked, chunks past the
// piece's end read 0.
template <int V, int D, int W, bool NT, class Use>
__device__ __forceinline__ void rows_each(const char* tile0, int64_t row_bytes, uint32_t bytes, const char* sc0,
                                          int64_t sc_row_bytes, uint32_t sc_bytes, int n, Use&& use) {
  const int voff = (int)threadIdx.x * 16;
  const int svoff = ((int)threadIdx.x >> 6) * 4;
  const char* pn = tile0;  // the next row to load
  const char* ps = sc0;
#define FA_Q8_LOAD(slot)                                                                           \
  {                                                                                                \
    const __amdgpu_buffer_rsrc_t r_ = row_rsrc(pn, bytes);                                         \
    const __amdgpu_buffer_rsrc_t q_ = row_rsrc(ps, sc_bytes);                                      \
    _Pragma("unroll") for (int v = 0; v < V; ++v) {                                                \
      x[slot][v] = __builtin_amdgcn_raw_buffer_load_b128(r_, voff + v * 64 * W * 16, 0, NT ? 2 : 0); \
      sc[slot][v] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(q_, svoff + v * W * 4, 0, 0)); \
    }                                                                                              \
    pn += row_bytes;                                                                               \
    ps += sc_row_bytes;                                                                            \
    asm volatile("" : "+s"(pn), "+s"(ps));                                                         \
  }
  u32x4 x[D][V];
  float sc[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < n) FA_Q8_LOAD(d)
  int i = 0;
  for (; i + 2 * D <= n; i += D) {  // steady state: every refill (row i + d + D) is a real row
#pragma unroll
    for (int d = 0; d < D; ++d) {
      use(i + d, x[d], sc[d]);
      __builtin_amdgcn_sched_barrier(0);  // consume slot d, then refill it
      FA_Q8_LOAD(d)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {  // drain: fewer than 2*D rows left
    if (i + d < n) {
      use(i + d, x[d], sc[d]);
      if (i + d + D < n) FA_Q8_LOAD(d)
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (i + D + d < n) use(i + D + d, x[d], sc[d]);
#undef FA_Q8_LOAD
}

// fa_deq_fold_q8.  Per column and row, every operation rounded to fp32 and none contracted:
//   x = scale * float(code);  center: x = g + x;  acc = acc + weight * x
// acc_in == NULL (wave-uniform) opens the round: the sums start at -0.0, the identity of the fp32
// add (-0.0 + t == t for every t, -0.0 and subnormals included), so row 0's product is the first sum
// bit for bit and every row runs the same code.  Else the piece's carried sums are loaded through a
// range-checked descriptor.  acc_out may be acc_in: a lane reads its quads before it writes them
// and no other lane touches them.  The code rows' descriptor range is the piece's columns rounded
// up to a dword (inside the row: strides are multiples of 16); the store's range is the columns
// themselves, so lanes past the end are dropped.
template <int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void deq_fold_kernel(const int8_t* __restrict__ stack, int64_t stride, int n,
                                                          const float* __restrict__ scales, int64_t sstride,
                                                          const float* __restrict__ weights,
                                                          const float* __restrict__ center, const float* acc_in,
                                                          float* acc_out, int64_t col0, int64_t ncols) {
  const int64_t chunks = (ncols + 1023) / 1024;
  const int64_t gr = gridDim.x;
  const int64_t k = (chunks + gr * W * V - 1) / (gr * W * V);  // rounds
  const int64_t pc = (chunks + gr * k - 1) / (gr * k);         // chunks per piece (<= W*V)
  const int64_t pieces = (chunks + pc - 1) / pc;
  const bool first = acc_in == nullptr;
  const bool cen = center != nullptr;
  const int q0 = (int)threadIdx.x * 4;  // the lane's first fp32 quad of slot 0: chunk `wave`, 16 columns per lane
  for (int64_t p = blockIdx.x; p < pieces; p += gr) {
    const int64_t cb = p * pc;
    const int64_t ce = cb + pc < chunks ? cb + pc : chunks;
    const int64_t colb = cb * 1024;
    const int64_t cend = ce * 1024 < ncols ? ce * 1024 : ncols;
    const int cols = cend > colb ? (int)(cend - colb) : 0;
    if (cols <= 0) continue;
    const __amdgpu_buffer_rsrc_t rg = col_rsrc<const float>(cen ? center + col0 : nullptr, colb / 4, cols);
    XV g[V][4], acc[V][4];
    if (cen) {
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 4; ++j) g[v][j] = buf_load_tquad<float>(rg, q0 + v * W * 256 + j);
    }
    if (first) {
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[v][j] = XV{-0.f, -0.f, -0.f, -0.f};
    } else {
      const __amdgpu_buffer_rsrc_t ra = col_rsrc<const float>(acc_in, colb / 4, cols);
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[v][j] = buf_load_tquad<float>(ra, q0 + v * W * 256 + j);
    }
    const char* tile0 = reinterpret_cast<const char*>(stack + col0 + colb);
    const char* sc0 = reinterpret_cast<const char*>(scales + col0 / 1024 + cb);
    const uint32_t bytes = ((uint32_t)cols + 3u) & ~3u;
    auto sweep = [&](auto with_center) {
      rows_each<V, D, W, NT>(tile0, stride, bytes, sc0, sstride * 4, (uint32_t)(ce - cb) * 4u, n,
                             [&](int i, const u32x4(&x)[V], const float(&sc)[V]) {
                               const float a = weights[i];
#pragma unroll
                               for (int v = 0; v < V; ++v)
#pragma unroll
                                 for (int j = 0; j < 4; ++j) {
                                   XV t = sc[v] * codes_of(x[v][j]);
                                   if constexpr (decltype(with_center)::value) t = g[v][j] + t;
                                   acc[v][j] = acc[v][j] + a * t;
                                 }
                             });
    };
    if (cen) sweep(std::true_type{}); else sweep(std::false_type{});
    const __amdgpu_buffer_rsrc_t ro = col_rsrc<float>(acc_out, colb / 4, cols);
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int j = 0; j < 4; ++j) buf_store_tquad<float>(ro, q0 + v * W * 256 + j, acc[v][j]);
  }
}

}  // namespace quant
}  // namespace fa
