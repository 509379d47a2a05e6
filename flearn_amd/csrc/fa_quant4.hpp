// fa_quant4.hpp — int4 block-quantized uploads (fa_deq_fold_q4): the weighted
// fp32 sum of one chunk of clients whose rows are 4-bit two's-complement codes, two per byte (even
// column in the low nibble), with one fp32 scale per 128 columns, dequantized in registers.
// fa::quant::deq_fold_kernel's sibling with the family's work split (equal interleaved pieces of
// <= W*V chunks derived from the grid, per-row range-checked descriptors, one 16-B non-temporal
// load per lane and row, a D-deep load pipeline, the piece's centre and sums in registers, one
// range-checked store per piece).  What differs: a 16-B load is 32 columns, so a wave's chunk is
// 2048 columns = 16 scale blocks and four neighbouring lanes share a scale — a row's scale is a
// per-lane 4-byte load at ((chunk of the piece) * 16 + (lane >> 2)) * 4 of the scale row, riding
// the pipeline slot beside the row's codes (issued after them, returned in order under the same
// vmcnt); a lane keeps 32 sums per chunk; and a nibble becomes a float without a bit-field extract
// (codes16_of).  Included by fa_quant4.hip only.  The kernel lives in fa::q4: the inventories pin
// the kernels of fa, fa::clip, fa::clipfold, fa::noise and fa::quant.
#pragma once

#include <type_traits>

#include "fa_numerics.hpp"

namespace fa {
namespace q4 {

typedef vec4<float>::type XV;

constexpr int kChunk = 2048;  // columns of one wave-chunk (FA_Q4_CHUNK): 64 lanes x 16 B x 2
constexpr int kBlock = 128;   // columns per scale (FA_Q4_BLOCK): 4 lanes

// The 8 codes of one dword, each times 16, as two quads in column order.  A nibble moved to the top
// of its byte is the byte 16 q in two's complement: the high nibbles are there already
// (w & 0xF0F0F0F0), the low ones after a shift by 4, and the sign-extending byte select of the
// int-to-float conversion does the rest — 3 bit operations and 8 conversions per 8 codes.  16 q is
// exact in fp32; the caller multiplies by scale / 16.
__device__ __forceinline__ void codes16_of(uint32_t w, XV& even, XV& odd) {
  const uint32_t hi = w & 0xF0F0F0F0u;         // byte b: 16 * code 2b + 1
  const uint32_t lo = (w << 4) & 0xF0F0F0F0u;  // byte b: 16 * code 2b
  even = XV{(float)(int8_t)(lo), (float)(int8_t)(hi), (float)(int8_t)(lo >> 8), (float)(int8_t)(hi >> 8)};
  odd = XV{(float)(int8_t)(lo >> 16), (float)(int8_t)(hi >> 16), (float)(int8_t)(lo >> 24), (float)(int8_t)(hi >> 24)};
}

// quant::rows_each's pipeline: rows 0..n-1 of the piece in order, slot d holding row i + d's code
// quads x[d][v] and the lane's scale sc[d][v] (chunk v * W + wave of the piece, block lane >> 2 of
// it); use(i, x, sc) consumes row i.  Two running scalar row pointers.  The scale load's offset sits
// in the VGPR offset ((thread >> 2) * 4: 16 scales per wave) and the instruction offset
// (v * W * 64); both are range-checked, blocks past the piece's end read 0.
template <int V, int D, int W, bool NT, class Use>
__device__ __forceinline__ void rows_each(const char* tile0, int64_t row_bytes, uint32_t bytes, const char* sc0,
                                          int64_t sc_row_bytes, uint32_t sc_bytes, int n, Use&& use) {
  const int voff = (int)threadIdx.x * 16;
  const int svoff = ((int)threadIdx.x >> 2) * 4;
  const char* pn = tile0;  // the next row to load
  const char* ps = sc0;
#define FA_Q4_LOAD(slot)                                                                           \
  {                                                                                                \
    const __amdgpu_buffer_rsrc_t r_ = row_rsrc(pn, bytes);                                         \
    const __amdgpu_buffer_rsrc_t q_ = row_rsrc(ps, sc_bytes);                                      \
    _Pragma("unroll") for (int v = 0; v < V; ++v) {                                                \
      x[slot][v] = __builtin_amdgcn_raw_buffer_load_b128(r_, voff + v * 64 * W * 16, 0, NT ? 2 : 0); \
      sc[slot][v] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(q_, svoff + v * W * 64, 0, 0)); \
    }                                                                                              \
    pn += row_bytes;                                                                               \
    ps += sc_row_bytes;                                                                            \
    asm volatile("" : "+s"(pn), "+s"(ps));                                                         \
  }
  u32x4 x[D][V];
  float sc[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < n) FA_Q4_LOAD(d)
  int i = 0;
  for (; i + 2 * D <= n; i += D) {  // steady state: every refill (row i + d + D) is a real row
#pragma unroll
    for (int d = 0; d < D; ++d) {
      use(i + d, x[d], sc[d]);
      __builtin_amdgcn_sched_barrier(0);  // consume slot d, then refill it
      FA_Q4_LOAD(d)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {  // drain: fewer than 2*D rows left
    if (i + d < n) {
      use(i + d, x[d], sc[d]);
      if (i + d + D < n) FA_Q4_LOAD(d)
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (i + D + d < n) use(i + D + d, x[d], sc[d]);
#undef FA_Q4_LOAD
}

// fa_deq_fold_q4.  Per column and row, every operation rounded to fp32 and none contracted:
//   x = scale * float(code);  center: x = g + x;  acc = acc + weight * x
// computed as (scale / 16) * float(16 code): a legal scale is 0 or >= 2^-100 (FA_Q4_MIN_SCALE), so
// scale / 16 is exact (normal, or a zero of the same sign) and the product is the same real number,
// rounded once — the same bits, -0.0 and overflow to inf included.  acc_in == NULL (wave-uniform)
// opens the round at -0.0, the identity of the fp32 add, so row 0's product is the first sum bit
// for bit; else the piece's carried sums are loaded through a range-checked descriptor.  acc_out
// may be acc_in: a lane reads its quads before it writes them and no other lane touches them.  A
// lane's 32 columns of chunk c are fp32 quads c * 512 + lane * 8 + 0..7.  The code rows' descriptor
// range is the piece's bytes rounded up to a dword (inside the row: strides are multiples of 16),
// the scale rows' the piece's blocks, the store's the columns themselves, so what a ragged end
// computes from the nibbles past it is dropped.
template <int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void deq_fold4_kernel(const uint8_t* __restrict__ stack, int64_t stride, int n,
                                                           const float* __restrict__ scales, int64_t sstride,
                                                           const float* __restrict__ weights,
                                                           const float* __restrict__ center, const float* acc_in,
                                                           float* acc_out, int64_t col0, int64_t ncols) {
  const int64_t chunks = (ncols + kChunk - 1) / kChunk;
  const int64_t gr = gridDim.x;
  const int64_t k = (chunks + gr * W * V - 1) / (gr * W * V);  // rounds
  const int64_t pc = (chunks + gr * k - 1) / (gr * k);         // chunks per piece (<= W*V)
  const int64_t pieces = (chunks + pc - 1) / pc;
  const bool first = acc_in == nullptr;
  const bool cen = center != nullptr;
  const int q0 = (int)threadIdx.x * 8;  // the lane's first fp32 quad of slot 0: chunk `wave`, 32 columns per lane
  for (int64_t p = blockIdx.x; p < pieces; p += gr) {
    const int64_t cb = p * pc;
    const int64_t ce = cb + pc < chunks ? cb + pc : chunks;
    const int64_t colb = cb * kChunk;
    const int64_t cend = ce * kChunk < ncols ? ce * kChunk : ncols;
    const int cols = cend > colb ? (int)(cend - colb) : 0;
    if (cols <= 0) continue;
    const __amdgpu_buffer_rsrc_t rg = col_rsrc<const float>(cen ? center + col0 : nullptr, colb / 4, cols);
    XV g[V][8], acc[V][8];
    if (cen) {
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 8; ++j) g[v][j] = buf_load_tquad<float>(rg, q0 + v * W * 512 + j);
    }
    if (first) {
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[v][j] = XV{-0.f, -0.f, -0.f, -0.f};
    } else {
      const __amdgpu_buffer_rsrc_t ra = col_rsrc<const float>(acc_in, colb / 4, cols);
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[v][j] = buf_load_tquad<float>(ra, q0 + v * W * 512 + j);
    }
    const char* tile0 = reinterpret_cast<const char*>(stack + (col0 + colb) / 2);
    const char* sc0 = reinterpret_cast<const char*>(scales + (col0 + colb) / kBlock);
    const uint32_t bytes = (((uint32_t)cols + 1u) / 2u + 3u) & ~3u;
    const uint32_t sc_bytes = (((uint32_t)cols + (uint32_t)kBlock - 1u) / (uint32_t)kBlock) * 4u;
    auto sweep = [&](auto with_center) {
      rows_each<V, D, W, NT>(tile0, stride, bytes, sc0, sstride * 4, sc_bytes, n,
                             [&](int i, const u32x4(&x)[V], const float(&sc)[V]) {
                               const float a = weights[i];
#pragma unroll
                               for (int v = 0; v < V; ++v) {
                                 const float s16 = sc[v] * 0.0625f;  // exact: see above
#pragma unroll
                                 for (int j = 0; j < 4; ++j) {
                                   XV c[2];
                                   codes16_of(x[v][j], c[0], c[1]);
#pragma unroll
                                   for (int h = 0; h < 2; ++h) {
                                     XV t = s16 * c[h];
                                     if constexpr (decltype(with_center)::value) t = g[v][2 * j + h] + t;
                                     acc[v][2 * j + h] = acc[v][2 * j + h] + a * t;
                                   }
                                 }
                               }
                             });
    };
    if (cen) sweep(std::true_type{}); else sweep(std::false_type{});
    const __amdgpu_buffer_rsrc_t ro = col_rsrc<float>(acc_out, colb / 4, cols);
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int j = 0; j < 8; ++j) buf_store_tquad<float>(ro, q0 + v * W * 512 + j, acc[v][j]);
  }
}

}  // namespace q4
}  // namespace fa
