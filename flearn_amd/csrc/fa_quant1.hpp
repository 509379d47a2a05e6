// fa_quant1.hpp — 1-bit sign uploads (fa_deq_fold_q1): the weighted fp32 sum
// of one chunk of clients whose rows are one sign bit per column (column c is bit c % 8 of byte
// c / 8, 1 = negative) with one fp32 magnitude per 128 columns.  A dequantized value is no product:
// it is the block's scale with the code's sign.  fa::q4::deq_fold4_kernel's sibling with the
// family's work split (equal interleaved pieces of <= W*V chunks derived from the grid, per-row
// range-checked descriptors on running 64-bit scalar row pointers, a D-deep load pipeline, the
// piece's centre and sums in registers, one range-checked store per piece).  What differs: a lane
// loads ONE DWORD per row, 32 columns, so a wave's chunk is 64 lanes x 4 B = 2048 columns = 16 scale
// blocks and four neighbouring lanes share a scale (a per-lane 4-byte load at
// ((chunk of the piece) * 16 + (lane >> 2)) * 4 of the scale row, riding the pipeline slot beside
// the row's codes); a row is 256 B per wave, so the depth D is set by load latency against two VGPRs
// per slot, not by bytes in flight (fa_quant1_geometry.hpp); and an element costs a shift, a
// bit-field insert and an add (sign_fold_kernel, below).  Included by fa_quant1.hip only.  The
// kernel lives in fa::q1: the inventories pin the kernels of fa, fa::clip, fa::clipfold, fa::noise
// and fa::quant.
#pragma once

#include <type_traits>

#include "fa_numerics.hpp"

namespace fa {
namespace q1 {

typedef vec4<float>::type XV;

constexpr int kChunk = 2048;  // columns of one wave-chunk (FA_Q1_CHUNK): 64 lanes x 4 B x 8
constexpr int kBlock = 128;   // columns per scale (FA_Q1_BLOCK): 4 lanes

// `mag` with the sign of columns 4 j .. 4 j + 3 of the lane's dword `w`: per element one shift that
// brings the column's bit to bit 31 and one v_bfi_b32 (copysign) that puts it on `mag`.
__device__ __forceinline__ XV signed_quad(float mag, uint32_t w, int j) {
  XV t;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    t[e] = __builtin_copysignf(mag, __builtin_bit_cast(float, w << (31 - (4 * j + e))));
  return t;
}

// q4::rows_each's pipeline on dword loads: rows 0..n-1 of the piece in order, slot d holding row
// i + d's code dword x[d][v] (chunk v * W + wave of the piece, columns lane * 32 .. + 31 of it) and
// the lane's scale sc[d][v] (block lane >> 2 of that chunk); use(i, x, sc) consumes row i.  Two
// running scalar row pointers.  Both loads are range-checked: bytes and blocks past the piece's end
// read 0.
template <int V, int D, int W, bool NT, class Use>
__device__ __forceinline__ void rows_each(const char* tile0, int64_t row_bytes, uint32_t bytes, const char* sc0,
                                          int64_t sc_row_bytes, uint32_t sc_bytes, int n, Use&& use) {
  const int voff = (int)threadIdx.x * 4;
  const int svoff = ((int)threadIdx.x >> 2) * 4;
  const char* pn = tile0;  // the next row to load
  const char* ps = sc0;
#define FA_Q1_LOAD(slot)                                                                           \
  {                                                                                                \
    const __amdgpu_buffer_rsrc_t r_ = row_rsrc(pn, bytes);                                         \
    const __amdgpu_buffer_rsrc_t q_ = row_rsrc(ps, sc_bytes);                                      \
    _Pragma("unroll") for (int v = 0; v < V; ++v) {                                                \
      x[slot][v] = __builtin_amdgcn_raw_buffer_load_b32(r_, voff + v * 64 * W * 4, 0, NT ? 2 : 0); \
      sc[slot][v] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(q_, svoff + v * W * 64, 0, 0)); \
    }                                                                                              \
    pn += row_bytes;                                                                               \
    ps += sc_row_bytes;                                                                            \
    asm volatile("" : "+s"(pn), "+s"(ps));                                                         \
  }
  uint32_t x[D][V];
  float sc[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < n) FA_Q1_LOAD(d)
  int i = 0;
  for (; i + 2 * D <= n; i += D) {  // steady state: every refill (row i + d + D) is a real row
#pragma unroll
    for (int d = 0; d < D; ++d) {
      use(i + d, x[d], sc[d]);
      __builtin_amdgcn_sched_barrier(0);  // consume slot d, then refill it
      FA_Q1_LOAD(d)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {  // drain: fewer than 2*D rows left
    if (i + d < n) {
      use(i + d, x[d], sc[d]);
      if (i + d + D < n) FA_Q1_LOAD(d)
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (i + D + d < n) use(i + D + d, x[d], sc[d]);
#undef FA_Q1_LOAD
}

// fa_deq_fold_q1.  Per column and row, every operation rounded to fp32 and none contracted:
//   x = copysign(scale, bit ? -1 : +1);  center: x = g + x;  acc = acc + weight * x
// Without a centre the product is hoisted: p = weight * |scale| is formed once per lane and row and
// an element's product is p with its sign bit replaced by (sign of p) xor (the column's bit) — the
// row's dword is complemented once when p is negative, so the element itself is a shift and a
// bit-field insert.  That is fl32(weight * x) bit for bit: |x| = |scale| for all 32 columns of the
// lane, round-to-nearest-even is symmetric in the sign (fl(a * (-s)) = -fl(a * s), overflow to inf
// and underflow included), and the sign of an IEEE product — of a zero and of an infinity too — is
// the xor of its operands' signs, which is what the complement computes.  Only a NaN product (a NaN
// weight, inf * 0) may differ, in its sign: a NaN's bits are free in this family.  With a centre
// nothing can be hoisted: t = g + x, acc += weight * t, as the siblings do.
// acc_in == NULL (wave-uniform) opens the round at -0.0, the identity of the fp32 add, so row 0's
// product is the first sum bit for bit; else the piece's carried sums are loaded through a
// range-checked descriptor.  acc_out may be acc_in: a lane reads its quads before it writes them and
// no other lane touches them.  A lane's 32 columns of chunk c are fp32 quads c * 512 + lane * 8 +
// 0..7.  The code rows' descriptor range is the piece's bytes rounded up to a dword (inside the row:
// strides are multiples of 16), the scale rows' the piece's blocks, the store's the columns
// themselves, so what a ragged end computes from the bits past it is dropped.
template <int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void sign_fold_kernel(const uint8_t* __restrict__ stack, int64_t stride, int n,
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
    const char* tile0 = reinterpret_cast<const char*>(stack + (col0 + colb) / 8);
    const char* sc0 = reinterpret_cast<const char*>(scales + (col0 + colb) / kBlock);
    const uint32_t bytes = (((uint32_t)cols + 7u) / 8u + 3u) & ~3u;
    const uint32_t sc_bytes = (((uint32_t)cols + (uint32_t)kBlock - 1u) / (uint32_t)kBlock) * 4u;
    auto sweep = [&](auto with_center) {
      rows_each<V, D, W, NT>(tile0, stride, bytes, sc0, sstride * 4, sc_bytes, n,
                             [&](int i, const uint32_t(&x)[V], const float(&sc)[V]) {
                               const float a = weights[i];
#pragma unroll
                               for (int v = 0; v < V; ++v) {
                                 if constexpr (decltype(with_center)::value) {
#pragma unroll
                                   for (int j = 0; j < 8; ++j) {
                                     const XV t = g[v][j] + signed_quad(sc[v], x[v], j);
                                     acc[v][j] = acc[v][j] + a * t;
                                   }
                                 } else {
                                   const float pr = a * __builtin_fabsf(sc[v]);  // the row's one product
                                   // the product's sign is xor-ed into every bit of the row at once
                                   const uint32_t w = x[v] ^ (uint32_t)(__builtin_bit_cast(int32_t, pr) >> 31);
#pragma unroll
                                   for (int j = 0; j < 8; ++j) acc[v][j] = acc[v][j] + signed_quad(pr, w, j);
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

}  // namespace q1
}  // namespace fa
