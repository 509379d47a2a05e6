// fa_mx.hpp — OCP Microscaling uploads (fa_deq_fold_mx): the weighted fp32 sum
// of one chunk of clients whose rows are MXFP4 (E2M1, two codes per byte, even column in the low
// nibble) or MXFP8 (E4M3 "fn", one code per byte) with one E8M0 scale byte per 32 columns, decoded in
// registers by gfx950's scaled converts.  fa::q4::deq_fold4_kernel's sibling with the family's work
// split (equal interleaved pieces of <= W*V chunks derived from the grid, per-row range-checked
// descriptors on running 64-bit scalar row pointers, a D-deep load pipeline, the piece's centre and
// sums in registers, one range-checked store per piece; no LDS, no scratch).  What differs:
//   * a lane owns 32 consecutive columns of a row — exactly one scale block — for both element
//     types: one 16-B load of FP4 codes, or two 16-B loads of FP8 codes at lane * 32 and
//     lane * 32 + 16.  A wave's chunk is 64 lanes x 32 = 2048 columns and 64 scale bytes either way,
//     so the two types share the piece arithmetic, the sums' layout and the store;
//   * the lane's scale is ONE BYTE, loaded per lane and row (byte `lane` of the chunk's 64) in the
//     codes' pipeline slot, issued after them and returned in order under the same vmcnt;
//   * decoding is the hardware's: v_cvt_scalef32_pk_f32_fp4 / _fp8 turn two codes into two fp32
//     values already multiplied by the block's scale, given as the float 2^(e - 127) = bits e << 23
//     (a normal for every legal e), formed once per lane and row.  op_sel picks the byte of the dword
//     (FP4) or its half (FP8); 16 converts decode a lane's 32 columns.
// Included by fa_mx.hip only.  The kernel lives in fa::mx: the inventories pin the kernels of fa,
// fa::clip, fa::clipfold, fa::noise and fa::quant.
#pragma once

#include <type_traits>

#include "fa_numerics.hpp"

namespace fa {
namespace mx {

typedef vec4<float>::type XV;
typedef float XP __attribute__((ext_vector_type(2)));

constexpr int kChunk = 2048;  // columns of one wave-chunk (FA_MX_CHUNK): 64 lanes x 32
constexpr int kBlock = 32;    // columns per scale byte (FA_MX_BLOCK): one lane

template <int ELEM>
struct Codes {
  static_assert(ELEM == 4 || ELEM == 8, "MXFP4 or MXFP8");
  static constexpr int kLoads = ELEM / 4;           // 16-B loads per lane, row and chunk
  static constexpr int kLaneBytes = 16 * kLoads;    // a lane's 32 columns
  u32x4 q[kLoads];
};

// Columns 4 Q .. 4 Q + 3 of the lane's 32, times the scale `s`: two packed converts.  FP4: dword
// Q / 2 holds columns 8 (Q / 2) .. + 7, a byte two of them (low nibble first).  FP8: dword Q is the
// quad, its low half the first two columns.
template <int ELEM, int Q>
__device__ __forceinline__ XV quad_of(const Codes<ELEM>& c, float s) {
  XP lo, hi;
  if constexpr (ELEM == 4) {
    const uint32_t w = c.q[0][Q / 2];
    lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, (Q & 1) * 2);
    hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, (Q & 1) * 2 + 1);
  } else {
    const uint32_t w = c.q[Q / 4][Q % 4];
    lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, s, false);
    hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, s, true);
  }
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}

// q4::rows_each's pipeline: rows 0..n-1 of the piece in order, slot d holding row i + d's codes
// x[d][v] (chunk v * W + wave of the piece, columns lane * 32 .. + 31 of it) and the lane's scale
// byte e[d][v]; use(i, x, e) consumes row i.  Two running scalar row pointers.  All loads are
// range-checked: bytes past the piece's end read 0 (code 0 with scale bits 0: what those lanes
// compute is dropped by the store).
template <int ELEM, int V, int D, int W, bool NT, class Use>
__device__ __forceinline__ void rows_each(const char* tile0, int64_t row_bytes, uint32_t bytes, const char* sc0,
                                          int64_t sc_row_bytes, uint32_t sc_bytes, int n, Use&& use) {
  constexpr int LB = Codes<ELEM>::kLaneBytes;
  const int voff = (int)threadIdx.x * LB;
  const int svoff = (int)threadIdx.x;
  const char* pn = tile0;  // the next row to load
  const char* ps = sc0;
#define FA_MX_LOAD(slot)                                                                             \
  {                                                                                                  \
    const __amdgpu_buffer_rsrc_t r_ = row_rsrc(pn, bytes);                                           \
    const __amdgpu_buffer_rsrc_t q_ = row_rsrc(ps, sc_bytes);                                        \
    _Pragma("unroll") for (int v = 0; v < V; ++v) {                                                  \
      _Pragma("unroll") for (int l = 0; l < Codes<ELEM>::kLoads; ++l)                                \
        x[slot][v].q[l] = __builtin_amdgcn_raw_buffer_load_b128(r_, voff + v * 64 * W * LB + l * 16, 0, NT ? 2 : 0); \
      e[slot][v] = __builtin_amdgcn_raw_buffer_load_b8(q_, svoff + v * W * 64, 0, 0);                \
    }                                                                                                \
    pn += row_bytes;                                                                                 \
    ps += sc_row_bytes;                                                                              \
    asm volatile("" : "+s"(pn), "+s"(ps));                                                           \
  }
  Codes<ELEM> x[D][V];
  uint8_t e[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < n) FA_MX_LOAD(d)
  int i = 0;
  for (; i + 2 * D <= n; i += D) {  // steady state: every refill (row i + d + D) is a real row
#pragma unroll
    for (int d = 0; d < D; ++d) {
      use(i + d, x[d], e[d]);
      __builtin_amdgcn_sched_barrier(0);  // consume slot d, then refill it
      FA_MX_LOAD(d)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {  // drain: fewer than 2*D rows left
    if (i + d < n) {
      use(i + d, x[d], e[d]);
      if (i + d + D < n) FA_MX_LOAD(d)
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (i + D + d < n) use(i + D + d, x[d], e[d]);
#undef FA_MX_LOAD
}

// fa_deq_fold_mx.  Per column and row, every operation rounded to fp32 and none contracted:
//   x = decode(code) * 2^(e - 127);  center: x = g + x;  acc = acc + weight * x
// x is the convert's result.  It is exact: a decoded E2M1 or E4M3 value has at most 4 significant
// bits and, for a legal scale byte (27 <= e <= 227), the product is zero or an fp32 normal between
// 2^-109 and 448 * 2^100, so neither rounding nor subnormal flushing inside the convert can touch it.
// What is hoisted is the scale operand alone (bits e << 23, one shift per lane and row, shared by the
// 16 converts).  The weight is NOT folded into it: the scale operand may be read as a power of two
// only (its exponent field), and weight * x must be its own rounding, followed by the add's — a
// packed multiply and a packed add (v_pk_mul_f32, v_pk_add_f32), never an fma, which would contract
// the two.  With a centre there is one more packed add before the product.  So the bits are
// fa_fold's on the dequantized rows, -0.0 (code S.000...0 decodes to -0.0) and overflow to inf
// included; E4M3's NaN codes give NaN sums, and only a NaN's bits are free.
// acc_in == NULL (wave-uniform) opens the round at -0.0, the identity of the fp32 add, so row 0's
// product is the first sum bit for bit; else the piece's carried sums are loaded through a
// range-checked descriptor.  acc_out may be acc_in: a lane reads its quads before it writes them and
// no other lane touches them.  A lane's 32 columns of chunk c are fp32 quads c * 512 + lane * 8 +
// 0..7.  The code rows' descriptor range is the piece's bytes rounded up to a dword (inside the row:
// strides are multiples of 16), the scale rows' the piece's blocks, the store's the columns
// themselves, so what a ragged end computes from the codes past it is dropped.
template <int ELEM, int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void mx_fold_kernel(const uint8_t* __restrict__ stack, int64_t stride, int n,
                                                         const uint8_t* __restrict__ scales, int64_t sstride,
                                                         const float* __restrict__ weights,
                                                         const float* __restrict__ center, const float* acc_in,
                                                         float* acc_out, int64_t col0, int64_t ncols) {
  constexpr int PB = 8 / ELEM;  // columns per byte
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
    const char* tile0 = reinterpret_cast<const char*>(stack + (col0 + colb) / PB);
    const char* sc0 = reinterpret_cast<const char*>(scales + (col0 + colb) / kBlock);
    const uint32_t bytes = (((uint32_t)cols + (uint32_t)PB - 1u) / (uint32_t)PB + 3u) & ~3u;
    const uint32_t sc_bytes = ((uint32_t)cols + (uint32_t)kBlock - 1u) / (uint32_t)kBlock;
    auto sweep = [&](auto with_center) {
      rows_each<ELEM, V, D, W, NT>(
          tile0, stride, bytes, sc0, sstride, sc_bytes, n,
          [&](int i, const Codes<ELEM>(&x)[V], const uint8_t(&e)[V]) {
            const float a = weights[i];
#pragma unroll
            for (int v = 0; v < V; ++v) {
              const float s = __builtin_bit_cast(float, (uint32_t)e[v] << 23);  // 2^(e - 127)
#define FA_MX_QUAD(Q)                                                          \
  {                                                                            \
    XV t = quad_of<ELEM, Q>(x[v], s);                                          \
    if constexpr (decltype(with_center)::value) t = g[v][Q] + t;               \
    acc[v][Q] = acc[v][Q] + a * t;                                             \
  }
              FA_MX_QUAD(0) FA_MX_QUAD(1) FA_MX_QUAD(2) FA_MX_QUAD(3)
              FA_MX_QUAD(4) FA_MX_QUAD(5) FA_MX_QUAD(6) FA_MX_QUAD(7)
#undef FA_MX_QUAD
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

}  // namespace mx
}  // namespace fa
