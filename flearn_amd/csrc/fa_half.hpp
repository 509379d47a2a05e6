// fa_half.hpp — float16 client stacks (fa_reduce_f16): the packed-half accumulation policies and
// the oct row pipeline.  Included by fa_reduce.hip and, through fa_device.hpp, by the tuning tools.
//
// float16 client stacks (fa_reduce_f16).  The fp32 row pipeline's shape with 2-byte elements: a
// lane's 16-B load is an OCT (8 contiguous halves), a wave instruction still reads 1 KiB of one
// row, rows roll through a D-deep register pipeline in list order, and the piece's end is covered
// by the descriptors' range check.  That check is per DWORD, so a piece with an odd column count
// loads its rows through a range rounded up to an even count (the row's next half comes along; it
// lies inside the row, whose stride is a multiple of 8, and its lane slot is never stored), and
// stores out16 through a range rounded DOWN to an even count, the last odd half by one 2-byte
// store of the lane that owns it.
// What numpy / torch compute on float16 uploads depends on the weight type (semantics.resolve_half;
// DESIGN.md section 10); the policies below are those arithmetics.  numpy's and torch's half `+`
// and `*` are the correctly rounded IEEE operations (computed in fp32 and rounded again, which is
// the same: 24 >= 2*11 + 2), i.e. v_pk_mul_f16 / v_pk_add_f16, subnormals kept (the kernels run
// with float_denorm_mode_16_64 = 3).  No contraction (-ffp-contract=off): fl16(a*x) + acc has two
// roundings.
#pragma once

#include "fa_numerics.hpp"

namespace fa {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef double f64x8 __attribute__((ext_vector_type(8)));

// numpy float16 arrays x Python float/int/bool or np.float16 weights: fl16(fl16(a)*x), f16 sum.
// The weight arrives as a float holding the half value (exact) and is narrowed back (exact).
struct AccH16Pk {
  typedef float w_t;
  typedef h16x8 acc_v;
  static __device__ __forceinline__ h16x8 mul(float w, h16x8 x) { return (h16x8)(_Float16)w * x; }
};
// torch float16 tensors x Python float/int weights: the product is fl16(fl32(fl32(a)*fl32(x)))
// (two roundings: TensorIterator multiplies in float and stores half), the sum is f16.
struct AccH16Torch {
  typedef float w_t;
  typedef h16x8 acc_v;
  static __device__ __forceinline__ h16x8 mul(float w, h16x8 x) {
    return __builtin_convertvector((f32x8)w * __builtin_convertvector(x, f32x8), h16x8);
  }
};
// numpy float16 arrays x np.float32 weights: promoted to fp32 (the fp32 reduce's W32_DIV32)
struct AccH16W32 {
  typedef float w_t;
  typedef f32x8 acc_v;
  static __device__ __forceinline__ f32x8 mul(float w, h16x8 x) { return (f32x8)w * __builtin_convertvector(x, f32x8); }
};
// numpy float16 arrays x np.float64 / np.int64 weights: promoted to f64 (the fp32 reduce's W64)
struct AccH16W64 {
  typedef double w_t;
  typedef f64x8 acc_v;
  static __device__ __forceinline__ f64x8 mul(double w, h16x8 x) { return (f64x8)w * __builtin_convertvector(x, f64x8); }
};

// How the sum is divided (np.divide(w, np.sum(a)), strategy.py:127-129) and in which type the
// result is born; the other outputs are conversions of that result.
enum DivH16 : int {
  kDivF64 = 0,  // f64 result: q = fl64(acc) / W;  out32 = fl32(q), out16 = fl16(fl32(q)) (what
                // load_state_dict of the float64 result into a half module stores)
  kDivF32 = 1,  // np.float32 weights: q = acc / fl32(W), a float32 result
  kDivF16 = 2   // np.float16 weights: q = fl16(fl32(acc) / fl32(W16)), a float16 result
};

struct EpiH16 {
  double denom;
  uint16_t* out16;
  float* out32;
  double* out64;
};

template <bool NT>
__device__ __forceinline__ h16x8 buf_load_oct(__amdgpu_buffer_rsrc_t r, int voff) {
  return __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, NT ? 2 : 0));
}

// rows_sweep for octs: acc[v] = sum_i mul(w[i], x[i]) in list order, the first product
// initialising the sum; `bytes` is the (even-rounded) valid range of every row of the piece.
template <class HP, int V, int D, int W, bool NT>
__device__ __forceinline__ void rows_sweep_h16(const char* tile0, int64_t row_bytes, uint32_t bytes, int n,
                                               const typename HP::w_t* __restrict__ w,
                                               typename HP::acc_v (&acc)[V]) {
  const int voff = (int)threadIdx.x * 16;
  auto row = [&](int i) { return tile0 + (int64_t)i * row_bytes; };
  h16x8 x[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (1 + d < n) {
      const __amdgpu_buffer_rsrc_t r = row_rsrc(row(1 + d), bytes);
#pragma unroll
      for (int v = 0; v < V; ++v) x[d][v] = buf_load_oct<NT>(r, voff + v * 64 * W * 16);
    }
  {
    const __amdgpu_buffer_rsrc_t r = row_rsrc(row(0), bytes);
    const typename HP::w_t w0 = w[0];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = HP::mul(w0, buf_load_oct<NT>(r, voff + v * 64 * W * 16));
  }
  int i = 1;
  for (; i + 2 * D <= n; i += D) {  // steady state: every refill is a real row
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const typename HP::w_t wi = w[i + d];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = acc[v] + HP::mul(wi, x[d][v]);
      __builtin_amdgcn_sched_barrier(0);  // consume slot d, then refill it (see rows_sweep)
      const __amdgpu_buffer_rsrc_t r = row_rsrc(row(i + d + D), bytes);
#pragma unroll
      for (int v = 0; v < V; ++v) x[d][v] = buf_load_oct<NT>(r, voff + v * 64 * W * 16);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {  // drain: fewer than 2*D rows left (wave-uniform branches)
    if (i + d < n) {
      const typename HP::w_t wi = w[i + d];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = acc[v] + HP::mul(wi, x[d][v]);
      if (i + d + D < n) {
        const __amdgpu_buffer_rsrc_t r = row_rsrc(row(i + d + D), bytes);
#pragma unroll
        for (int v = 0; v < V; ++v) x[d][v] = buf_load_oct<NT>(r, voff + v * 64 * W * 16);
      }
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (i + D + d < n) {
      const typename HP::w_t wi = w[i + D + d];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = acc[v] + HP::mul(wi, x[d][v]);
    }
  }
}

// Divide and store one piece: columns [cbase, cbase + cols) of the outputs, lane slots
// o = threadIdx.x + v*STEP (octs of the piece).  Every store goes through a descriptor whose range
// is the piece's columns (a null output: an empty range), 16 B per instruction.
template <class HP, int DIV, int V, int STEP>
__device__ __forceinline__ void finish_piece_h16(const EpiH16& e, int64_t cbase, int cols,
                                                 const typename HP::acc_v (&acc)[V]) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  typedef float f4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t r16 = row_rsrc(e.out16 + cbase, e.out16 ? (uint32_t)(cols & ~1) * 2u : 0u);
  const __amdgpu_buffer_rsrc_t r32 = row_rsrc(e.out32 + cbase, e.out32 ? (uint32_t)cols * 4u : 0u);
  const __amdgpu_buffer_rsrc_t r64 = row_rsrc(e.out64 + cbase, e.out64 ? (uint32_t)cols * 8u : 0u);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = ((int)threadIdx.x + v * STEP) * 8;  // the oct's first column in the piece
    f64x8 o64;
    f32x8 o32;
    h16x8 o16;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (DIV == kDivF64) {
        const double q = (double)acc[v][j] / e.denom;
        o64[j] = q;
        o32[j] = (float)q;
        o16[j] = (_Float16)o32[j];
      } else if constexpr (DIV == kDivF32) {
        const float q = (float)acc[v][j] / (float)e.denom;
        o64[j] = (double)q;
        o32[j] = q;
        o16[j] = (_Float16)q;
      } else {
        const _Float16 q = (_Float16)((float)acc[v][j] / (float)e.denom);
        o64[j] = (double)q;
        o32[j] = (float)q;
        o16[j] = q;
      }
    }
    if (e.out64) {
      // whole-line f64 stores: a lane's oct is 64 B of f64, so stored lane by lane each instruction
      // would write every fourth 16 B of the wave's 4 KiB.  The wave regroups its 256 16-B units
      // through LDS (4 KiB per wave, as buf_store_tquad's XL does for quads) and instruction j
      // writes the j-th contiguous KiB.  100 x 25.6 M numpy-weak with out64: 0.915 -> 0.781 ms,
      // 72.8 -> 85.2% of 8 TB/s (tools/bench_half.py).  Wave-convergent:
      // e.out64 and the caller's branches are block-uniform.
      __shared__ d2 xch[STEP / 64][256];
      int tid = (int)threadIdx.x;
      asm volatile("" : "+v"(tid));  // (see buf_store_tquad: keeps the addresses out of the sweep)
      const int lane = tid & 63;
      d2* s = xch[tid >> 6];
#pragma unroll
      for (int j = 0; j < 4; ++j) s[4 * lane + j] = d2{o64[2 * j], o64[2 * j + 1]};
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      __builtin_amdgcn_wave_barrier();
      d2 t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = s[64 * j + lane];
      const int base = (tid - lane + v * STEP) * 64;  // the wave's first byte of this slot
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, t[j]), r64, base + 1024 * j + lane * 16, 0,
                                               kEpiStore64Aux);
      __builtin_amdgcn_wave_barrier();  // the next slot's writes come after these reads
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
    }
    if (e.out32) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        __builtin_amdgcn_raw_buffer_store_b128(
            __builtin_bit_cast(u32x4, f4{o32[4 * j], o32[4 * j + 1], o32[4 * j + 2], o32[4 * j + 3]}), r32,
            c * 4 + 16 * j, 0, kEpiStoreAux);
    }
    if (e.out16) {
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o16), r16, c * 2, 0, kEpiStoreAux);
      if (cols & 1) {  // the piece's last, odd half: its dword is outside r16's range
        const int k = cols - 1 - c;
        if (k >= 0 && k < 8) {
          _Float16 last = o16[0];
#pragma unroll
          for (int j = 1; j < 8; ++j) last = k == j ? o16[j] : last;
          e.out16[cbase + cols - 1] = __builtin_bit_cast(uint16_t, last);
        }
      }
    }
  }
}

// reduce_kernel_rows for float16 stacks: equal interleaved pieces of pc <= W*V 1-KiB chunks (512
// halves of a row each), block b sweeping pieces b, b+grid, ...; D = rows in flight per slot.
template <class HP, int DIV, int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void reduce_kernel_rows_h16(const uint16_t* __restrict__ stack, int64_t stride,
                                                                 int n, const typename HP::w_t* __restrict__ w,
                                                                 int64_t col0, int64_t ncols, EpiH16 e) {
  const int64_t nocts = (ncols + 7) / 8;
  const int64_t chunks = (nocts + 63) / 64;
  const int64_t g = gridDim.x;
  const int64_t k = (chunks + g * W * V - 1) / (g * W * V);  // rounds
  const int64_t pc = (chunks + g * k - 1) / (g * k);         // chunks per piece (<= W*V)
  const int64_t pieces = (chunks + pc - 1) / pc;
  for (int64_t p = blockIdx.x; p < pieces; p += g) {
    const int64_t ob = p * pc * 64;
    const int64_t oe = ob + pc * 64 < nocts ? ob + pc * 64 : nocts;
    const int64_t cend = oe * 8 < ncols ? oe * 8 : ncols;
    const int cols = cend > ob * 8 ? (int)(cend - ob * 8) : 0;
    if (cols > 0) {
      typename HP::acc_v acc[V];
      rows_sweep_h16<HP, V, D, W, NT>(reinterpret_cast<const char*>(stack + col0 + ob * 8), stride * 2,
                                      (uint32_t)((cols + 1) & ~1) * 2u, n, w, acc);
      finish_piece_h16<HP, DIV, V, 64 * W>(e, ob * 8, cols, acc);
    }
  }
}

}  // namespace fa
