// fa_trim.hpp — coordinate-wise trimmed sums (fa_trim_sum): the totalOrder keys, the in-register
// sorting network and the two trim kernels.  Included by fa_rows.hip and, through fa_device.hpp,
// by the tuning tools.
#pragma once

#include <type_traits>
#include <utility>

#include "fa_geometry.hpp"
#include "fa_numerics.hpp"

namespace fa {

// ---------------------------------------------------------------------------------------------
// Coordinate-wise trimmed sums (fa_trim_sum): per column, the clients' values in
// IEEE totalOrder, the `trim` smallest and largest dropped, the rest summed in ascending order.
// ---------------------------------------------------------------------------------------------
// totalOrder of fp32 bit patterns as the signed-integer order of the key (an involution: the same
// two operations map a key back)
__device__ __forceinline__ int trim_key(int b) { return b ^ ((b >> 31) & 0x7fffffff); }
__device__ __forceinline__ int64_t trim_key(int64_t b) { return b ^ ((b >> 63) & INT64_MAX); }

template <int A, int B, bool ON, int NP>
__device__ __forceinline__ void trim_exchange(int (&key)[NP]) {
  if constexpr (ON) {  // v_min_i32 / v_max_i32 on two named registers
    int lo = key[A] < key[B] ? key[A] : key[B], hi = key[A] < key[B] ? key[B] : key[A];
    // both results made opaque here, in program order: left to the scheduler, a layer's NP/2
    // minima are all computed before its maxima and the kernel needs 2 NP registers (dependent
    // VALU operations issue back to back anyway)
    asm volatile("" : "+v"(lo), "+v"(hi));
    key[A] = lo;
    key[B] = hi;
  }
}

template <int NP, int P, int K, int... M>
__device__ __forceinline__ void trim_layer(int (&key)[NP], std::integer_sequence<int, M...>) {
  (trim_exchange<trim_net_pair(NP, P, K, M).a, trim_net_pair(NP, P, K, M).b, trim_net_pair(NP, P, K, M).on>(key), ...);
}

// layers (P, K), (P, K/2), ..., (P, 1), (2P, 2P), ... of the network in fa_geometry.hpp
template <int NP, int P = 1, int K = 1>
__device__ __forceinline__ void trim_sort(int (&key)[NP]) {
  trim_layer<NP, P, K>(key, std::make_integer_sequence<int, NP / 2>{});
  if constexpr (K > 1)
    trim_sort<NP, P, K / 2>(key);
  else if constexpr (2 * P < NP)
    trim_sort<NP, 2 * P, 2 * P>(key);
}

// fp32 rows, n <= NP clients.  A lane owns one column: a block of W waves owns a piece of 64 * W
// consecutive columns (256 B of every row per wave) and strides over the window's pieces by the
// grid.  Per piece every row is read through a range-checked descriptor (row_rsrc) whose range is
// the piece's valid bytes — lanes past the ragged end load 0 and their stores are dropped by the
// output descriptor's range — one dword per lane and row, all n loads issued before the first
// compare, straight into the NP sort registers; slots >= n hold the key 0x7fffffff, which sorts
// last and never enters the sum (a +NaN with that payload ties with it: the same bits).  The sort
// is Batcher's odd-even merge sort, fully unrolled v_min_i32 / v_max_i32 pairs on compile-time
// register indices (trim_net_pair: 1,471 exchanges at NP = 128); then ranks trim .. n - trim - 1
// are mapped back and summed in ascending order, the first kept value initialising the sum, under
// wave-uniform scalar bounds.  No scratch: every index of key[] is a constant.
template <int NP, int W, bool NT>
__global__ __launch_bounds__(64 * W, trim_waves_per_simd(NP)) void trim_kernel_rows(const float* __restrict__ stack, int64_t stride, int n,
                                                          int trim, float* __restrict__ acc_out, int64_t col0,
                                                          int64_t ncols) {
  static_assert(NP >= 4 && (NP & (NP - 1)) == 0, "the network sorts a power of two");
  const int64_t pieces = (ncols + 64 * W - 1) / (64 * W);
  const int64_t row_bytes = stride * 4;
  const int voff = (int)threadIdx.x * 4;
  for (int64_t p = blockIdx.x; p < pieces; p += gridDim.x) {
    // the bounds made opaque per piece: as loop invariants every one of the ~3 NP wave-uniform
    // conditions below is computed ahead of the loop and kept in a scalar register pair (NP = 128:
    // 566 of them spilled)
    int nn = n, lo = trim;
    asm volatile("" : "+s"(nn), "+s"(lo));
    const int hi = nn - lo;  // kept ranks [lo, hi)
    const int64_t c0 = p * (64 * W);
    const int cols = ncols - c0 < 64 * W ? (int)(ncols - c0) : 64 * W;
    const uint32_t bytes = (uint32_t)cols * 4u;
    const char* pn = reinterpret_cast<const char*>(stack + col0 + c0);  // the next row to load
    int key[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      // n > NP / 2 (NP is the smallest that holds n), so only the upper half is conditional
      if (i < (NP > 4 ? NP / 2 : 1) || i < nn) {
        key[i] = (int)__builtin_amdgcn_raw_buffer_load_b32(row_rsrc(pn, bytes), voff, 0, NT ? 2 : 0);
        pn += row_bytes;
        asm volatile("" : "+s"(pn));  // one running scalar pointer, as in rows_fold_sweep
        // the loads stay in row order, each descriptor's four scalars built next to its load
        __builtin_amdgcn_sched_barrier(0);
      } else {
        key[i] = 0x7fffffff;
      }
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) key[i] = trim_key(key[i]);
    trim_sort<NP>(key);
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < NP; ++r) {
      if (r >= lo && r < hi) {
        const float x = __builtin_bit_cast(float, trim_key(key[r]));
        acc = r == lo ? x : acc + x;
      }
    }
    const __amdgpu_buffer_rsrc_t ro = col_rsrc<float>(acc_out, c0 / 4, cols);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, acc), ro, voff, 0, kEpiStoreAux);
  }
}

// The 8-byte kinds (T = double: float64 buffers; int64_t: BN counters — small buckets): one column
// per lane, grid-stride, no local array.  The next key in order (the smallest above the last one,
// with its multiplicity) is selected by a pass over the column's n values, so a column costs
// O(n^2) loads, from cache after the first pass.  Correct for any n <= FA_TRIM_MAX_CLIENTS, and
// not a hot path.  Sums over ranks trim .. n - trim - 1 in ascending order; int64 wraps.
template <typename T>
__global__ __launch_bounds__(kThreads) void trim_kernel_elem(const T* __restrict__ stack, int64_t stride, int n,
                                                             int trim, T* __restrict__ acc_out, int64_t col0,
                                                             int64_t ncols) {
  static_assert(sizeof(T) == 8, "8-byte kinds");
  constexpr bool kFloat = !std::is_integral<T>::value;
  const int lo = trim, hi = n - trim;
  for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * kThreads) {
    const int64_t* x = reinterpret_cast<const int64_t*>(stack + col0 + c);
    T acc = T(0);
    int64_t prev = 0;
    int rank = 0;  // values below `prev` or equal to it: ranks [0, rank)
    while (rank < hi) {
      int64_t best = 0;
      int cnt = 0;
      for (int i = 0; i < n; ++i) {
        const int64_t b = x[(int64_t)i * stride], k = kFloat ? trim_key(b) : b;
        if (rank > 0 && k <= prev) continue;
        if (cnt == 0 || k < best) {
          best = k;
          cnt = 1;
        } else if (k == best) {
          ++cnt;
        }
      }
      const T v = __builtin_bit_cast(T, kFloat ? trim_key(best) : best);
      const int r1 = rank + cnt < hi ? rank + cnt : hi;
      for (int r = rank > lo ? rank : lo; r < r1; ++r) acc = r == lo ? v : add<T>(acc, v);
      rank += cnt;
      prev = best;
    }
    acc_out[c] = acc;
  }
}

}  // namespace fa
