// fa_trimwide.hpp — coordinate-wise trimmed sums of 129 .. 1024 clients (fa_trim_sum_wide; DESIGN.md
// section 19): a column's clients spread over several lanes, each lane's run sorted in registers by
// fa_trim.hpp's network, the runs merged by bitonic stages whose wide layers go through LDS.
// Included by fa_trimwide.hip only.
#pragma once

#include <utility>

#include "fa_numerics.hpp"
#include "fa_trim.hpp"

namespace fa {
namespace trimwide {

constexpr int kRun = 128;      // slots a thread holds: trim_sort<128>
constexpr int kThreads = 256;  // one block per CU (launch bounds): 512 VGPRs per lane

// One half-cleaner of a bitonic merge inside the thread: slots (a, a + ST) for every a with bit ST
// clear, ascending, 64 exchanges on compile-time indices.
template <int ST, int... M>
__device__ __forceinline__ void merge_layer(int (&key)[kRun], std::integer_sequence<int, M...>) {
  (trim_exchange<M / ST * 2 * ST + M % ST, M / ST * 2 * ST + M % ST + ST, true>(key), ...);
}

// strides 64 .. 1: what is left of a merge stage once its run is a bitonic sequence (448 exchanges)
template <int ST = kRun / 2>
__device__ __forceinline__ void merge_run(int (&key)[kRun]) {
  merge_layer<ST>(key, std::make_integer_sequence<int, kRun / 2>{});
  if constexpr (ST > 1) merge_run<ST / 2>(key);
}

// One layer at a stride of whole runs.  xch is [slot][thread] (= [slot][run][column]: a thread's
// index is run * C + column), so the 64 lanes of a wave write and read 64 consecutive dwords.  The
// thread leaves its run, and after the barrier reads its partner's (thread `ptid`), slot by slot —
// mirrored (REV: the first layer of a stage, slot i against slot 2^m * 128 - 1 - i) or straight —
// keeping the smaller keys on the low side of the pair and the larger on the high side:
// v_med3_i32 with `bound` = INT_MIN is the minimum, with INT_MAX the maximum, so the side is a lane's
// own.  The second barrier frees the buffer for the next layer.  Every thread of the block comes here.
template <bool REV>
__device__ __forceinline__ void cross_layer(int (&key)[kRun], int* xch, int tid, int ptid, int bound) {
#pragma unroll
  for (int s = 0; s < kRun; ++s) xch[s * kThreads + tid] = key[s];
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kRun; ++s) {
    const int other = xch[(REV ? kRun - 1 - s : s) * kThreads + ptid];
    int kept;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(kept) : "v"(key[s]), "v"(other), "v"(bound));
    key[s] = kept;
  }
  __syncthreads();
}

// Stage M of log2 R: sorted groups of 2^(M-1) runs become sorted groups of 2^M.  The mirrored layer
// pairs run g of a group with run 2^M - 1 - g; the straight layers follow at strides of
// 2^(M-2) .. 1 runs, then the seven strides inside the thread.
template <int M, int K>
__device__ __forceinline__ void merge_straight(int (&key)[kRun], int* xch, int tid, int run, int c) {
  if constexpr (K >= 0) {
    cross_layer<false>(key, xch, tid, tid ^ ((1 << K) * c), run & (1 << K) ? INT32_MAX : INT32_MIN);
    merge_straight<M, K - 1>(key, xch, tid, run, c);
  }
}

template <int R, int M = 1>
__device__ __forceinline__ void merge_stages(int (&key)[kRun], int* xch, int tid, int run, int c) {
  if constexpr ((1 << M) <= R) {
    cross_layer<true>(key, xch, tid, tid ^ (((1 << M) - 1) * c), run & (1 << (M - 1)) ? INT32_MAX : INT32_MIN);
    merge_straight<M, M - 2>(key, xch, tid, run, c);
    merge_run(key);
    merge_stages<R, M + 1>(key, xch, tid, run, c);
  }
}

// fp32 rows, NP / 2 < n <= NP clients, NP in {256, 512, 1024}.  A column's NP slots are R = NP / 128
// runs; thread (run j, column c) = j * C + c of the block holds rows 128 j .. 128 j + 127 of column
// c of the piece, C = 256 / R columns wide (128 B of a row at NP = 1024); the block strides over
// the window's pieces by the grid.  Loads as in trim_kernel_rows: one dword per lane and row through
// a range-checked descriptor whose range is the piece's valid bytes, all of a run's loads issued
// before the first compare, straight into the sort registers, slots of rows >= n holding the key
// 0x7fffffff.  A descriptor is a wave's scalars, so where a wave holds two runs (C = 32) each half
// of its lanes loads under its own.  Then trim_sort<128> per thread, log2 R merge stages
// (merge_stages), and thread (j, c) holds ranks 128 j .. 128 j + 127 of its column.  The kept ranks
// trim .. n - trim - 1 are added in ascending order into one fp32 chain per column, the running sum
// handed from run j to run j + 1 through LDS (relay); the run that holds the last kept rank stores.
// Lanes past a ragged piece's end load zeros, take every barrier, and their stores are dropped by
// the output descriptor's range.  No scratch: every index of key[] is a constant.
template <int NP, bool NT>
__global__ __launch_bounds__(kThreads, 1) void merge_trim_kernel(const float* __restrict__ stack, int64_t stride, int n,
                                                                  int trim, float* __restrict__ acc_out, int64_t col0,
                                                                  int64_t ncols) {
  static_assert(NP == 256 || NP == 512 || NP == 1024, "two to eight runs of 128");
  constexpr int R = NP / kRun, C = kThreads / R;
  constexpr int RW = C >= 64 ? 1 : 64 / C;  // runs per wave
  __shared__ int xch[kRun * kThreads];       // 128 KiB
  __shared__ float relay[C];
  const int64_t pieces = (ncols + C - 1) / C;
  const int64_t row_bytes = stride * 4;
  int tid = (int)threadIdx.x;
  const int col = tid % C, run = tid / C;
  const int voff = col * 4;
  // the run of the wave's first lane: a scalar, and with RW == 1 the whole wave's
  const int run0 = __builtin_amdgcn_readfirstlane(run);
  for (int64_t p = blockIdx.x; p < pieces; p += gridDim.x) {
    // the bounds made opaque per piece, as in trim_kernel_rows
    int nn = n, lo = trim;
    asm volatile("" : "+s"(nn), "+s"(lo));
    const int hi = nn - lo;  // kept ranks [lo, hi)
    const int64_t c0 = p * C;
    const int cols = ncols - c0 < C ? (int)(ncols - c0) : C;
    const uint32_t bytes = (uint32_t)cols * 4u;
    const char* piece = reinterpret_cast<const char*>(stack + col0 + c0);
    int key[kRun];
#pragma unroll
    for (int h = 0; h < RW; ++h) {
      if (RW == 1 || run - run0 == h) {
        const int first = (run0 + h) * kRun;           // the run's first row: a scalar
        const char* pn = piece + first * row_bytes;    // the next row to load
        const int rows = nn - first;                   // real rows of the run (<= 0: all padding)
#pragma unroll
        for (int i = 0; i < kRun; ++i) {
          if (i < rows) {
            key[i] = (int)__builtin_amdgcn_raw_buffer_load_b32(row_rsrc(pn, bytes), voff, 0, NT ? 2 : 0);
            pn += row_bytes;
            asm volatile("" : "+s"(pn));  // one running scalar pointer
            __builtin_amdgcn_sched_barrier(0);
          } else {
            key[i] = 0x7fffffff;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kRun; ++i) key[i] = trim_key(key[i]);
    trim_sort<kRun>(key);
    merge_stages<R>(key, xch, tid, run, C);
    // the sum: run j adds its kept ranks [lo - 128 j, hi - 128 j) of [0, 128) onto what run j - 1
    // left in relay[]; the steps and their barriers are taken by the whole block (lo, hi: scalars)
    const __amdgpu_buffer_rsrc_t ro = col_rsrc<float>(acc_out, c0 / 4, cols);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int jlo = lo - j * kRun, jhi = hi - j * kRun;
      if (jhi > 0 && jlo < kRun) {
        if (run == j) {
          float acc = jlo < 0 ? relay[col] : 0.f;
#pragma unroll
          for (int r = 0; r < kRun; ++r) {
            if (r >= jlo && r < jhi) {
              const float x = __builtin_bit_cast(float, trim_key(key[r]));
              acc = r == jlo ? x : acc + x;
            }
          }
          if (jhi <= kRun)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, acc), ro, voff, 0, kEpiStoreAux);
          else
            relay[col] = acc;
        }
        __syncthreads();
      }
    }
  }
}

}  // namespace trimwide
}  // namespace fa
