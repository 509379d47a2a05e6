// fa_gram.hpp — the client Gram matrix (fa_gram_f32): gram_kernel_tile, the engine's one
// contraction and its one MFMA kernel, and gram_finish_kernel, which sums the blocks' partial
// tiles in float64.  Included by fa_gram.hip and, through fa_device.hpp, by the tuning tools.
#pragma once

#include "fa_geometry.hpp"
#include "fa_numerics.hpp"

namespace fa {

// ---------------------------------------------------------------------------------------------
// G[i][j] = sum_k y_i[k] * y_j[k], y_i[k] = fl32(x_i[k] - c[k]), on
// v_mfma_f32_32x32x2_f32: exact fp32 products and sums, a k-ordered fmaf chain per entry.
// ---------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// How an instantiation spreads its work over the block's 4 waves.  G is symmetric, so only the
// T (T + 1) / 2 upper 32 x 32 tiles (a <= b) are computed.  TS groups of waves split the tiles,
// the KS waves of a group split each LDS chunk's columns; KS x TS = 4 and every wave has TPW tiles:
//   NP  32: 1 tile,   KS 4, TS 1, TPW 1      NP  96: 6 tiles,  KS 2, TS 2, TPW 3
//   NP  64: 3 tiles,  KS 4, TS 1, TPW 3      NP 128: 10 tiles, KS 2, TS 2, TPW 5
// so each SIMD issues the same number of MFMAs, on TPW independent accumulators.
template <int NP>
struct GramShape {
  static_assert(NP % kGramTile == 0 && NP >= kGramTile && NP <= kGramMaxClients, "whole 32-row tiles");
  static constexpr int T = NP / kGramTile;
  static constexpr int TILES = T * (T + 1) / 2;
  static constexpr int KS = TILES <= 3 ? 4 : 2;
  static constexpr int TS = 4 / KS;
  static constexpr int TPW = TILES / TS;
  static constexpr int KC = gram_kc(NP);
  static constexpr int PITCH = KC + 4;               // floats; 4 mod 64: conflict-free b128 reads
  static constexpr int E = KC >= 256 ? 4 : 2;        // floats per lane and load (16 B; Kc 128: 8 B)
  static constexpr int LPR = KC / (64 * E);          // wave loads per row and chunk
  static constexpr int RPW = NP / 4;                 // rows per wave: wave, wave + 4, ...
  static constexpr int KW = KC / KS;                 // a wave's columns of every chunk
  typedef float vec __attribute__((ext_vector_type(E)));  // what one lane holds of one load
  static_assert(TILES % TS == 0 && KW % 8 == 0 && kGramLc % KC == 0, "even split");
  static_assert(4 * TPW * 16 * 64 <= 2 * NP * PITCH, "the end-of-block exchange fits the tiles' LDS");
};

// 16 or 8 bytes per lane through a descriptor, as one instruction
template <class V, int AUX>
__device__ __forceinline__ V gram_buf_load(__amdgpu_buffer_rsrc_t r, int voff) {
  if constexpr (sizeof(V) == 16)
    return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, AUX));
  else
    return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(r, voff, 0, AUX));
}

// One chunk of one wave's rows into registers: row r = wave + 4 i through its own range-checked
// descriptor (row_rsrc) whose range is the chunk's valid bytes, so a ragged end loads 0 and no
// address past the window is ever formed into a fetch; one row per wave instruction, 1 KiB (Kc
// 128: 512 B) contiguous, non-temporal.  Rows >= n are not loaded (wave-uniform).
template <int NP, bool NT>
__device__ __forceinline__ void gram_load(typename GramShape<NP>::vec (&st)[GramShape<NP>::RPW][GramShape<NP>::LPR],
                                          const char* p, int64_t row_bytes, int wave, int n, uint32_t bytes,
                                          int lane) {
  using S = GramShape<NP>;
  // the bound made opaque per chunk: as a loop invariant every one of the RPW wave-uniform
  // conditions is computed ahead of the chunk loop and kept in a scalar register pair
  asm volatile("" : "+s"(n));
#pragma unroll
  for (int i = 0; i < S::RPW; ++i) {
    if (wave + 4 * i < n) {
      const __amdgpu_buffer_rsrc_t r = row_rsrc(p, bytes);
#pragma unroll
      for (int j = 0; j < S::LPR; ++j) {
        const int voff = (lane + 64 * j) * S::E * 4;
        st[i][j] = gram_buf_load<typename S::vec, NT ? 2 : 0>(r, voff);
      }
    }
    p += 4 * row_bytes;
    asm volatile("" : "+s"(p));  // one running scalar pointer, as in trim_kernel_rows
    // the loads stay in row order, each descriptor's four scalars built next to its load
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The staged rows into one LDS tile, minus the centre (one fp32 subtract per element)
template <int NP, bool CEN>
__device__ __forceinline__ void gram_stage(float* __restrict__ tile,
                                           const typename GramShape<NP>::vec (&st)[GramShape<NP>::RPW][GramShape<NP>::LPR],
                                           const typename GramShape<NP>::vec (&cs)[GramShape<NP>::LPR], int wave, int n,
                                           int lane) {
  using S = GramShape<NP>;
  asm volatile("" : "+s"(n));  // as in gram_load
#pragma unroll
  for (int i = 0; i < S::RPW; ++i) {
    if (wave + 4 * i < n) {
#pragma unroll
      for (int j = 0; j < S::LPR; ++j) {
        *reinterpret_cast<typename S::vec*>(tile + (wave + 4 * i) * S::PITCH + (lane + 64 * j) * S::E) =
            CEN ? st[i][j] - cs[j] : st[i][j];
      }
    }
  }
}

// fp32 rows, n <= NP clients, 256 threads.  The block owns the chunks [cb, ce) of Kc columns of
// the window (plan_gram_window).  Per chunk the 4 waves load the n rows (gram_load) into registers
// while the previous chunk is multiplied, then write them, centred, into the other of two LDS tiles
// [NP][Kc + 4]; rows n .. NP-1 of both tiles are zeroed once and never written again.  Both MFMA
// operands come from that tile: for the tile (a, b) lane l reads 16 B of row 32a + (l & 31) and of
// row 32b + (l & 31) at column 8g + 4 (l >> 5) of the wave's column slice and issues 4 MFMAs,
// element s of both reads being step s — step s multiplies columns 8g + s (lanes 0-31, k = 0) and
// 8g + 4 + s (lanes 32-63, k = 1); the same columns in both operands, in an order fixed by the
// plan.  After kGramLc columns of the window the inner accumulators are added into the outer fp32
// tile and cleared.  At the end the KS waves' outer tiles are added in wave order through LDS and
// the block stores its upper tiles as partial number blockIdx.x: [NP][NP] floats, row from the A
// operand (C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  No atomics.
// Padded rows are zero, so whatever 0 x inf makes lands in padded rows and columns of the partial,
// which gram_finish_kernel never reads.
template <int NP, bool CEN, bool NT>
__global__ __launch_bounds__(256) void gram_kernel_tile(const float* __restrict__ stack, int64_t stride, int n,
                                                        const float* __restrict__ center, int64_t col0,
                                                        int64_t ncols, int64_t chunks, float* __restrict__ partials) {
  using S = GramShape<NP>;
  __shared__ __attribute__((aligned(16))) float lds[2 * NP * S::PITCH];
  const int tid = (int)threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ks = wave % S::KS, ts = wave / S::KS;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  for (int i = tid; i < 2 * NP * S::PITCH / 4; i += 256) reinterpret_cast<f32x4*>(lds)[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the wave's tiles: number ts * TPW + t of (0,0), (0,1), ..., (0,T-1), (1,1), ...
  int ta[S::TPW], tb[S::TPW], aoff[S::TPW], boff[S::TPW];
#pragma unroll
  for (int t = 0; t < S::TPW; ++t) {
    int a = 0, rem = ts * S::TPW + t;
    while (rem >= S::T - a) {
      rem -= S::T - a;
      ++a;
    }
    ta[t] = a;
    tb[t] = a + rem;
    aoff[t] = (32 * ta[t] + (lane & 31)) * S::PITCH + ks * S::KW + 4 * half;
    boff[t] = (32 * tb[t] + (lane & 31)) * S::PITCH + ks * S::KW + 4 * half;
  }
  f32x16 inner[S::TPW], outer[S::TPW];
#pragma unroll
  for (int t = 0; t < S::TPW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) inner[t][r] = outer[t][r] = 0.f;

  const int64_t cb = (int64_t)blockIdx.x * chunks / gridDim.x, ce = ((int64_t)blockIdx.x + 1) * chunks / gridDim.x;
  const int64_t row_bytes = stride * 4;
  typename S::vec st[S::RPW][S::LPR], cs[S::LPR];
  auto fetch = [&](int64_t c) {
    const int64_t c0 = c * S::KC;
    const uint32_t bytes = (uint32_t)(ncols - c0 < S::KC ? ncols - c0 : S::KC) * 4u;
    gram_load<NP, NT>(st, reinterpret_cast<const char*>(stack + col0 + c0) + wave * row_bytes, row_bytes, wave, n,
                      bytes, lane);
    if constexpr (CEN) {
      const __amdgpu_buffer_rsrc_t r = row_rsrc(center + col0 + c0, bytes);
#pragma unroll
      for (int j = 0; j < S::LPR; ++j) {
        const int voff = (lane + 64 * j) * S::E * 4;
        cs[j] = gram_buf_load<typename S::vec, 0>(r, voff);
      }
    }
  };
  __syncthreads();  // the zeros are in place
  if (cb < ce) {
    fetch(cb);
    gram_stage<NP, CEN>(lds, st, cs, wave, n, lane);
  }
  __syncthreads();
  int run = 0;  // columns of the window in the inner chain
  for (int64_t c = cb; c < ce; ++c) {
    const float* cur = lds + ((c - cb) & 1) * (NP * S::PITCH);
    float* nxt = lds + (((c - cb) & 1) ^ 1) * (NP * S::PITCH);
    const bool more = c + 1 < ce;
    if (more) fetch(c + 1);
#pragma unroll
    for (int g = 0; g < S::KW / 8; ++g) {
#pragma unroll
      for (int t = 0; t < S::TPW; ++t) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(cur + aoff[t] + 8 * g);
        const f32x4 b = *reinterpret_cast<const f32x4*>(cur + boff[t] + 8 * g);
#pragma unroll
        for (int s = 0; s < 4; ++s) inner[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], inner[t], 0, 0, 0);
      }
    }
    run += S::KC;
    if (run >= kGramLc || !more) {
#pragma unroll
      for (int t = 0; t < S::TPW; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          outer[t][r] += inner[t][r];
          inner[t][r] = 0.f;
        }
      }
      run = 0;
    }
    if (more) gram_stage<NP, CEN>(nxt, st, cs, wave, n, lane);
    // one barrier per chunk: `nxt` was last read before the previous barrier, `cur` is next
    // written after this one
    __syncthreads();
  }
  // the KS column slices of every tile, added in wave order by the slice-0 wave
  if (ks > 0) {
#pragma unroll
    for (int t = 0; t < S::TPW; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) lds[((wave * S::TPW + t) * 16 + r) * 64 + lane] = outer[t][r];
  }
  __syncthreads();
  if (ks == 0) {
    float* out = partials + (int64_t)blockIdx.x * (NP * NP);
#pragma unroll
    for (int t = 0; t < S::TPW; ++t) {
#pragma unroll
      for (int k = 1; k < S::KS; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) outer[t][r] += lds[(((wave + k) * S::TPW + t) * 16 + r) * 64 + lane];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * ta[t] + (r & 3) + 8 * (r >> 2) + 4 * half, col = 32 * tb[t] + (lane & 31);
        out[row * NP + col] = outer[t][r];
      }
    }
  }
}

// G[i][j] (float64, [n][n]) = the blocks' partials of the entry, converted and added in block
// order; the entry is read at (min(i, j), max(i, j)), the upper triangle the tile kernel wrote,
// so G[i][j] and G[j][i] are the same bits.
__global__ __launch_bounds__(kThreads) void gram_finish_kernel(const float* __restrict__ partials, int64_t grid,
                                                               int np, int n, double* __restrict__ gram_out) {
  const int idx = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (idx >= n * n) return;
  const int i = idx / n, j = idx % n, lo = i < j ? i : j, hi = i < j ? j : i;
  const float* p = partials + lo * np + hi;
  double s = 0.0;
  for (int64_t b = 0; b < grid; ++b) s += (double)p[b * np * np];
  gram_out[idx] = s;
}

}  // namespace fa
