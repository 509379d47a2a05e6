// fa_clipfold.hpp — streamed norm-clipped rounds (fa_clip_fold_f32): the
// clipped sum of one chunk of clients, opening the round's sum or continuing the previous chunk's.
// clip_sum_kernel's sibling (fa_clip.hpp): its work split, descriptors, load pipeline and three-way
// rule, through the same __device__ helpers, plus one pointer, acc_in.  Included by fa_clip.hip
// only, after fa_clip.hpp.  The kernel lives in fa::clipfold: the inventories pin the kernels of
// fa, fa::clip and fa::noise.
#pragma once

#include "fa_clip.hpp"

namespace fa {
namespace clipfold {

using clip::XV;

// acc_in == NULL (wave-uniform): clip_sum_kernel, row 0's clipped upload initialises the sums.
// Else the piece's carried sums are loaded through a range-checked descriptor (lanes past the
// piece's end load 0 and their stores are dropped), issued with the centre's loads before the ramp,
// and every row 0..n-1 is added.  acc_out may be acc_in: a lane reads its quads before it writes
// them and no other lane touches them.
template <int V, int D, int W, bool NT>
__global__ __launch_bounds__(64 * W) void clip_fold_kernel(const float* __restrict__ stack, int64_t stride, int n,
                                                           const float* __restrict__ center,
                                                           const float* __restrict__ scale, const float* acc_in,
                                                           float* acc_out, int64_t col0, int64_t ncols) {
  const int64_t nquads = (ncols + 3) / 4;
  const int64_t chunks = (nquads + 63) / 64;
  const int64_t gr = gridDim.x;
  const int64_t k = (chunks + gr * W * V - 1) / (gr * W * V);  // rounds
  const int64_t pc = (chunks + gr * k - 1) / (gr * k);         // chunks per piece (<= W*V)
  const int64_t pieces = (chunks + pc - 1) / pc;
  const bool first = acc_in == nullptr;
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
    if (!first) {
      const __amdgpu_buffer_rsrc_t ra = col_rsrc<const float>(acc_in, qb, cols);
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = buf_load_tquad<float>(ra, (int)threadIdx.x + v * 64 * W);
    }
    auto sweep = [&](int s) {  // s: the first row of the pipeline, 1 behind an opening row 0
      clip::rows_each<V, D, W, NT>(
          tile0, stride * 4, bytes, s, n, [&](int i) { return scale[i] > 0.f; },
          [&] {  // opening chunk: row 0, behind the ramp's loads as in clip_sum_kernel
            if (!first) return;
            const float s0 = scale[0];
            if (s0 > 0.f) {
              const __amdgpu_buffer_rsrc_t r = row_rsrc(tile0, bytes);
#pragma unroll
              for (int v = 0; v < V; ++v) acc[v] = buf_load_quad<NT>(r, (int)threadIdx.x * 16 + v * 64 * W * 16, 0);
            }
            clip::clip_first<V>(acc, g, s0);
          },
          [&](int i, const XV(&x)[V]) { clip::clip_add<V>(acc, g, scale[i], x); });
    };
    // One pipeline with a run-time start row keeps clip_sum_kernel's registers for V >= 2; at
    // V = 1 (D = 16: sixteen ramp conditions on s) it spilled ten scalar registers, so that depth
    // gets one copy of the pipeline per start row, each with a constant s.
    if constexpr (V == 1) {
      if (first) sweep(1); else sweep(0);
    } else {
      sweep(first ? 1 : 0);
    }
    const __amdgpu_buffer_rsrc_t ro = col_rsrc<float>(acc_out, qb, cols);
#pragma unroll
    for (int v = 0; v < V; ++v) buf_store_tquad<float>(ro, (int)threadIdx.x + v * 64 * W, acc[v]);
  }
}

}  // namespace clipfold
}  // namespace fa
