// fa_noise.hpp — the Gaussian noise of a DP-FedAvg round (fa_gauss_add_f32):
// a counter-based generator, so a column's noise is a function of (seed, sequence, absolute column)
// and of nothing else — not of the grid, the window or the device.  Philox4x32-10 (Salmon et al.
// 2011) gives four words per counter q = column / 4; each word becomes a uniform in (0, 1) that is
// exact in fp32, and Box-Muller turns words (0, 1) and (2, 3) into the normals of columns 4q .. 4q+3.
// tests/noise_ref.py restates the whole in float64.  Included by fa_noise.hip only.  The kernel lives
// in fa::noise: the kernel inventory pins the kernels of namespace fa itself.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace fa {
namespace noise {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;  // the round's multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;  // the key's increments
constexpr int kPhiloxRounds = 10;
constexpr int kNoiseThreads = 256;

struct Words {
  uint32_t w[4];
};

// Philox4x32-10: ten rounds of (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the
// key bumped before every round but the first.  Each product is one 32 x 32 -> 64-bit multiply.
__device__ __forceinline__ Words philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                            uint32_t k1) {
#pragma unroll
  for (int r = 0; r < kPhiloxRounds; ++r) {
    if (r) {
      k0 += kPhiloxW0;
      k1 += kPhiloxW1;
    }
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  return Words{{c0, c1, c2, c3}};
}

// ((w >> 9) + 0.5) * 2^-23 in [2^-24, 1 - 2^-24]: 2 * (w >> 9) + 1 is a 24-bit odd integer, so the
// conversion and the power-of-two scale are exact
__device__ __forceinline__ float uniform01(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * 0x1p-24f; }

// Box-Muller on one pair of words: z0 = r cos(2 pi u_b), z1 = r sin(2 pi u_b), r = sqrt(-2 ln u_a),
// on the hardware's transcendentals: v_log_f32 is log2, so -2 ln u = (-2 ln 2) * log2(u); v_sin_f32
// and v_cos_f32 take revolutions, so u_b goes in as it is.  u_a >= 2^-24 is a normal number and
// log2(u_a) <= log2(1 - 2^-24) < 0, so r is finite and positive.  Measured on MI355X against the
// float64 restatement over 2^20 columns: |z - z_ref| <= 6.4e-7, the library's logf / sqrtf /
// sincospif 7.1e-7 and 16% slower.
__device__ __forceinline__ void normal_pair(uint32_t wa, uint32_t wb, float& z0, float& z1) {
  constexpr float kMinus2Ln2 = -1.3862943611198906f;
  const float r = __builtin_amdgcn_sqrtf(kMinus2Ln2 * __builtin_amdgcn_logf(uniform01(wa)));
  const float ub = uniform01(wb);
  z0 = r * __builtin_amdgcn_cosf(ub);
  z1 = r * __builtin_amdgcn_sinf(ub);
}

// fa_gauss_add_f32: acc[c] = fl32(acc[c] + fl32(sigma * z(q0 * 4 + c))) for c in [0, ncols).  One
// 16-B quad per lane and step, grid-stride over the window's quads: a dwordx4 load, one Philox call,
// four normals, a dwordx4 store.  The last quad of a window whose width is no multiple of 4 is
// loaded and stored element by element, so nothing outside acc[0, ncols) is touched.  No LDS, no
// atomics.  (k0, k1): the seed's halves; (s0, s1): the sequence's.
__global__ __launch_bounds__(kNoiseThreads) void gauss_add_kernel(float* __restrict__ acc, int64_t q0, int64_t ncols,
                                                                   float sigma, uint32_t k0, uint32_t k1, uint32_t s0,
                                                                   uint32_t s1) {
  const int64_t whole = ncols / 4, nquads = (ncols + 3) / 4;
  const int64_t step = (int64_t)gridDim.x * kNoiseThreads;
  for (int64_t q = (int64_t)blockIdx.x * kNoiseThreads + threadIdx.x; q < nquads; q += step) {
    const uint64_t ctr = (uint64_t)(q0 + q);
    const Words x = philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), s0, s1, k0, k1);
    float z[4];
    normal_pair(x.w[0], x.w[1], z[0], z[1]);
    normal_pair(x.w[2], x.w[3], z[2], z[3]);
    float* p = acc + q * 4;
    if (q < whole) {
      float4 a = *reinterpret_cast<const float4*>(p);
      a.x = a.x + sigma * z[0];
      a.y = a.y + sigma * z[1];
      a.z = a.z + sigma * z[2];
      a.w = a.w + sigma * z[3];
      *reinterpret_cast<float4*>(p) = a;
    } else {
      const int left = (int)(ncols - q * 4);  // 1 .. 3
#pragma unroll
      for (int e = 0; e < 3; ++e)
        if (e < left) p[e] = p[e] + sigma * z[e];
    }
  }
}

}  // namespace noise
}  // namespace fa
