// fa_transport.hpp — the kernels that move or make bytes and reduce nothing: the plain copy, the
// paced all-gather push, the cache fences and the benchmark's uniform fill.  Included by
// fa_transport.hip only among the product's units (copy_kernel, push_kernel and fill_uniform_kernel
// are no templates and may be defined once per library) and, through fa_device.hpp, by the tools.
#pragma once

#include "fa_numerics.hpp"

namespace fa {

// Plain copy (fa_copy): 16-B non-temporal loads and stores, grid-stride; the last nbytes % 16
// bytes by the first block's lanes.  Pointers 16-byte aligned (checked on the host).
__global__ __launch_bounds__(kThreads) void copy_kernel(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src,
                                                        int64_t nbytes) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const int64_t quads = nbytes >> 4;
  const u4* s = reinterpret_cast<const u4*>(src);
  u4* d = reinterpret_cast<u4*>(dst);
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kThreads)
    __builtin_nontemporal_store(__builtin_nontemporal_load(s + q), d + q);
  const int64_t tail = nbytes - (quads << 4);
  if (blockIdx.x == 0 && threadIdx.x < tail) dst[(quads << 4) + threadIdx.x] = src[(quads << 4) + threadIdx.x];
}

// One-shot all-gather leg (fa_push): each lane loads 16 B of the local stripe once and stores it
// into every destination (the peers' receive buffers over their xGMI links, and the local one);
// the closing system-scope fence makes the peer stores visible once the kernel has completed.
// Paced: every wave drains its stores (vmcnt(0): on gfx9 the counter covers stores) before its
// next round's loads, so at most U x n_dsts KiB per wave is in flight and the grid sets the total.
// Stores queued beyond a link's bandwidth-delay product back up into the data fabric the reduce
// beside them streams through: on one GPU's PCIe stand-in, 8 blocks reach 52 GB/s either way and
// slow the reduce 1.27-1.32x paced, 1.27-2.08x unpaced (2.08 in the same run as the paced 1.27;
// tools/overlap_probe.py paced<U>x<B> / pushhost<B>).
struct PushDsts {
  uint8_t* p[8];
};

// One system-scope cache fence per wave: RELEASE (K = 0) writes the L2 back to HBM, ACQUIRE
// (K = 1) invalidates it, so that a copy engine (which reads and writes HBM behind the L2) and the
// kernels around it see each other's data (fa_cache_fence).  Each XCD has its own L2: the launch
// spreads one wave over every XCD, several times over.
template <int K>
__global__ __launch_bounds__(64) void cache_fence_kernel() {
  if (K == 0)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  else
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
}

__global__ __launch_bounds__(kThreads) void push_kernel(const uint8_t* __restrict__ src, int64_t quads, PushDsts d,
                                                        int n_dsts) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  constexpr int U = 4;  // quads per lane per round: U loads, then U stores to every destination
  const u4* s = reinterpret_cast<const u4*>(src);
  const int64_t G = (int64_t)gridDim.x * kThreads;
  for (int64_t q0 = (int64_t)blockIdx.x * kThreads + threadIdx.x; q0 < quads; q0 += U * G) {
    u4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t q = q0 + u * G;
      v[u] = q < quads ? __builtin_nontemporal_load(s + q) : u4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i >= n_dsts) break;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t q = q0 + u * G;
        if (q < quads) reinterpret_cast<u4*>(d.p[i])[q] = v[u];
      }
    }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // pace: this round's stores done first
  }
  __threadfence_system();
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(kThreads) void fill_uniform_kernel(float* __restrict__ dst,
                                                                int64_t stride, int64_t ncols,
                                                                uint64_t seed, int64_t row0,
                                                                int64_t colg0) {
  const int64_t r = blockIdx.y;
  const uint64_t key_row = (seed * 0xD1B54A32D192ED03ull) ^ ((uint64_t)(row0 + r) << 40);
  float* out = dst + r * stride;
  for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < ncols;
       c += (int64_t)gridDim.x * kThreads) {
    const uint64_t h = splitmix64(key_row ^ (uint64_t)(colg0 + c));
    out[c] = (float)(h >> 40) * 0x1.0p-23f - 1.0f;
  }
}

}  // namespace fa
