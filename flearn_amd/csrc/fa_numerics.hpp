// fa_numerics.hpp — the numerics every kernel family shares: quad loads and stores, the
// accumulation policies, the fused epilogue (Epi, update, epi_compute, finish_quad, finish_piece),
// the buffer-descriptor helpers and the rolling row pipeline (rows_sweep).  Header-only templates in
// namespace fa; included by every family header (fa_stack, fa_segrows, fa_half, fa_fold, fa_trim,
// fa_transport) and by fa_host.hpp.
//
// Hot path: Strategy.server_ensemble (flearn/common/strategy/strategy.py:102-130), i.e. for
// every element p of the flattened model bucket
//     acc = a0*x[0][p];  acc += a_n*x[n][p]  (n = 1..N-1, in list order);  w = acc / sum(a)
// optionally followed by the AVGM / FedOPT update (avgm.py:19-36, opt.py:23-65).
//
// Mapping (HBM-bound streaming reduce, 0.5 flop/B, no MFMA):
//   * a TILE is kThreads*V quads (4 contiguous fp32 = one 16-B global_load_dwordx4) of every
//     client row; thread t owns quads t, t+kThreads, ... so each wave instruction reads 1 KiB
//     contiguous of one row;
//   * the client loop walks the rows in list order (the bit-exact sequential fp32 sum numpy
//     does) unrolled U deep: U*V independent 16-B loads in flight per thread hide HBM latency
//     behind a running sum that depends only on already-arrived data;
//   * every client value is read exactly once per launch (NT: non-temporal loads);
//   * the epilogue (divide, optional momentum/adaptive update, f32/f64 stores) is fused: the only
//     HBM traffic is N*P*4 bytes of client reads plus O(P) output/state bytes.
// Compile with -ffp-contract=off: a fused a*x+acc changes fp32 rounding and breaks bit-parity.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flearn_amd.h"

namespace fa {

constexpr int kThreads = 256;

template <typename T>
struct vec4 {
  typedef T type __attribute__((ext_vector_type(4)));
};

template <typename T, bool NT>
__device__ __forceinline__ typename vec4<T>::type load_quad(const T* p) {
  if constexpr (NT)
    return __builtin_nontemporal_load(reinterpret_cast<const typename vec4<T>::type*>(p));
  else
    return *reinterpret_cast<const typename vec4<T>::type*>(p);
}

template <typename T>
__device__ __forceinline__ typename vec4<T>::type load_quad_guarded(const T* p, int valid) {
  typename vec4<T>::type r = {T(0), T(0), T(0), T(0)};
  if (valid > 0) r[0] = p[0];
  if (valid > 1) r[1] = p[1];
  if (valid > 2) r[2] = p[2];
  if (valid > 3) r[3] = p[3];
  return r;
}

template <typename T>
__device__ __forceinline__ void store_quad(T* p, typename vec4<T>::type v, int valid) {
  if (valid == 4) {
    *reinterpret_cast<typename vec4<T>::type*>(p) = v;
  } else {
    if (valid > 0) p[0] = v[0];
    if (valid > 1) p[1] = v[1];
    if (valid > 2) p[2] = v[2];
  }
}

// ---------------------------------------------------------------------------------------------
// Accumulation policies: product dtype = sum dtype, chosen by numpy's promotion of the weight
// type against the tensor dtype (resolved on the host: flearn_amd/semantics.py).
// ---------------------------------------------------------------------------------------------
struct AccF32 {  // fp32 tensors x Python-float/int or np.float32 weights
  typedef float x_t;
  typedef float w_t;
  typedef float acc_t;
  static __device__ __forceinline__ float mul(float w, float x) { return w * x; }
};
struct AccF32W64 {  // fp32 tensors x np.float64/np.int64 weights: promoted to f64
  typedef float x_t;
  typedef double w_t;
  typedef double acc_t;
  static __device__ __forceinline__ double mul(double w, float x) { return w * (double)x; }
};
struct AccF64 {  // f64 tensors (and int64 buffers cast to f64) x f64 weights
  typedef double x_t;
  typedef double w_t;
  typedef double acc_t;
  static __device__ __forceinline__ double mul(double w, double x) { return w * x; }
};
struct AccI64 {  // int64 buffers x Python-int weights: int64 arithmetic, wraps like numpy
  typedef int64_t x_t;
  typedef int64_t w_t;
  typedef int64_t acc_t;
  static __device__ __forceinline__ int64_t mul(int64_t w, int64_t x) {
    return (int64_t)((uint64_t)w * (uint64_t)x);
  }
};

template <typename A>
__device__ __forceinline__ A add(A a, A b) {
  return a + b;
}
template <>
__device__ __forceinline__ int64_t add<int64_t>(int64_t a, int64_t b) {
  return (int64_t)((uint64_t)a + (uint64_t)b);
}

// ---------------------------------------------------------------------------------------------
// Epilogue: mean in precision T (double for DIV64/W64, float for DIV32) and the optional
// server-side optimizer update, all in T with the reference's operation order.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct Epi {
  T denom;
  const float* prev;
  T* v;
  T beta, eta, tau, beta2, c;  // c = 1 - beta2 (evaluated in double on the host, as Python does);
                               // FA_OP_DYN: c = alpha / N (a Python float, cast to T by numpy)
  float* h;                    // FA_OP_DYN: fp32 h; v holds theta
  T n;                         // FA_OP_DYN: len(w_local_lst)
  float alpha32;               // FA_OP_DYN: fl32(alpha) — alpha * (fp32 h) stays fp32
  float* out32;
  double* out64;
  unsigned long long* trace;  // tuning only (reduce_kernel_rowmajor<..., TR = true>): phase timestamps
  T* v_out;                   // where the updated v goes; NULL: back into v (in place)
  double rdenom;              // 1.0 / denom, rounded once on the host (quot)
  int rq;                     // quot's reciprocal form is exact for this denom (fa::recip_quot_exact)
};

// Which quotient a launch takes is wave-uniform (e.rq), so the callers branch once per piece and
// pass it down as RQ.  The reciprocal form exists for fp32 sums divided in double only.
template <typename T, typename A>
constexpr bool kHasRecipQuot = sizeof(T) == 8 && sizeof(A) == 4;

// sum / denom in T.  RQ: the same double without the divide (13 f64 instructions on gfx950, a
// v_rcp_f64 among them): two fma steps on x * (1/denom), bit-identical to IEEE x / denom for every
// fp32 x when denom's significand has at most 27 bits and 2^-100 <= |denom| <= 2^100 — the proof is
// in DESIGN.md §2, the rule in fa::recip_quot_exact (fa_geometry.hpp).  Zeros, infinities and NaN
// come out of the first product as the divide would give them (the remainder step would turn an
// infinity into NaN).
template <typename T, typename A, int RQ>
__device__ __forceinline__ T quot(const Epi<T>& e, A a) {
  if constexpr (RQ != 0 && kHasRecipQuot<T, A>) {
    const double x = (double)a, d = (double)e.denom;
    const double q0 = x * e.rdenom;
#ifdef FA_TUNE_QUOT_MUL  // tools/tune_reduce.hip's timing probe (rq = 2): the bare product, WRONG results
    if constexpr (RQ == 2) return q0;
#endif
    const double q = __builtin_fma(__builtin_fma(-q0, d, x), e.rdenom, q0);
    return (q0 == 0.0 || !__builtin_isfinite(q0)) ? q0 : q;
  } else {
    return (T)a / e.denom;
  }
}

template <typename T>
__device__ __forceinline__ T sign_of(T x) {
  // np.sign: -1, 0, +1, NaN for NaN
  return x > T(0) ? T(1) : (x < T(0) ? T(-1) : (x == T(0) ? T(0) : x));
}

template <typename T, int OP>
__device__ __forceinline__ T update(const Epi<T>& e, T g, T l, T& vv) {
  if constexpr (OP == FA_OP_MEAN) {
    return g;
  } else {
    const T d = g - l;  // delta_w = w_glob - w_local            avgm.py:22-25 / opt.py:30-33
    if constexpr (OP == FA_OP_AVGM) {
      vv = d + e.beta * vv;  // v_t = delta + beta*v_t           avgm.py:31-32
      return l + vv;         // w_local + v_t                    avgm.py:34-35
    } else {
      const T m = d * d;  // np.multiply(delta, delta)            opt.py:52
      if constexpr (OP == FA_OP_ADAGRAD) {
        vv = vv + m;  //                                          opt.py:53-54
      } else if constexpr (OP == FA_OP_YOGI) {
        vv = vv - (e.c * m) * sign_of<T>(vv - m);  //             opt.py:55-58
      } else {
        vv = e.beta2 * vv + e.c * m;  //                          opt.py:59-60
      }
      return l + (e.eta * d) / (sqrt(vv) + e.tau);  //          opt.py:62-63
    }
  }
}

// divide and update one quad: a = its sums, l / vv = its loaded state in, updated state out (l:
// FedDyn's h), w = the new global values
template <typename T, int OP, typename A, int RQ = 0>
__device__ __forceinline__ void epi_compute(const Epi<T>& e, const typename vec4<A>::type a,
                                            typename vec4<float>::type& l, typename vec4<T>::type& vv,
                                            typename vec4<T>::type& w) {
  if constexpr (OP == FA_OP_DYN) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const T g = quot<T, A, RQ>(e, a[j]);
      const T d = g * e.n - vv[j];                  // delta_theta = w_glob*N - theta   dyn.py:20-21
      const float hn = (float)((T)l[j] - e.c * d);  // h -= alpha/N * delta (fp32 h)    dyn.py:26
      const float ah = e.alpha32 * hn;              // alpha * h stays fp32              dyn.py:33
      w[j] = g - (T)ah;                             // w_glob - alpha*h                  dyn.py:33
      l[j] = hn;
      vv[j] = w[j];                                 // theta = w_glob                    dyn.py:34
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const T g = quot<T, A, RQ>(e, a[j]);  // np.divide(w_glob, np.sum(a))  strategy.py:127-129
      T vj = vv[j];
      w[j] = update<T, OP>(e, g, (T)l[j], vj);
      vv[j] = vj;
    }
  }
}

// One quad through guarded generic loads and stores (the 8-byte kinds, the ragged window end, the
// standalone update): the arithmetic is epi_compute's.
template <typename T, int OP, typename A>
__device__ __forceinline__ void finish_quad(const Epi<T>& e, int64_t c, int valid,
                                            typename vec4<A>::type acc) {
  typename vec4<T>::type w;
  typename vec4<T>::type vv = {T(0), T(0), T(0), T(0)};
  typename vec4<float>::type l = {0.f, 0.f, 0.f, 0.f};
  if constexpr (OP != FA_OP_MEAN) {
    const float* ls = OP == FA_OP_DYN ? e.h : e.prev;  // the fp32 per-column operand
    if (valid == 4) {
      l = *reinterpret_cast<const typename vec4<float>::type*>(ls + c);
      vv = *reinterpret_cast<const typename vec4<T>::type*>(e.v + c);
    } else {
      l = load_quad_guarded(ls + c, valid);
      vv = load_quad_guarded(e.v + c, valid);
    }
  }
  epi_compute<T, OP, A>(e, acc, l, vv, w);
  if constexpr (OP == FA_OP_DYN) store_quad<float>(e.h + c, l, valid);
  if constexpr (OP != FA_OP_MEAN) store_quad<T>((e.v_out ? e.v_out : e.v) + c, vv, valid);
  if (e.out32) {
    typename vec4<float>::type o = {(float)w[0], (float)w[1], (float)w[2], (float)w[3]};
    store_quad<float>(e.out32 + c, o, valid);
  }
  if (e.out64) {
    typename vec4<double>::type o = {(double)w[0], (double)w[1], (double)w[2], (double)w[3]};
    store_quad<double>(e.out64 + c, o, valid);
  }
}

// Buffer descriptors (4-byte elements).  Per client row a block builds a buffer resource whose
// base is the row's first quad of its piece and whose num_records is the piece's valid byte
// count; lane offsets (VGPR) are the same for every row.  Accesses past the valid range are
// dropped by the hardware range check (they return 0, generate no memory request and need no
// branch), so a partial piece runs the same instruction stream as a full one.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}

template <bool NT>
__device__ __forceinline__ vec4<float>::type buf_load_quad(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, NT ? 2 : 0);
  return __builtin_bit_cast(vec4<float>::type, u);
}

// ---------------------------------------------------------------------------------------------
// Piece epilogue through buffer descriptors.  A lane's slots of a piece are quads
// q = threadIdx.x + v*STEP; the state operands (prev or h, v) are loaded for B slots at once,
// UNCONDITIONALLY, through descriptors whose range is the piece's valid columns — the raw-buffer
// range check is per dword on gfx950 (tools/probe_oob.py), so lanes past the end read 0 and their
// stores are dropped, with no branch — then the B results are computed and stored.  With one
// guarded generic load per quad (finish_quad) the compiler waited for each quad's loads, and for
// the previous quad's stores, before the next: 24 serial HBM round trips at every piece-group end
// of the fused FedAVGM kernel.
// ---------------------------------------------------------------------------------------------
// Cache policy bits of the epilogue's state loads and result / state stores (2 = non-temporal).
// Non-temporal stores: +1.6% on 100 x 25.6 M mean, +1.2% AVGM, +-0.1% Adagrad 100 x 86.6 M (5
// interleaved passes each, tools/gpu_epi_aux2.sh, profiles/r02/tune_epiaux/); non-temporal state
// loads were mixed (-1..-5% Adagrad) and stay cached.
constexpr int kEpiLoadAux = 0;
constexpr int kEpiStoreAux = 2;
// 8-byte elements (v_t / theta state in f64, the f64 result) are stored as two 16-B halves per
// quad, each instruction covering every other 16 B of a wave's 2 KiB: partial 128-B lines.
constexpr int kEpiStore64Aux = kEpiStoreAux;
template <typename T>
__device__ __forceinline__ typename vec4<T>::type buf_load_tquad(__amdgpu_buffer_rsrc_t r, int q) {
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(typename vec4<T>::type, __builtin_amdgcn_raw_buffer_load_b128(r, q * 16, 0, kEpiLoadAux));
  } else {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2 lo = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, q * 32, 0, kEpiLoadAux));
    const d2 hi = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, q * 32 + 16, 0, kEpiLoadAux));
    return typename vec4<T>::type{lo[0], lo[1], hi[0], hi[1]};
  }
}

// XL (whole-line f64 stores): the wave's 64 consecutive f64 quads (2 KiB) are regrouped through
// LDS so that each of the two store instructions writes 1 KiB contiguous (eight whole 128-B
// lines) instead of every other 16 B of the 2 KiB (DESIGN.md §4 finding 22).  Callers run it
// wave-convergent with q = (the wave's first quad) + lane (finish_piece's slots).  The product
// enables it where it does not make the kernel spill (reduce_kernel_rowmajor's XL,
// reduce_kernel_segrows_rm's XLS).
template <typename T, bool XL = false>
__device__ __forceinline__ void buf_store_tquad(__amdgpu_buffer_rsrc_t r, int q, typename vec4<T>::type v) {
  if constexpr (sizeof(T) == 4) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, q * 16, 0, kEpiStoreAux);
  } else if constexpr (XL) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    __shared__ d2 xch[8][128];  // 2 KiB per wave, up to 8 waves per block
    // the thread index made opaque HERE: otherwise the lane-dependent LDS and store addresses
    // are hoisted out of the group sweep and held in VGPRs through it (KG = 4: the sweep is at
    // 256 + 256 registers already, and those few more spilled it to scratch)
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    d2* s = xch[tid >> 6];
    s[2 * lane] = d2{v[0], v[1]};
    s[2 * lane + 1] = d2{v[2], v[3]};
    // lane l reads what lanes l/2 and 32 + l/2 wrote: a cross-lane dependency the compiler does
    // not see, so pin the order (one wave's LDS operations complete in order)
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_wave_barrier();
    const d2 a = s[lane], b = s[64 + lane];
    const int base = (q - lane) * 32;  // the wave's first byte
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, a), r, base + lane * 16, 0, kEpiStore64Aux);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, b), r, base + 1024 + lane * 16, 0,
                                           kEpiStore64Aux);
    __builtin_amdgcn_wave_barrier();  // the next slot's writes come after these reads
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
  } else {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo), r, q * 32, 0, kEpiStore64Aux);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi), r, q * 32 + 16, 0, kEpiStore64Aux);
  }
}

template <typename E>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t col_rsrc(E* base, int64_t qbase, int cols) {
  // a null array (no out32 / out64) gets an empty range: every access is dropped.  Scalar
  // arithmetic only (a select between two descriptors is lowered to VGPRs, and every access
  // through a VGPR descriptor becomes a readfirstlane loop)
  // through readfirstlane: the Epi fields may have been reloaded from the private copy the kernel
  // makes for the noinline ragged path, and the compiler then cannot prove them wave-uniform
  const uint64_t a = (uint64_t)(uintptr_t)base + (uint64_t)(qbase * 4 * (int64_t)sizeof(E));
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane(base ? cols * (int)sizeof(E) : 0);
  return row_rsrc(reinterpret_cast<const void*>((uintptr_t)(((uint64_t)hi << 32) | lo)), n);
}

// The four descriptors of one piece's epilogue (state operands, results); a null array or, for
// the plain mean, the state gets an empty range.
template <typename T, int OP>
struct EpiRsrc {
  __amdgpu_buffer_rsrc_t rl, rv, rvo, r32, r64;
  __device__ __forceinline__ EpiRsrc(const Epi<T>& e, int64_t qbase, int cols)
      : rl(col_rsrc<const float>(OP == FA_OP_DYN ? e.h : e.prev, qbase, OP == FA_OP_MEAN ? 0 : cols)),
        rv(col_rsrc<T>(e.v, qbase, OP == FA_OP_MEAN ? 0 : cols)),
        rvo(col_rsrc<T>(e.v_out ? e.v_out : e.v, qbase, OP == FA_OP_MEAN ? 0 : cols)),
        r32(col_rsrc<float>(e.out32, qbase, cols)),
        r64(col_rsrc<double>(e.out64, qbase, cols)) {}
};

// state operands of quad q (zeros for the plain mean, which has none)
template <typename T, int OP>
__device__ __forceinline__ void epi_load(const EpiRsrc<T, OP>& r, int q, typename vec4<float>::type& l,
                                         typename vec4<T>::type& vv) {
  if constexpr (OP != FA_OP_MEAN) {
    l = buf_load_tquad<float>(r.rl, q);
    vv = buf_load_tquad<T>(r.rv, q);
  } else {
    l = typename vec4<float>::type{0.f, 0.f, 0.f, 0.f};
    vv = typename vec4<T>::type{T(0), T(0), T(0), T(0)};
  }
}

// store quad q's updated state and results.  GUARD = false: the result stores are issued
// unconditionally (a null out32 / out64 has an empty descriptor range, so they are dropped) and
// the quad is one basic block.
template <typename T, int OP, bool GUARD = true, bool XL = false>
__device__ __forceinline__ void epi_store(const Epi<T>& e, const EpiRsrc<T, OP>& r, int q,
                                          const typename vec4<float>::type l, const typename vec4<T>::type vv,
                                          const typename vec4<T>::type w) {
  if constexpr (OP == FA_OP_DYN) buf_store_tquad<float>(r.rl, q, l);
  if constexpr (OP != FA_OP_MEAN) buf_store_tquad<T, XL>(r.rvo, q, vv);
  if (!GUARD || e.out32) buf_store_tquad<float>(r.r32, q, typename vec4<float>::type{(float)w[0], (float)w[1], (float)w[2], (float)w[3]});
  if (!GUARD || e.out64) buf_store_tquad<double, XL>(r.r64, q, typename vec4<double>::type{(double)w[0], (double)w[1], (double)w[2], (double)w[3]});
}

template <typename T, int OP, typename A, bool GUARD = true, bool XL = false, int RQ = 0>
__device__ __forceinline__ void epi_quad(const Epi<T>& e, const EpiRsrc<T, OP>& r, int q,
                                         const typename vec4<A>::type a, typename vec4<float>::type l,
                                         typename vec4<T>::type vv) {
  typename vec4<T>::type w;
  epi_compute<T, OP, A, RQ>(e, a, l, vv, w);
  epi_store<T, OP, GUARD, XL>(e, r, q, l, vv, w);
}

template <typename T, int OP, typename A, int V, int STEP, int B, bool XL, int RQ>
__device__ __forceinline__ void finish_piece_rq(const Epi<T>& e, const EpiRsrc<T, OP>& r,
                                                const typename vec4<A>::type (&acc)[V]) {
#pragma unroll
  for (int b0 = 0; b0 < V; b0 += B) {
    typename vec4<float>::type l[B];
    typename vec4<T>::type vv[B];
#pragma unroll
    for (int b = 0; b < B; ++b) epi_load<T, OP>(r, (int)threadIdx.x + (b0 + b) * STEP, l[b], vv[b]);
#pragma unroll
    for (int b = 0; b < B; ++b)
      epi_quad<T, OP, A, true, XL, RQ>(e, r, (int)threadIdx.x + (b0 + b) * STEP, acc[b0 + b], l[b], vv[b]);
  }
}

template <typename T, int OP, typename A, int V, int STEP, int B, bool XL = false>
__device__ __forceinline__ void finish_piece(const Epi<T>& e, int64_t qbase, int cols,
                                             const typename vec4<A>::type (&acc)[V]) {
  static_assert(V % B == 0, "batch must divide the slots");
  if (cols <= 0) return;
  const EpiRsrc<T, OP> r(e, qbase, cols);
  // (the plain mean only: a second copy of a fused epilogue costs the row-major kernels, which run
  // at the register limit, spills to scratch, and the divide is a small part of those chains)
  if constexpr (OP == FA_OP_MEAN && kHasRecipQuot<T, A>) {
    if (e.rq == 1) return finish_piece_rq<T, OP, A, V, STEP, B, XL, 1>(e, r, acc);
#ifdef FA_TUNE_QUOT_MUL
    if (e.rq == 2) return finish_piece_rq<T, OP, A, V, STEP, B, XL, 2>(e, r, acc);
#endif
  }
  finish_piece_rq<T, OP, A, V, STEP, B, XL, 0>(e, r, acc);
}

// acc + w*x on whole quads, written as <4 x T> IR operations: per-element scalar code gets packed
// by the SLP vectorizer, which re-places the packed products after the pipeline's scheduling
// barriers.  Elementwise identical to P::mul / add (no contraction under -ffp-contract=off).
template <class P>
__device__ __forceinline__ typename vec4<typename P::acc_t>::type quad_axpy(
    typename vec4<typename P::acc_t>::type acc, typename P::w_t w, typename vec4<float>::type x) {
  typedef typename vec4<typename P::acc_t>::type AV;
  if constexpr (sizeof(typename P::acc_t) == 4)
    return acc + w * x;
  else
    return acc + (AV)(typename P::acc_t)w * __builtin_convertvector(x, AV);
}
template <class P>
__device__ __forceinline__ typename vec4<typename P::acc_t>::type quad_mul(
    typename P::w_t w, typename vec4<float>::type x) {
  typedef typename vec4<typename P::acc_t>::type AV;
  if constexpr (sizeof(typename P::acc_t) == 4)
    return w * x;
  else
    return (AV)(typename P::acc_t)w * __builtin_convertvector(x, AV);
}

// Row addressing of the pipeline: a contiguous client stack (row i at tile0 + i*row_bytes), or a
// table of per-client device pointers (row i at ptr[i] + off: uploads read where they lie).
struct StackRows {
  const char* tile0;
  int64_t row_bytes;
  __device__ __forceinline__ const char* operator()(int i) const { return tile0 + (int64_t)i * row_bytes; }
};
struct PtrRows {
  const float* const* __restrict__ ptr;  // wave-uniform index: scalar loads
  int64_t off_bytes;
  __device__ __forceinline__ const char* operator()(int i) const {
    return reinterpret_cast<const char*>(ptr[i]) + off_bytes;
  }
};

// The rolling register pipeline over rows 0..n-1 of one piece (nq full quads, `bytes` = nq*16
// per row; lane l owns quads l, l+64W, ...): acc[v] = sum_i w[i]*x[i] in list order.
template <class P, int V, int D, int W, bool NT, class R>
__device__ __forceinline__ void rows_sweep(const R& row, uint32_t bytes, int n,
                                           const typename P::w_t* __restrict__ w,
                                           typename vec4<typename P::acc_t>::type (&acc)[V],
                                           int voff = (int)threadIdx.x * 16) {
  typedef typename vec4<float>::type XV;
  XV x[D][V];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (1 + d < n) {
      const __amdgpu_buffer_rsrc_t r = row_rsrc(row(1 + d), bytes);
#pragma unroll
      for (int v = 0; v < V; ++v) x[d][v] = buf_load_quad<NT>(r, voff + v * 64 * W * 16, 0);
    }
  {
    const __amdgpu_buffer_rsrc_t r = row_rsrc(row(0), bytes);
    const typename P::w_t w0 = w[0];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = quad_mul<P>(w0, buf_load_quad<NT>(r, voff + v * 64 * W * 16, 0));
  }
  // rows 1..n-1: slot d holds row i+d; consume it, refill it with row i+d+D (steady state:
  // every refill is a real row, so no branch)
  int i = 1;
  for (; i + 2 * D <= n; i += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const typename P::w_t wi = w[i + d];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = quad_axpy<P>(acc[v], wi, x[d][v]);
      // pin the order "consume slot d, then refill it": if the scheduler hoists the refill
      // (or the products of later slots) the old values need copies, and the copies wait for
      // every in-flight row — the pipeline collapses into batches
      __builtin_amdgcn_sched_barrier(0);
      const __amdgpu_buffer_rsrc_t r = row_rsrc(row(i + d + D), bytes);
#pragma unroll
      for (int v = 0; v < V; ++v) x[d][v] = buf_load_quad<NT>(r, voff + v * 64 * W * 16, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // drain: fewer than 2*D rows left (wave-uniform branches)
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (i + d < n) {
      const typename P::w_t wi = w[i + d];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = quad_axpy<P>(acc[v], wi, x[d][v]);
      if (i + d + D < n) {
        const __amdgpu_buffer_rsrc_t r = row_rsrc(row(i + d + D), bytes);
#pragma unroll
        for (int v = 0; v < V; ++v) x[d][v] = buf_load_quad<NT>(r, voff + v * 64 * W * 16, 0);
      }
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (i + D + d < n) {
      const typename P::w_t wi = w[i + D + d];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = quad_axpy<P>(acc[v], wi, x[d][v]);
    }
  }
}

}  // namespace fa
