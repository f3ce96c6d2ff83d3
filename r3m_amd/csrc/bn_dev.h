// r3m_amd — device helpers shared by the BatchNorm passes (bn.hip) and the pooling family (bn_pool.hip): the traversal order and
// cache policy of the streamed tensors, the storage-type dispatch, and the f32x4[V4] vector helpers (V4 = 1: 4 channels per lane,
// V4 = 2: 8 channels, one 16-byte bf16 access).
#pragma once
#include "common.h"
#include "conv_dev.h"

// Traversal order of the streaming BatchNorm passes. The 256 MiB Infinity Cache still holds the TAIL of the tensor the previous
// kernel streamed; a consumer that walks the rows in the opposite direction hits it first. R3M_BN_REV bit 1: forward apply, bit 2:
// backward reduce, bit 4: backward apply walk from the last block down (compile-time; variants built by tools/build_ab.sh).
#ifndef R3M_BN_REV
#define R3M_BN_REV 0
#endif
#define BN_BID(bit) ((R3M_BN_REV & (bit)) ? (gridDim.x - 1 - blockIdx.x) : blockIdx.x)

namespace r3m {

// activations are float or bf16_t (T); per-channel coefficients, statistics and partial sums are always fp32
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// Streamed activation tensors (each byte touched once per pass, GBs apart from its next use) use the non-temporal cache
// policy: +3-7 % on every pass (fp32 backward 5.6 -> 6.0 TB/s, forward+residual 6.0 -> 6.35; tools/bn_bench.py against a
// -DR3M_BN_NT=0 build), ≈0.6 % of the whole step.
#ifndef R3M_BN_NT
#define R3M_BN_NT 1
#endif
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 lds4(const float* p) {
#if R3M_BN_NT
  return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
#else
  return *reinterpret_cast<const f32x4*>(p);
#endif
}
__device__ __forceinline__ f32x4 lds4(const bf16_t* p) {
#if R3M_BN_NT
  const u32x2 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
  return __builtin_convertvector(__builtin_bit_cast(bf16x4, raw), f32x4);
#else
  return ld4t(p);
#endif
}
__device__ __forceinline__ void sts4(float* p, f32x4 v) {
#if R3M_BN_NT
  __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
#else
  *reinterpret_cast<f32x4*>(p) = v;
#endif
}
__device__ __forceinline__ void sts4(bf16_t* p, f32x4 v) {
#if R3M_BN_NT
  __builtin_nontemporal_store(__builtin_bit_cast(u32x2, __builtin_convertvector(v, bf16x4)), reinterpret_cast<u32x2*>(p));
#else
  st4t(p, v);
#endif
}

// dispatch a templated kernel launch on the activation storage type
#define DT_DISPATCH(dt, NAME, ...)                                        \
  do {                                                                    \
    if ((dt) == DT_BF16) { typedef bf16_t T; __VA_ARGS__; }               \
    else if ((dt) == DT_F32) { typedef float T; __VA_ARGS__; }            \
    else { set_last_error(NAME ": unknown dtype %d", (int)(dt)); return 1; } \
  } while (0)

static inline bool is_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

// v as the storage type T holds it
template <class T>
__device__ __forceinline__ f32x4 round_as(f32x4 v);
template <>
__device__ __forceinline__ f32x4 round_as<float>(f32x4 v) { return v; }
template <>
__device__ __forceinline__ f32x4 round_as<bf16_t>(f32x4 v) { return __builtin_convertvector(__builtin_convertvector(v, bf16x4), f32x4); }

// Channel vectors per thread of the pooling kernels: 4 channels (one f32x4) for fp32, 8 channels (two f32x4, one 16-byte load) for
// bf16 — the bf16 tensors are half the bytes, so the 4-wide kernels were instruction-bound there (measured 4.1 / 2.5 / 3.6 TB/s
// against 7.2 / 5.4 / 5.5 TB/s for fp32). (The streaming passes of bn.hip take V4 from the launcher: bf16 with C = 4 runs 4-wide.)
template <class T>
struct PoolVec { static constexpr int V4 = 1; };
template <>
struct PoolVec<bf16_t> { static constexpr int V4 = 2; };

__device__ __forceinline__ void widen8(bf16x8 v, f32x4 (&q)[2]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { q[0][e] = (float)v[e]; q[1][e] = (float)v[4 + e]; }
}
__device__ __forceinline__ bf16x8 narrow8(const f32x4 (&q)[2]) {
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[e] = (bf16_t)q[0][e]; o[4 + e] = (bf16_t)q[1][e]; }
  return o;
}

template <int V4, class T>
__device__ __forceinline__ void ldv(const T* __restrict__ p, f32x4 (&q)[V4]) {   // cached: the gathered, re-read operands
  if constexpr (V4 == 1) q[0] = ld4t(p);
  else widen8(*reinterpret_cast<const bf16x8*>(p), q);
}
template <int V4, class T>
__device__ __forceinline__ void ldv_stream(const T* __restrict__ p, f32x4 (&q)[V4]) {   // read once
  if constexpr (V4 == 1) {
    q[0] = lds4(p);
  } else {
#if R3M_BN_NT
    widen8(__builtin_bit_cast(bf16x8, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p))), q);
#else
    widen8(*reinterpret_cast<const bf16x8*>(p), q);
#endif
  }
}
template <int V4, class T>
__device__ __forceinline__ void stv(T* __restrict__ p, const f32x4 (&q)[V4], bool stream) {
  if constexpr (V4 == 1) {
    if (stream) sts4(p, q[0]); else st4t(p, q[0]);
  } else {
    const bf16x8 o = narrow8(q);
    if (stream && R3M_BN_NT) __builtin_nontemporal_store(__builtin_bit_cast(u32x4, o), reinterpret_cast<u32x4*>(p));
    else *reinterpret_cast<bf16x8*>(p) = o;
  }
}
template <int V4>
__device__ __forceinline__ void ld_codes(const unsigned char* __restrict__ p, unsigned (&a)[V4]) {   // 4 argmax codes per word
  if constexpr (V4 == 1) a[0] = *reinterpret_cast<const unsigned*>(p);
  else { const uint2 v = *reinterpret_cast<const uint2*>(p); a[0] = v.x; a[1] = v.y; }
}
template <int V4>
__device__ __forceinline__ void ldc(const float* __restrict__ p, f32x4 (&q)[V4]) {   // per-channel coefficients (fp32, L1/L2 hits)
#pragma unroll
  for (int k = 0; k < V4; ++k) q[k] = ld4(p + 4 * k);
}

}  // namespace r3m
