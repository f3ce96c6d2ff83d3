// r3m_amd — the pooling family for NHWC activations on gfx950: MaxPool 3x3/2, the stem tail fused around it (BatchNorm + ReLU +
// MaxPool forward; MaxPool-backward + ReLU/BatchNorm-backward, both passes) and the global average pool. HBM-bound passes like the
// streaming BatchNorm passes of bn.hip, whose cache policy and vector helpers (bn_dev.h) they share.
//
// Reference semantics: torchvision ResNet ReLU + MaxPool2d(3,2,1) and AdaptiveAvgPool2d(1).
#include "bn_dev.h"

namespace r3m {

// ---------------------------------------------------------------------------------------------------------
// MaxPool2d(kernel 3, stride 2, padding 1), NHWC. Forward keeps the window-local argmax (0..8, first maximum in
// row-major scan order, like ATen) in one byte per output element; backward is a gather over the <= 4 windows that
// contain an input pixel, so it needs neither atomics nor a zero-fill pass.
// ---------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ Z, T* __restrict__ P,
                                                           unsigned char* __restrict__ amax, long long total, int Hi, int Wi,
                                                           int Ho, int Wo, int C4) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  long long t = idx / C4;
  const int px = (int)(t % Wo); t /= Wo;
  const int py = (int)(t % Ho);
  const long long n = t / Ho;
  f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int bi[4] = {0, 0, 0, 0};
  bool first = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int y = py * 2 - 1 + i;
    if ((unsigned)y >= (unsigned)Hi) continue;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int x = px * 2 - 1 + j;
      if ((unsigned)x >= (unsigned)Wi) continue;
      const f32x4 v = ld4t(Z + (((n * Hi + y) * Wi + x) * C4 + c4) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (first || v[e] > best[e]) { best[e] = v[e]; bi[e] = i * 3 + j; }
      first = false;
    }
  }
  st4t(P + idx * 4, best);
  *reinterpret_cast<uchar4*>(amax + idx * 4) = make_uchar4((unsigned char)bi[0], (unsigned char)bi[1], (unsigned char)bi[2], (unsigned char)bi[3]);
}

int launch_maxpool_fwd(const void* Z, void* P, unsigned char* amax, int N, int Hi, int Wi, int C, int dt, hipStream_t s) {
  const int Ho = (Hi + 2 - 3) / 2 + 1, Wo = (Wi + 2 - 3) / 2 + 1;
  const long long total = (long long)N * Ho * Wo * (C / 4);
  DT_DISPATCH(dt, "maxpool_fwd",
              hipLaunchKernelGGL((maxpool_fwd_kernel<T>), dim3(ceil_div(total, 256)), dim3(256), 0, s, static_cast<const T*>(Z),
                                 static_cast<T*>(P), amax, total, Hi, Wi, Ho, Wo, C / 4));
  return check_launch("maxpool_fwd");
}

template <class T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ dP, const unsigned char* __restrict__ amax,
                                                           T* __restrict__ dZ, long long total, int Hi, int Wi, int Ho,
                                                           int Wo, int C4) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  long long t = idx / C4;
  const int x = (int)(t % Wi); t /= Wi;
  const int y = (int)(t % Hi);
  const long long n = t / Hi;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  // windows py with 2*py-1 <= y <= 2*py+1
  const int py0 = y >> 1, py1 = (y + 1) >> 1;
  const int px0 = x >> 1, px1 = (x + 1) >> 1;
  for (int py = py0; py <= py1; ++py) {
    if (py >= Ho) continue;
    const int i = y - (py * 2 - 1);
    for (int px = px0; px <= px1; ++px) {
      if (px >= Wo) continue;
      const int j = x - (px * 2 - 1);
      const int code = i * 3 + j;
      const long long o = (((n * Ho + py) * Wo + px) * C4 + c4) * 4;
      const uchar4 a = *reinterpret_cast<const uchar4*>(amax + o);
      const f32x4 d = ld4t(dP + o);
      if (a.x == code) g[0] += d[0];
      if (a.y == code) g[1] += d[1];
      if (a.z == code) g[2] += d[2];
      if (a.w == code) g[3] += d[3];
    }
  }
  st4t(dZ + idx * 4, g);
}

int launch_maxpool_bwd(const void* dP, const unsigned char* amax, void* dZ, int N, int Hi, int Wi, int C, int dt, hipStream_t s) {
  const int Ho = (Hi + 2 - 3) / 2 + 1, Wo = (Wi + 2 - 3) / 2 + 1;
  const long long total = (long long)N * Hi * Wi * (C / 4);
  DT_DISPATCH(dt, "maxpool_bwd",
              hipLaunchKernelGGL((maxpool_bwd_kernel<T>), dim3(ceil_div(total, 256)), dim3(256), 0, s, static_cast<const T*>(dP), amax,
                                 static_cast<T*>(dZ), total, Hi, Wi, Ho, Wo, C / 4));
  return check_launch("maxpool_bwd");
}

// ---------------------------------------------------------------------------------------------------------
// Stem tail fused: BatchNorm + ReLU + MaxPool (forward) and MaxPool-backward + ReLU/BatchNorm-backward (both passes).
// The activated stem output Z0 [F,112,112,64] is the largest tensor of the network (4.1 GB fp32 at 1280 frames); the
// unfused sequence wrote it, re-read it for the pooling, and in backward wrote / twice re-read the equally large dZ0.
// Fused, Z0 and dZ0 never exist: forward reads Y0 and writes the pooled tensor + argmax; the backward passes read Y0 and
// gather dZ0 on the fly from the 4x smaller pooled gradient (L2 hits). Arithmetic per element is unchanged: z =
// relu(fmaf(y, scale, shift)) (rounded to the storage type before the comparison, as the stored Z0 was), first maximum in
// scan order, dz = sum of the pooled gradients whose argmax points here (rounded to the storage type as the stored dZ0 was).
// ---------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void bn_relu_maxpool_fwd_kernel(const T* __restrict__ Y, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, T* __restrict__ P,
                                                                   unsigned char* __restrict__ amax, long long total, int Hi,
                                                                   int Wi, int Ho, int Wo, int CV) {
  constexpr int V4 = PoolVec<T>::V4, V = 4 * V4;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % CV);
  long long t = idx / CV;
  const int px = (int)(t % Wo); t /= Wo;
  const int py = (int)(t % Ho);
  const long long n = t / Ho;
  f32x4 sc[V4], sh[V4], best[V4];
  unsigned bi[V4];
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    sc[k] = ld4(scale + cv * V + 4 * k); sh[k] = ld4(shift + cv * V + 4 * k);
    best[k] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    bi[k] = 0u;
  }
  bool first = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int y = py * 2 - 1 + i;
    if ((unsigned)y >= (unsigned)Hi) continue;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int x = px * 2 - 1 + j;
      if ((unsigned)x >= (unsigned)Wi) continue;
      f32x4 yv[V4];
      ldv<V4>(Y + (((n * Hi + y) * Wi + x) * CV + cv) * V, yv);
#pragma unroll
      for (int k = 0; k < V4; ++k) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(yv[k][e], sc[k][e], sh[k][e]), 0.f);
        v = round_as<T>(v);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (first || v[e] > best[k][e]) { best[k][e] = v[e]; bi[k] = (bi[k] & ~(0xffu << (8 * e))) | ((unsigned)(i * 3 + j) << (8 * e)); }
      }
      first = false;
    }
  }
  stv<V4>(P + idx * V, best, false);
  if constexpr (V4 == 1) *reinterpret_cast<unsigned*>(amax + idx * V) = bi[0];
  else *reinterpret_cast<uint2*>(amax + idx * V) = make_uint2(bi[0], bi[1]);
}

// bf16 form of the fused forward. The activated values are >= 0 and rounded to bf16, so as fp32 bit patterns they order like
// integers and their low 16 bits are free: key = bits(z) | (15 - code) turns "first maximum in scan order" into ONE integer max per
// candidate (largest value, then smallest window code), instead of a compare and two selects. A thread owns (px, 8 channels) and walks
// POOL_SEG consecutive output rows downwards: the horizontal 3-tap maxima of input row 2*py+1 are carried into window py+1 (whose
// row 2*(py+1)-1 it is) with the code's row part re-based by plain subtraction (the low bits never borrow: 15 - 3i - j >= 7), so an
// output costs two new input rows, not three. Measured against the one-output-per-thread kernel above: see DESIGN.md §4.2.
constexpr int POOL_SEG = 8;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct Keys8 { int k[8]; };
struct f32x8 { f32x4 lo, hi; };   // the 8 channels' coefficients
__device__ __forceinline__ f32x8 ld8f(const float* p) { f32x8 r; r.lo = ld4(p); r.hi = ld4(p + 4); return r; }

__device__ __forceinline__ void pool_tap_keys(const bf16_t* __restrict__ p, const f32x8& sc, const f32x8& sh, int kc, Keys8& h) {
  const u32x4 raw = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float ylo = __builtin_bit_cast(float, raw[q] << 16), yhi = __builtin_bit_cast(float, raw[q] & 0xffff0000u);
    const float slo = q < 2 ? sc.lo[2 * q] : sc.hi[2 * q - 4], shi = q < 2 ? sc.lo[2 * q + 1] : sc.hi[2 * q - 3];
    const float tlo = q < 2 ? sh.lo[2 * q] : sh.hi[2 * q - 4], thi = q < 2 ? sh.lo[2 * q + 1] : sh.hi[2 * q - 3];
    f32x2 z;
    z[0] = fmaxf(fmaf(ylo, slo, tlo), 0.f);
    z[1] = fmaxf(fmaf(yhi, shi, thi), 0.f);
    const unsigned u = __builtin_bit_cast(unsigned, __builtin_convertvector(z, bf16x2));   // one v_cvt_pk_bf16_f32
    const int klo = (int)((u << 16) | (unsigned)kc), khi = (int)((u & 0xffff0000u) | (unsigned)kc);
    h.k[2 * q] = h.k[2 * q] > klo ? h.k[2 * q] : klo;
    h.k[2 * q + 1] = h.k[2 * q + 1] > khi ? h.k[2 * q + 1] : khi;
  }
}

// horizontal maxima (keys with the column part of the code) of input row y at columns 2*px-1 .. 2*px+1
__device__ __forceinline__ void pool_row_keys(const bf16_t* __restrict__ Yrow, int px, int Wi, int CV, int cv, const f32x8& sc,
                                              const f32x8& sh, Keys8& h) {
#pragma unroll
  for (int e = 0; e < 8; ++e) h.k[e] = 0;
  const bf16_t* p = Yrow + ((long long)(2 * px) * CV + cv) * 8;
  if (px > 0) pool_tap_keys(p - (long long)CV * 8, sc, sh, 15, h);
  pool_tap_keys(p, sc, sh, 14, h);
  if (2 * px + 1 < Wi) pool_tap_keys(p + (long long)CV * 8, sc, sh, 13, h);
}

__global__ __launch_bounds__(1024) void bn_relu_maxpool_fwd16_kernel(const bf16_t* __restrict__ Y, const float* __restrict__ scale,
                                                                     const float* __restrict__ shift, bf16_t* __restrict__ P,
                                                                     unsigned char* __restrict__ amax, int Hi, int Wi, int Ho, int Wo,
                                                                     int CV, int cv_log2, int segs) {
  const int n = blockIdx.x / segs, seg = blockIdx.x - n * segs;
  const int py0 = seg * POOL_SEG;
  const int py1 = py0 + POOL_SEG < Ho ? py0 + POOL_SEG : Ho;
  const int items = Wo * CV;
  const bf16_t* Yn = Y + (long long)n * Hi * Wi * CV * 8;
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int px = it >> cv_log2, cv = it & (CV - 1);
    const f32x8 sc = ld8f(scale + cv * 8), sh = ld8f(shift + cv * 8);
    Keys8 hp, ha, hb;
    if (py0 > 0) pool_row_keys(Yn + (long long)(2 * py0 - 1) * Wi * CV * 8, px, Wi, CV, cv, sc, sh, hp);
    else {
#pragma unroll
      for (int e = 0; e < 8; ++e) hp.k[e] = 0;
    }
    for (int py = py0; py < py1; ++py) {
      pool_row_keys(Yn + (long long)(2 * py) * Wi * CV * 8, px, Wi, CV, cv, sc, sh, ha);
      if (2 * py + 1 < Hi) pool_row_keys(Yn + (long long)(2 * py + 1) * Wi * CV * 8, px, Wi, CV, cv, sc, sh, hb);
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) hb.k[e] = 0;
      }
      u32x4 val;
      unsigned code[2];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        int b[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int e = 2 * q + r;
          int m = ha.k[e] - 3;                       // window row 1; an absent row (key 0) goes negative and loses
          m = hp.k[e] > m ? hp.k[e] : m;             // window row 0
          const int m2 = hb.k[e] - 6;                // window row 2
          b[r] = m > m2 ? m : m2;
          hp.k[e] = hb.k[e];
        }
        val[q] = ((unsigned)b[0] >> 16) | ((unsigned)b[1] & 0xffff0000u);
        const unsigned c2 = ((unsigned)b[0] & 15u) | (((unsigned)b[1] & 15u) << 8);
        if ((q & 1) == 0) code[q >> 1] = c2; else code[q >> 1] |= c2 << 16;
      }
      const long long o = ((((long long)n * Ho + py) * Wo + px) * CV + cv) * 8;
      *reinterpret_cast<u32x4*>(P + o) = val;
      *reinterpret_cast<uint2*>(amax + o) = make_uint2(0x0f0f0f0fu - code[0], 0x0f0f0f0fu - code[1]);
    }
  }
}

static inline int ilog2_exact(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
// threads of a block that owns Wo x CV (pixel, channel-vector) items: all of them when they fit, else 1024 (a multiple of CV <= 256)
static inline int pool_row_threads(int items) { return items >= 1024 ? 1024 : (items + 63) / 64 * 64; }

// Quad rows per block of the pooled reduce: 8, or more when that would give more partial rows than the plain fp32 reduce of the
// same tensor writes (the size every BatchNorm workspace is laid out for).
static inline void pool_reduce_geometry(int N, int Hi, int Wi, int C, int* rq, int* nblk, int* cap_out = nullptr) {
  const int Ho = (Hi + 2 - 3) / 2 + 1;
  const int quad_rows = N * Ho;
  const int cap = bn_bwd_partial_rows((long long)N * Hi * Wi, C, DT_F32);
  int r = ceil_div(quad_rows, cap);
  if (r < 8) r = 8;
  *rq = r;
  *nblk = ceil_div(quad_rows, r);
  if (cap_out) *cap_out = cap;
}

// Every launch figure of the fused stem tail at one shape. The three launchers below take their grids, blocks and LDS sizes from
// here and pool_debug_geometry (r3m_debug_pool_geometry) reports the same struct, so the two cannot drift.
struct PoolGeometry {
  int Ho, Wo, V, CV;                                      // pooled extents; elements per lane (4 fp32 | 8 bf16); channel vectors C / V
  // forward: the bf16 row-walking kernel (fwd_rows = 1: one block per (frame, segment of POOL_SEG output rows), fwd_items = Wo x CV
  // items per block) or the one-output-per-thread kernel (fwd_rows = 0: no segments, 256 outputs per block of 256 threads)
  int fwd_rows, fwd_segs, fwd_blocks, fwd_threads, fwd_items;
  long long fwd_total;                                    // (pixel, channel-vector) outputs of the whole tensor
  // backward (bwd_ok = 0: the backward refuses this C and the fields below are 0). reduce: blocks = partial rows, per_cv = threads
  // of a block that share one channel vector, G = the groups the kernel's second LDS stage adds them in (min(per_cv, 8))
  int bwd_ok, rq, red_blocks, red_threads, red_items, per_cv, G, red_lds, red_cap;
  int app_blocks, app_threads;
};

static PoolGeometry pool_geometry(int N, int Hi, int Wi, int C, int dt) {
  PoolGeometry g = {};
  g.Ho = (Hi + 2 - 3) / 2 + 1;
  g.Wo = (Wi + 2 - 3) / 2 + 1;
  g.V = dt == DT_BF16 ? 4 * PoolVec<bf16_t>::V4 : 4 * PoolVec<float>::V4;
  g.CV = C / g.V;
  g.fwd_total = (long long)N * g.Ho * g.Wo * g.CV;
  g.fwd_rows = dt == DT_BF16 && is_pow2(C) && C <= 2048;
  if (g.fwd_rows) {
    g.fwd_segs = ceil_div(g.Ho, POOL_SEG);
    g.fwd_blocks = N * g.fwd_segs;
    g.fwd_items = g.Wo * g.CV;
    g.fwd_threads = pool_row_threads(g.fwd_items);
  } else {
    g.fwd_blocks = ceil_div(g.fwd_total, 256);
    g.fwd_items = 256;
    g.fwd_threads = 256;
  }
  g.bwd_ok = is_pow2(C) && C >= 8 && C <= 1024;
  if (g.bwd_ok) {
    pool_reduce_geometry(N, Hi, Wi, C, &g.rq, &g.red_blocks, &g.red_cap);
    g.red_items = g.Wo * g.CV;
    g.red_threads = pool_row_threads(g.red_items);
    g.per_cv = g.red_threads / g.CV;                      // bn_bwd_reduce_pool_kernel: nt >> cv_log2
    g.G = g.per_cv < 8 ? g.per_cv : 8;
    g.red_lds = (int)((size_t)2 * (g.V / 4) * g.red_threads * sizeof(f32x4));
    g.app_blocks = N * g.Ho;
    g.app_threads = pool_row_threads(g.Wo * g.CV);
  }
  return g;
}

int launch_bn_relu_maxpool_fwd(const void* Y, const BnCoef& K, void* P, unsigned char* amax, int N, int Hi, int Wi, int C, int dt,
                               hipStream_t s) {
  R3M_REQUIRE(C % 8 == 0, "bn_relu_maxpool_fwd: C=%d must be a multiple of 8", C);
  const PoolGeometry g = pool_geometry(N, Hi, Wi, C, dt);
  if (g.fwd_rows) {
    hipLaunchKernelGGL(bn_relu_maxpool_fwd16_kernel, dim3(g.fwd_blocks), dim3(g.fwd_threads), 0, s, static_cast<const bf16_t*>(Y), K.scale,
                       K.shift, static_cast<bf16_t*>(P), amax, Hi, Wi, g.Ho, g.Wo, g.CV, ilog2_exact(g.CV), g.fwd_segs);
    return check_launch("bn_relu_maxpool_fwd16");
  }
  DT_DISPATCH(dt, "bn_relu_maxpool_fwd", {
    hipLaunchKernelGGL((bn_relu_maxpool_fwd_kernel<T>), dim3(g.fwd_blocks), dim3(g.fwd_threads), 0, s, static_cast<const T*>(Y), K.scale,
                       K.shift, static_cast<T*>(P), amax, g.fwd_total, Hi, Wi, g.Ho, g.Wo, g.CV);
  });
  return check_launch("bn_relu_maxpool_fwd");
}

// Backward through the (never stored) pre-pool activation, quad form. Windows of 3x3 / stride 2 / pad 1 tile the image into 2x2
// quads: quad (qy, qx) = pixels (2qy + a, 2qx + b), a, b in {0, 1}, lies inside its HOME window (qy, qx) (codes 4, 5, 7, 8); its right
// column is also column 0 of window (qy, qx+1) (codes 3, 6), its lower row is row 0 of window (qy+1, qx) (codes 1, 2), and pixel
// (1, 1) is code 0 of window (qy+1, qx+1). One thread = one quad x V channels: four window reads (pooled gradient + argmax bytes,
// the home one coalesced with the pooled tensor's own layout) serve four pixels, all twelve loads are issued before the first use,
// and there is no data-dependent loop. (The per-pixel gather it replaces read 2.25 windows per pixel in a divergent loop with a
// wait per window: 2.2-3.0 TB/s; rounds of dependent L2 hits, not bytes, were the bound.) Per pixel the contributions are added
// in window scan order, as the stand-alone maxpool_bwd_kernel does, and rounded to the storage type as the stored dZ0 was.
template <class T>
struct PoolQuad {
  static constexpr int V4 = PoolVec<T>::V4;
  f32x4 y[4][V4];      // pixel (a, b) at [2a + b]
  f32x4 dz[4][V4];
  bool va, vb;         // row 2qy+1 / column 2qx+1 exist
};

template <class T>
__device__ __forceinline__ void pool_quad(const T* __restrict__ dP, const unsigned char* __restrict__ amax, const T* __restrict__ Y,
                                          long long n, int qy, int qx, int cv, int Hi, int Wi, int Ho, int Wo, int CV, PoolQuad<T>& q) {
  constexpr int V4 = PoolVec<T>::V4, V = 4 * V4;
  const bool hr = qx + 1 < Wo, hd = qy + 1 < Ho;
  q.va = 2 * qy + 1 < Hi;
  q.vb = 2 * qx + 1 < Wi;
  const long long o = (((n * Ho + qy) * Wo + qx) * CV + cv) * V;
  const long long sW = (long long)CV * V, sH = (long long)Wo * CV * V;
  const long long oo[4] = {o, hr ? o + sW : o, hd ? o + sH : o, (hr && hd) ? o + sH + sW : o};
  const long long p = (((n * Hi + 2 * qy) * Wi + 2 * qx) * CV + cv) * V;
  const long long pH = (long long)Wi * CV * V;
  const long long pp[4] = {p, q.vb ? p + sW : p, q.va ? p + pH : p, (q.va && q.vb) ? p + pH + sW : p};
  unsigned a[4][V4];
  f32x4 d[4][V4];
#pragma unroll
  for (int w = 0; w < 4; ++w) ldv_stream<V4>(Y + pp[w], q.y[w]);
#pragma unroll
  for (int w = 0; w < 4; ++w) { ld_codes<V4>(amax + oo[w], a[w]); ldv<V4>(dP + oo[w], d[w]); }
#pragma unroll
  for (int k = 0; k < V4; ++k) {            // a window that does not exist matches no code
    if (!hr) { a[1][k] = 0xffffffffu; a[3][k] = 0xffffffffu; }
    if (!hd) { a[2][k] = 0xffffffffu; a[3][k] = 0xffffffffu; }
  }
#pragma unroll
  for (int k = 0; k < V4; ++k) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned cH = (a[0][k] >> (8 * e)) & 0xffu, cR = (a[1][k] >> (8 * e)) & 0xffu;
      const unsigned cD = (a[2][k] >> (8 * e)) & 0xffu, cX = (a[3][k] >> (8 * e)) & 0xffu;
      const float dH = d[0][k][e], dR = d[1][k][e], dD = d[2][k][e], dX = d[3][k][e];
      q.dz[0][k][e] = cH == 4u ? dH : 0.f;
      q.dz[1][k][e] = (cH == 5u ? dH : 0.f) + (cR == 3u ? dR : 0.f);
      q.dz[2][k][e] = (cH == 7u ? dH : 0.f) + (cD == 1u ? dD : 0.f);
      q.dz[3][k][e] = (((cH == 8u ? dH : 0.f) + (cR == 6u ? dR : 0.f)) + (cD == 2u ? dD : 0.f)) + (cX == 0u ? dX : 0.f);
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) q.dz[w][k] = round_as<T>(q.dz[w][k]);
  }
}

// pass 1 of BatchNorm backward with dZ gathered through the max-pool. A block owns `rq` consecutive quad rows (n, qy) and all
// Wo x CV (quad, channel-vector) items of a row; a thread's channel vector is loop-invariant, its sums stay in registers, and
// the block's threads of one channel vector are combined in a fixed order (two LDS stages) into one partial row.
template <class T>
__global__ __launch_bounds__(1024) void bn_bwd_reduce_pool_kernel(const T* __restrict__ dP, const unsigned char* __restrict__ amax,
                                                                   const T* __restrict__ Y, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd, float* __restrict__ partials,
                                                                   int quad_rows, int rq, int C, int CV, int cv_log2, int Hi, int Wi,
                                                                   int Ho, int Wo) {
  constexpr int V4 = PoolVec<T>::V4, V = 4 * V4;
  extern __shared__ f32x4 pool_red[];            // [2][V4][blockDim.x]
  const int nt = blockDim.x;
  const int cv = threadIdx.x & (CV - 1);
  const int c = cv * V;
  const int items = Wo * CV;
  f32x4 sc[V4], sh[V4], mu[V4], is[V4], s1[V4], s2[V4];
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    sc[k] = ld4(scale + c + 4 * k); sh[k] = ld4(shift + c + 4 * k); mu[k] = ld4(mean + c + 4 * k); is[k] = ld4(invstd + c + 4 * k);
    s1[k] = f32x4{0.f, 0.f, 0.f, 0.f}; s2[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int qr0 = blockIdx.x * rq;
  const int qr1 = qr0 + rq < quad_rows ? qr0 + rq : quad_rows;
  for (int qr = qr0; qr < qr1; ++qr) {
    const int n = qr / Ho, qy = qr - n * Ho;
    for (int it = threadIdx.x; it < items; it += nt) {
      PoolQuad<T> q;
      pool_quad<T>(dP, amax, Y, n, qy, it >> cv_log2, cv, Hi, Wi, Ho, Wo, CV, q);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const bool valid = ((w & 1) == 0 || q.vb) && ((w & 2) == 0 || q.va);
#pragma unroll
        for (int k = 0; k < V4; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float yv = q.y[w][k][e];
            const float g = (valid && fmaf(yv, sc[k][e], sh[k][e]) > 0.f) ? q.dz[w][k][e] : 0.f;
            s1[k][e] += g;
            s2[k][e] = fmaf(g, (yv - mu[k][e]) * is[k][e], s2[k][e]);
          }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V4; ++k) { pool_red[(0 * V4 + k) * nt + threadIdx.x] = s1[k]; pool_red[(1 * V4 + k) * nt + threadIdx.x] = s2[k]; }
  __syncthreads();
  // stage 2: G groups per channel vector, group g adds the threads g, g+G, ... of its vector; stage 3: one thread adds the groups
  const int per_cv = nt >> cv_log2;
  const int G = per_cv < 8 ? per_cv : 8;
  if ((int)threadIdx.x < G * CV) {
    const int g = threadIdx.x >> cv_log2;
#pragma unroll
    for (int k = 0; k < V4; ++k) { s1[k] = f32x4{0.f, 0.f, 0.f, 0.f}; s2[k] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int t = g; t < per_cv; t += G)
#pragma unroll
      for (int k = 0; k < V4; ++k) { s1[k] += pool_red[(0 * V4 + k) * nt + t * CV + cv]; s2[k] += pool_red[(1 * V4 + k) * nt + t * CV + cv]; }
  }
  __syncthreads();
  if ((int)threadIdx.x < G * CV) {
#pragma unroll
    for (int k = 0; k < V4; ++k) { pool_red[(0 * V4 + k) * nt + threadIdx.x] = s1[k]; pool_red[(1 * V4 + k) * nt + threadIdx.x] = s2[k]; }
  }
  __syncthreads();
  if ((int)threadIdx.x < CV) {
    for (int g = 1; g < G; ++g)
#pragma unroll
      for (int k = 0; k < V4; ++k) { s1[k] += pool_red[(0 * V4 + k) * nt + g * CV + cv]; s2[k] += pool_red[(1 * V4 + k) * nt + g * CV + cv]; }
#pragma unroll
    for (int k = 0; k < V4; ++k) {
      st4(partials + ((long long)blockIdx.x * 2 + 0) * C + c + 4 * k, s1[k]);
      st4(partials + ((long long)blockIdx.x * 2 + 1) * C + c + 4 * k, s2[k]);
    }
  }
}

// pass 2: dY = scale * (g - c1 - yhat * c2) with g gathered through the max-pool; one quad row (n, qy) per block.
template <class T>
__global__ __launch_bounds__(1024) void bn_bwd_apply_pool_kernel(const T* __restrict__ dP, const unsigned char* __restrict__ amax,
                                                                  const T* __restrict__ Y, const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ c1,
                                                                  const float* __restrict__ c2, T* __restrict__ dY, int CV, int cv_log2,
                                                                  int Hi, int Wi, int Ho, int Wo) {
  constexpr int V4 = PoolVec<T>::V4, V = 4 * V4;
  const int n = blockIdx.x / Ho, qy = blockIdx.x - n * Ho;
  const int items = Wo * CV;
  const int cv = threadIdx.x & (CV - 1);
  const int c = cv * V;
  f32x4 sc[V4], sh[V4], mu[V4], is[V4], k1[V4], k2[V4];
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    sc[k] = ld4(scale + c + 4 * k); sh[k] = ld4(shift + c + 4 * k); mu[k] = ld4(mean + c + 4 * k); is[k] = ld4(invstd + c + 4 * k);
    k1[k] = ld4(c1 + c + 4 * k); k2[k] = ld4(c2 + c + 4 * k);
  }
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int qx = it >> cv_log2;
    PoolQuad<T> q;
    pool_quad<T>(dP, amax, Y, n, qy, qx, cv, Hi, Wi, Ho, Wo, CV, q);
    const long long p = ((((long long)n * Hi + 2 * qy) * Wi + 2 * qx) * CV + cv) * V;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      f32x4 o[V4];
#pragma unroll
      for (int k = 0; k < V4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float yv = q.y[w][k][e];
          const float g = fmaf(yv, sc[k][e], sh[k][e]) > 0.f ? q.dz[w][k][e] : 0.f;
          const float yh = (yv - mu[k][e]) * is[k][e];
          o[k][e] = sc[k][e] * (g - k1[k][e] - yh * k2[k][e]);
        }
      const bool valid = ((w & 1) == 0 || q.vb) && ((w & 2) == 0 || q.va);
      if (valid) stv<V4>(dY + p + (long long)(w & 1) * CV * V + (long long)(w >> 1) * Wi * CV * V, o, true);
    }
  }
}

// rows of the partial buffer the pooled reduce writes
int bn_bwd_pool_partial_rows(int N, int Hi, int Wi, int C) {
  int rq, nblk;
  pool_reduce_geometry(N, Hi, Wi, C, &rq, &nblk);
  return nblk;
}

static int launch_bn_bwd_reduce_pool(const void* dP, const unsigned char* amax, const void* Y, const BnCoef& K, float* partials, int N,
                                     int Hi, int Wi, int C, int dt, hipStream_t s) {
  const PoolGeometry g = pool_geometry(N, Hi, Wi, C, dt);
  R3M_REQUIRE(g.bwd_ok, "bn_bwd_reduce_pool: C=%d must be a power of two in [8, 1024]", C);
  DT_DISPATCH(dt, "bn_bwd_reduce_pool", {
    hipLaunchKernelGGL((bn_bwd_reduce_pool_kernel<T>), dim3(g.red_blocks), dim3(g.red_threads), (size_t)g.red_lds, s,
                       static_cast<const T*>(dP), amax, static_cast<const T*>(Y), K.scale, K.shift, K.mean, K.invstd, partials, N * g.Ho, g.rq,
                       C, g.CV, ilog2_exact(g.CV), Hi, Wi, g.Ho, g.Wo);
  });
  return check_launch("bn_bwd_reduce_pool");
}

static int launch_bn_bwd_apply_pool(const void* dP, const unsigned char* amax, const void* Y, const BnCoef& K, void* dY, int N, int Hi,
                                    int Wi, int C, int dt, hipStream_t s) {
  const PoolGeometry g = pool_geometry(N, Hi, Wi, C, dt);
  R3M_REQUIRE(g.bwd_ok, "bn_bwd_apply_pool: C=%d must be a power of two in [8, 1024]", C);
  DT_DISPATCH(dt, "bn_bwd_apply_pool", {
    hipLaunchKernelGGL((bn_bwd_apply_pool_kernel<T>), dim3(g.app_blocks), dim3(g.app_threads), 0, s, static_cast<const T*>(dP), amax,
                       static_cast<const T*>(Y), K.scale, K.shift, K.mean, K.invstd, K.c1, K.c2, static_cast<T*>(dY), g.CV, ilog2_exact(g.CV),
                       Hi, Wi, g.Ho, g.Wo);
  });
  return check_launch("bn_bwd_apply_pool");
}

// What the launchers above pick for [N, Hi, Wi, C] of dtype dt, without launching anything (r3m_debug_pool_geometry; the index names
// are in include/r3m_hip.h)
int pool_debug_geometry(int N, int Hi, int Wi, int C, int dt, int* out, int cap) {
  R3M_REQUIRE(out && cap >= 18, "debug_pool_geometry: the output buffer needs 18 ints");
  R3M_REQUIRE(dt == DT_F32 || dt == DT_BF16, "debug_pool_geometry: unknown dtype %d", dt);
  R3M_REQUIRE(N >= 1 && Hi >= 1 && Wi >= 1 && C >= 8 && C % 8 == 0, "debug_pool_geometry: N=%d Hi=%d Wi=%d C=%d", N, Hi, Wi, C);
  const PoolGeometry g = pool_geometry(N, Hi, Wi, C, dt);
  const int v[18] = {g.Ho, g.Wo, g.fwd_rows, g.fwd_segs, g.fwd_blocks, g.fwd_threads, g.fwd_items, g.rq, g.red_blocks, g.red_threads,
                     g.red_items, g.per_cv, g.G, g.red_lds, g.red_cap, g.app_blocks, g.app_threads, g.V};
  for (int i = 0; i < 18; ++i) out[i] = v[i];
  return 0;
}

int bn_bwd_pool(const void* dP, const unsigned char* amax, const BnBwdSide& b, bool apply, int N, int Hi, int Wi, int C,
                int use_batch_stats, const BnScratch& w, int dt, hipStream_t s) {
  if (b.sums) {
    TRY(launch_bn_bwd_reduce_pool(dP, amax, b.Y, b.K, w.partial, N, Hi, Wi, C, dt, s));
    TRY(bn_bwd_combine(w.partial, bn_bwd_pool_partial_rows(N, Hi, Wi, C), (long long)N * Hi * Wi, use_batch_stats, b.out, nullptr, C, w.acc, s));
  }
  if (!apply) return 0;
  return launch_bn_bwd_apply_pool(dP, amax, b.Y, b.apply_coef(), b.dY, N, Hi, Wi, C, dt, s);
}

// ---------------------------------------------------------------------------------------------------------
// AdaptiveAvgPool2d(1) + flatten: [N, HW, C] -> [N, C]  and its backward (broadcast of dH / HW)
// ---------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const T* __restrict__ X, float* __restrict__ H, long long total,
                                                           int HW, int C4) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  const long long n = idx / C4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < HW; ++p) s += ld4t(X + ((n * HW + p) * C4 + c4) * 4);
  const float d = (float)HW;
#pragma unroll
  for (int e = 0; e < 4; ++e) s[e] = s[e] / d;
  st4(H + idx * 4, s);
}

int launch_avgpool_fwd(const void* X, float* H, int N, int HW, int C, int dt, hipStream_t s) {
  const long long total = (long long)N * (C / 4);
  DT_DISPATCH(dt, "avgpool_fwd",
              hipLaunchKernelGGL((avgpool_fwd_kernel<T>), dim3(ceil_div(total, 256)), dim3(256), 0, s, static_cast<const T*>(X), H, total, HW, C / 4));
  return check_launch("avgpool_fwd");
}

template <class T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ dH, T* __restrict__ dX, long long total,
                                                           int HW, int C4) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  const long long n = idx / ((long long)HW * C4);
  f32x4 g = ld4(dH + (n * C4 + c4) * 4);
  const float d = (float)HW;
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = g[e] / d;
  st4t(dX + idx * 4, g);
}

int launch_avgpool_bwd(const float* dH, void* dX, int N, int HW, int C, int dt, hipStream_t s) {
  const long long total = (long long)N * HW * (C / 4);
  DT_DISPATCH(dt, "avgpool_bwd",
              hipLaunchKernelGGL((avgpool_bwd_kernel<T>), dim3(ceil_div(total, 256)), dim3(256), 0, s, dH, static_cast<T*>(dX), total, HW, C / 4));
  return check_launch("avgpool_bwd");
}

}  // namespace r3m
