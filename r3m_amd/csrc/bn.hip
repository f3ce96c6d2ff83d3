// r3m_amd — BatchNorm2d (train / eval) forward + backward fused with ReLU and the residual add, for NHWC fp32 / bf16 activations
// on gfx950 (the pooling family, with the stem tail fused around the max-pool, is bn_pool.hip). All of these are HBM-bound
// passes: 16 B / lane coalesced streams, per-channel coefficients re-read from L1/L2, fixed-order reductions (bit-reproducible
// run to run).
//
// Reference semantics: torchvision ResNet BatchNorm2d(eps=1e-5, momentum=0.1) + ReLU.
//   train: normalise with the biased batch variance, update running_var with the unbiased one;
//   statistics: the conv epilogue (conv.hip EPI_STATS) leaves fp32 per-row-block sum / sum-of-squares, which are
//   combined here in fp64, so E[y^2] - mean^2 is evaluated without fp32 cancellation.
#include "bn_dev.h"
#include <cstdlib>

namespace r3m {

// ---------------------------------------------------------------------------------------------------------
// partials [rows][2][C] (fp32)  ->  acc [S][2][C] (fp64), S = gridDim.y slices, fixed order inside a slice
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_stats_reduce_kernel(const float* __restrict__ partials, int rows, int C,
                                                               double* __restrict__ acc) {
  __shared__ double red[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  double s = 0.0, ss = 0.0;
  if (c < C) {
    for (int r = blockIdx.y * 4 + ty; r < rows; r += 4 * gridDim.y) {
      s += (double)partials[((long long)r * 2 + 0) * C + c];
      ss += (double)partials[((long long)r * 2 + 1) * C + c];
    }
  }
  red[0][ty][tx] = s;
  red[1][ty][tx] = ss;
  __syncthreads();
  if (ty == 0 && c < C) {
    s = red[0][0][tx] + red[0][1][tx] + red[0][2][tx] + red[0][3][tx];
    ss = red[1][0][tx] + red[1][1][tx] + red[1][2][tx] + red[1][3][tx];
    acc[((long long)blockIdx.y * 2 + 0) * C + c] = s;
    acc[((long long)blockIdx.y * 2 + 1) * C + c] = ss;
  }
}

// Slices of the partial-row reduce: enough blocks for narrow layers with MANY rows (64 channels at 56 x 56 x 1280 frames: 62 720
// EPI_BNRED rows, one column block — 64 slices left 192 CUs idle and a 245-row serial walk per thread), within the accumulator
// buffer of 64 x 2 x 2048 doubles (S * C <= 131072).
static inline int slice_cap(int C) {
  int cap = 131072 / (C > 0 ? C : 1);
  if (cap > 256) cap = 256;
  if (cap < 64) cap = 64;
  return cap;
}
static inline int reduce_slices(int rows, int C) {
  int s = (rows + 15) / 16;
  const int cap = slice_cap(C);
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  return s;
}

// bytes of the fp64 slice accumulator for C channels (the largest slice count reduce_slices can pick for that C)
size_t bn_acc_bytes(int C) {
  return (size_t)slice_cap(C) * 2 * C * 8;
}

// acc must hold 131072 * 2 doubles (64 slices x 2 x 2048 channels, or more slices of fewer channels); the slice count is a pure function of the partial-row count (reduce_slices), so
// the finalize launchers below take the same `stat_rows` and recompute it.
static int launch_bn_stats_reduce(const float* partials, int rows, int C, double* acc, hipStream_t s) {
  const int S = reduce_slices(rows, C);
  hipLaunchKernelGGL(bn_stats_reduce_kernel, dim3(ceil_div(C, 64), S), dim3(256), 0, s, partials, rows, C, acc);
  return check_launch("bn_stats_reduce");
}

// Sum the S fp64 slices of acc[S][2][C] for one channel. Block = 64 channels x SG slice groups (group g adds slices g, g+SG, ...,
// combined in group order -> deterministic); returns true for the thread that owns the channel's totals. These per-layer
// kernels are pure latency: one thread walking 64 dependent slices made them 19 us each (~4 ms per step), 4 groups 15 us
// (S is up to 256); 16 groups with the loads of four slices in flight: see DESIGN.md §5.
constexpr int SG = 16;
__device__ __forceinline__ bool slice_totals(const double* __restrict__ acc, int S, int C, int* c_out, double* s_out, double* ss_out) {
  __shared__ double red[2][SG][64];
  const int tx = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  double s = 0.0, ss = 0.0;
  if (c < C) {
#pragma unroll 4
    for (int i = g; i < S; i += SG) {
      s += acc[((long long)i * 2 + 0) * C + c];
      ss += acc[((long long)i * 2 + 1) * C + c];
    }
  }
  red[0][g][tx] = s;
  red[1][g][tx] = ss;
  __syncthreads();
  *c_out = c;
  s = red[0][0][tx];
  ss = red[1][0][tx];
#pragma unroll
  for (int k = 1; k < SG; ++k) { s += red[0][k][tx]; ss += red[1][k][tx]; }
  *s_out = s;
  *ss_out = ss;
  return g == 0 && c < C;
}

__global__ __launch_bounds__(64 * SG) void bn_finalize_kernel(const double* __restrict__ acc, int S, double inv_count,
                                                           double unbias, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ running_mean,
                                                           float* __restrict__ running_var, float momentum, float eps,
                                                           float* __restrict__ mean_o, float* __restrict__ invstd_o,
                                                           float* __restrict__ scale_o, float* __restrict__ shift_o, int C) {
  int c;
  double s, ss;
  if (!slice_totals(acc, S, C, &c, &s, &ss)) return;
  const double mean = s * inv_count;
  double var = ss * inv_count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float meanf = (float)mean;
  const float varf = (float)var;
  const float invstd = 1.0f / sqrtf(varf + eps);
  const float sc = gamma[c] * invstd;
  mean_o[c] = meanf;
  invstd_o[c] = invstd;
  scale_o[c] = sc;
  shift_o[c] = fmaf(-meanf, sc, beta[c]);
  if (running_mean) {
    running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * meanf;
    running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)(var * unbias);
  }
}

// `stat_rows` = number of partial rows that were reduced (fixes the slice count), `count` = elements per channel.
static int launch_bn_finalize_rows(const double* acc, int stat_rows, long long count, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, float momentum, float eps, const BnCoefOut& o, int C,
                                   hipStream_t s) {
  const double inv_count = 1.0 / (double)count;
  const double unbias = count > 1 ? (double)count / (double)(count - 1) : 1.0;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(C, 64)), dim3(64 * SG), 0, s, acc, reduce_slices(stat_rows, C), inv_count,
                     unbias, gamma, beta, running_mean, running_var, momentum, eps, o.mean, o.invstd, o.scale, o.shift, C);
  return check_launch("bn_finalize");
}

int bn_train_coeffs(const float* stats, int stats_rows, long long count, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float momentum, float eps, const BnCoefOut& o, int C, double* acc, hipStream_t s) {
  TRY(launch_bn_stats_reduce(stats, stats_rows, C, acc, s));
  return launch_bn_finalize_rows(acc, stats_rows, count, gamma, beta, running_mean, running_var, momentum, eps, o, C, s);
}

// one channel's eval-mode coefficients from the running statistics: the arithmetic of both kernels below
__device__ __forceinline__ void bn_eval_coeffs_one(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                                   float* mean_o, float* invstd_o, float* scale_o, float* shift_o, int c) {
  const float invstd = 1.0f / sqrtf(rv[c] + eps);
  const float sc = gamma[c] * invstd;
  mean_o[c] = rm[c];
  invstd_o[c] = invstd;
  scale_o[c] = sc;
  shift_o[c] = fmaf(-rm[c], sc, beta[c]);
}
__global__ __launch_bounds__(256) void bn_eval_coeffs_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ rm, const float* __restrict__ rv,
                                                              float eps, float* __restrict__ mean_o, float* __restrict__ invstd_o,
                                                              float* __restrict__ scale_o, float* __restrict__ shift_o, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  bn_eval_coeffs_one(gamma, beta, rm, rv, eps, mean_o, invstd_o, scale_o, shift_o, c);
}

// The same coefficients for EVERY BatchNorm of a plan in one launch (plan_inference_prepare): the layer table travels in the kernel
// arguments (at most 56 entries), so the call makes no allocation and no host-to-device copy. Block b serves channels
// [256 (b - blk0), ...) of the entry whose block range holds b.
__global__ __launch_bounds__(256) void bn_eval_coeffs_table_kernel(const float* params, const float* bufs, float* arena, const BnEvalTable t,
                                                                    float eps) {
  int i = 0;
  while (i + 1 < t.n && (int)blockIdx.x >= t.e[i + 1].blk0) ++i;
  const BnEvalEntry e = t.e[i];
  const int c = ((int)blockIdx.x - e.blk0) * 256 + threadIdx.x;
  if (c >= e.C) return;
  const BnCoefOut o = bn_coef_out(arena + e.coef_off, e.C);
  bn_eval_coeffs_one(params + e.gamma_off, params + e.beta_off, bufs + e.rm_off, bufs + e.rv_off, eps, o.mean, o.invstd, o.scale, o.shift, c);
}

int launch_bn_eval_coeffs_table(const float* params, const float* bufs, float* arena, const BnEvalTable& t, float eps, hipStream_t s) {
  if (t.n <= 0) return 0;
  hipLaunchKernelGGL(bn_eval_coeffs_table_kernel, dim3(t.blocks), dim3(256), 0, s, params, bufs, arena, t, eps);
  return check_launch("bn_eval_coeffs_table");
}

int launch_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                          const BnCoefOut& o, int C, hipStream_t s) {
  hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, s, gamma, beta, running_mean,
                     running_var, eps, o.mean, o.invstd, o.scale, o.shift, C);
  return check_launch("bn_eval_coeffs");
}

// The streaming passes below are each written once for <T, V4>: a lane owns V = 4 * V4 consecutive channels, one 16-byte access of
// fp32 (V4 = 1) or of bf16 with C a multiple of 8 (V4 = 2); bf16 with C = 4 runs <bf16_t, 1>. Per-channel coefficients are f32x4 x[V4].

// ---------------------------------------------------------------------------------------------------------
// Z = [relu]( scale*Y + shift  [+ R]  [+ scale2*Y2 + shift2] )      (one read per operand, one write)
//   R      : identity branch (already activated block input)
//   Y2,... : downsample branch raw conv output with its own BatchNorm coefficients
// ---------------------------------------------------------------------------------------------------------
template <int MODE, class T, int V4>  // 0: plain, 1: + R, 2: + affine(Y2)
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const T* __restrict__ Y, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const T* __restrict__ R,
                                                          const float* __restrict__ scale2, const float* __restrict__ shift2,
                                                          T* __restrict__ Z, long long n, int cvmask, int relu,
                                                          unsigned* __restrict__ maskbits, int span) {
  // A block owns `span` consecutive items and walks them 256 at a time; the launcher only picks span > 256 when 256 is a
  // multiple of C/V, so the thread's channels and their coefficients are loop-invariant (loaded once — at 16 B of payload per load
  // the coefficient vectors would otherwise be most of the L1 traffic — and the block's accesses stay one contiguous range).
  // n is a multiple of LPW when maskbits is used: the lanes of a mask word are all in or all out.
  constexpr int V = 4 * V4, LPW = 32 / V;   // LPW: lanes per 32-bit mask word
  long long i = (long long)BN_BID(1) * span + threadIdx.x;
  if (i >= n) return;
  const long long end = min((long long)(BN_BID(1) + 1) * span, n);
  const int c = ((int)(i & cvmask)) * V;
  f32x4 sc[V4], sh[V4], sc2[V4], sh2[V4];
  ldc(scale + c, sc); ldc(shift + c, sh);
  if (MODE == 2) { ldc(scale2 + c, sc2); ldc(shift2 + c, sh2); }
  for (; i < end; i += 256) {
    f32x4 y[V4], r[V4], z[V4];
    ldv_stream<V4>(Y + i * V, y);
#pragma unroll
    for (int k = 0; k < V4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) z[k][e] = fmaf(y[k][e], sc[k][e], sh[k][e]);
    if (MODE != 0) ldv_stream<V4>(R + i * V, r);
#pragma unroll
    for (int k = 0; k < V4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (MODE == 1) z[k][e] += r[k][e];
        if (MODE == 2) z[k][e] += fmaf(r[k][e], sc2[k][e], sh2[k][e]);
      }
    if (relu) {
#pragma unroll
      for (int k = 0; k < V4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) z[k][e] = fmaxf(z[k][e], 0.f);
    }
    stv<V4>(Z + i * V, z, true);
    if (maskbits) {
      // ReLU mask of the stored activation, 1 bit per element: element j of the tensor is bit j & 31 of word j >> 5, so item i
      // owns V bits of word (i * V) >> 5. The backward kernels read this (1/32 of the bytes) instead of re-reading the activation
      // just to test z > 0.
      unsigned v = 0;
#pragma unroll
      for (int k = 0; k < V4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) v |= (z[k][e] > 0.f) ? (1u << (4 * k + e)) : 0u;
      v <<= V * (threadIdx.x & (LPW - 1));
      v |= __shfl_xor(v, 1); v |= __shfl_xor(v, 2);
      if (LPW == 8) v |= __shfl_xor(v, 4);
      if ((threadIdx.x & (LPW - 1)) == 0) maskbits[(i * V) >> 5] = v;
    }
  }
}

// Items per block of the elementwise passes (span = 256 * items consecutive items per block, walked 256 at a time).
// More than one item per thread needs 256 % cv == 0 (cv = C/4 or C/8 channel vectors per row) so that the thread's channels
// are loop-invariant. Measured (tools/bn_bench.py): the forward passes are fastest with one item per thread (6.0-6.3 TB/s
// against 5.5-5.9 with four); the backward apply pass, which carries six coefficient vectors per thread, gains 15-20 % from
// four items per thread in bf16, and a few % for C >= 512 in fp32. R3M_BN_ITEMS overrides.
static inline int bn_span(int cv, int items) {
  const int force = R3M_ENV_INT("R3M_BN_ITEMS", 0);
  if (force > 0) items = force;
  if (cv > 256 || 256 % cv != 0) items = 1;
  return 256 * items;
}
// Channels per lane of every streaming pass: 8 for bf16 with C a multiple of 8, else 4. The launchers below and bn_debug_geometry
// (r3m_debug_bn_geometry) take the width, and the span each elementwise launch picks, from here.
static inline int bn_vec(int dt, int C) { return dt == DT_BF16 && C % 8 == 0 ? 8 : 4; }
static inline int fwd_span(int vec, int C) { return vec == 8 ? bn_span(C / 8, C >= 2048 ? 4 : 1) : bn_span(C / 4, 1); }
static inline int apply_span(int vec, int C) { return vec == 8 ? bn_span(C / 8, 4) : bn_span(C / 4, C >= 512 ? 4 : 1); }
static inline int span_grid(long long items, int span) { return ceil_div(items, span); }   // blocks of a span-wide elementwise launch
static inline long long bn_items(long long rows, int C, int vec) { return rows * C / vec; }  // 16-byte items (vec elements each) of [rows][C]
static inline int col_blocks(int C, int vec, int cpb) { return ceil_div(C / vec, cpb); }      // gridDim.y of the backward reduce launches

// dispatch a <T, V4> launch on the storage type and the width bn_vec picked
#define BN_DISPATCH(dt, vec, NAME, ...)                                                   \
  do {                                                                                    \
    if ((dt) == DT_BF16 && (vec) == 8) { typedef bf16_t T; constexpr int V4 = 2; __VA_ARGS__; } \
    else if ((dt) == DT_BF16) { typedef bf16_t T; constexpr int V4 = 1; __VA_ARGS__; }    \
    else if ((dt) == DT_F32) { typedef float T; constexpr int V4 = 1; __VA_ARGS__; }      \
    else { set_last_error(NAME ": unknown dtype %d", (int)(dt)); return 1; }              \
  } while (0)

int launch_bn_act_fwd(const void* Y, const BnCoef& K, const void* R, const BnCoef* K2, void* Z, long long rows, int C, int relu,
                      unsigned* maskbits, int dt, hipStream_t s) {
  R3M_REQUIRE(is_pow2(C) && C >= 4, "bn_act_fwd: C=%d must be a power of two >= 4", C);
  R3M_REQUIRE(!maskbits || (rows * C / 4) % 8 == 0, "bn_act_fwd: bit mask needs rows*C to be a multiple of 32");
  const int vec = bn_vec(dt, C), span = fwd_span(vec, C);
  const long long n = bn_items(rows, C, vec);
  BN_DISPATCH(dt, vec, "bn_act_fwd", {
    const auto kernel = (R && K2) ? bn_act_fwd_kernel<2, T, V4> : R ? bn_act_fwd_kernel<1, T, V4> : bn_act_fwd_kernel<0, T, V4>;
    hipLaunchKernelGGL(kernel, dim3(span_grid(n, span)), dim3(256), 0, s, static_cast<const T*>(Y), K.scale, K.shift,
                       static_cast<const T*>(R), K2 ? K2->scale : nullptr, K2 ? K2->shift : nullptr, static_cast<T*>(Z), n, C / vec - 1, relu,
                       maskbits, span);
  });
  return check_launch("bn_act_fwd");
}

// ---------------------------------------------------------------------------------------------------------
// BatchNorm backward:  g = dZ * [z > 0],  yhat = (y - mean) * invstd.
//   pass 1: per-channel  sum(g)  and  sum(g * yhat);
//   pass 2: dY = scale * (g - c1 - yhat * c2)       (c1 = mean(g), c2 = mean(g*yhat); both 0 in eval mode).
// The ReLU mask is read as bits (Zbits, 1 per element, written by bn_act_fwd_kernel), or from the saved activation (Zmask, 4-wide
// only: residual blocks, where z also depends on the identity branch), or recomputed from y with the very same fmaf the forward
// used (no extra read).
// NB = 2 serves the TWO BatchNorms of a downsample block's tail in one launch (round 5). out = relu(bn3(y3) + bn_d(yd)): both
// BatchNorms see the same masked gradient g = dOut * [out > 0], so the stand-alone passes read dOut and the mask bits twice. Here they
// are read once: 20 instead of 24 bytes per element in pass 2 in fp32 (10 / 12 in bf16). Same arithmetic per element, block geometry
// and summation order as two NB = 1 launches (bit-identical results). The mask comes as bits: block outputs always have them.
// ---------------------------------------------------------------------------------------------------------
// g = dz where the forward's output was positive, else 0; the source is picked per vector, outside the per-element loops
template <class T, int V4, bool BITS_ONLY>
__device__ __forceinline__ void relu_grad(const T* __restrict__ Zmask, const unsigned* __restrict__ Zbits, long long off,
                                          const f32x4 (&dz)[V4], const f32x4 (&y)[V4], const f32x4 (&sc)[V4], const f32x4 (&sh)[V4],
                                          f32x4 (&g)[V4]) {
  constexpr int V = 4 * V4;
  if (BITS_ONLY || Zbits) {
    const unsigned nb = (Zbits[off >> 5] >> (off & 31)) & ((1u << V) - 1);
#pragma unroll
    for (int k = 0; k < V4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) g[k][e] = ((nb >> (4 * k + e)) & 1u) ? dz[k][e] : 0.f;
  } else if (V4 == 1 && Zmask) {
    const f32x4 z = ld4t(Zmask + off);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[0][e] = z[e] > 0.f ? dz[0][e] : 0.f;
  } else {
#pragma unroll
    for (int k = 0; k < V4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) g[k][e] = fmaf(y[k][e], sc[k][e], sh[k][e]) > 0.f ? dz[k][e] : 0.f;
  }
}

// pass 1. Work split: a block owns rows_per_block consecutive rows x up to 256 channel vectors (1024 / 2048 channels); each thread
// keeps its V channels' sums in registers. NB = 2: sum(g) is common, sum(g yhat) per BatchNorm; two partial sets [rows][2][C], the
// second `set_stride` floats behind the first.
template <class T, int V4, int NB>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dZ, const T* __restrict__ Zmask,
                                                             const unsigned* __restrict__ Zbits, const T* __restrict__ YA, BnCoef A,
                                                             const T* __restrict__ YB, BnCoef B, float* __restrict__ partials,
                                                             long long set_stride, long long rows, int C, int cpb, int rows_per_block) {
  constexpr int V = 4 * V4;
  __shared__ f32x4 red[(1 + NB) * V4][256];   // s1, then s2 of each BatchNorm, V4 vectors each
  const int tcol = threadIdx.x % cpb, trow = threadIdx.x / cpb;
  const int rpp = 256 / cpb;
  const int c = (blockIdx.y * cpb + tcol) * V;
  const long long r_begin = (long long)BN_BID(2) * rows_per_block;
  long long r_end = r_begin + rows_per_block;
  if (r_end > rows) r_end = rows;
  f32x4 sc[V4], sh[V4], mu[NB][V4], is[NB][V4], s1[V4], s2[NB][V4];
  if (NB == 1) { ldc(A.scale + c, sc); ldc(A.shift + c, sh); }
  ldc(A.mean + c, mu[0]); ldc(A.invstd + c, is[0]);
  if (NB == 2) { ldc(B.mean + c, mu[NB - 1]); ldc(B.invstd + c, is[NB - 1]); }
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    s1[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < NB; ++b) s2[b][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (long long r = r_begin + trow; r < r_end; r += rpp) {
    const long long off = r * C + c;
    f32x4 y[NB][V4], dz[V4], g[V4];
    ldv_stream<V4>(YA + off, y[0]);
    if (NB == 2) ldv_stream<V4>(YB + off, y[NB - 1]);
    ldv_stream<V4>(dZ + off, dz);
    relu_grad<T, V4, NB == 2>(Zmask, Zbits, off, dz, y[0], sc, sh, g);
#pragma unroll
    for (int k = 0; k < V4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s1[k][e] += g[k][e];
#pragma unroll
        for (int b = 0; b < NB; ++b) s2[b][k][e] = fmaf(g[k][e], (y[b][k][e] - mu[b][k][e]) * is[b][k][e], s2[b][k][e]);
      }
  }
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    red[k][threadIdx.x] = s1[k];
#pragma unroll
    for (int b = 0; b < NB; ++b) red[(1 + b) * V4 + k][threadIdx.x] = s2[b][k];
  }
  __syncthreads();
  if (trow == 0) {
    for (int j = 1; j < rpp; ++j) {
#pragma unroll
      for (int k = 0; k < V4; ++k) {
        s1[k] += red[k][j * cpb + tcol];
#pragma unroll
        for (int b = 0; b < NB; ++b) s2[b][k] += red[(1 + b) * V4 + k][j * cpb + tcol];
      }
    }
    float* p1 = partials + ((long long)BN_BID(2) * 2 + 0) * C + c;
    float* p2 = partials + ((long long)BN_BID(2) * 2 + 1) * C + c;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int k = 0; k < V4; ++k) {
        st4(p1 + b * set_stride + 4 * k, s1[k]);
        st4(p2 + b * set_stride + 4 * k, s2[b][k]);
      }
  }
}

// cpb: channel vectors per block, rpp (optional): rows a block reads per pass, rpb: rows per block, nblk: blocks = partial rows
static inline void bwd_geometry(long long rows, int C, int vec, int* cpb, int* rpb, int* nblk, int* rpp_out = nullptr) {
  const int cv = C / vec;
  *cpb = cv < 256 ? cv : 256;
  const int rpp = 256 / *cpb;
  if (rpp_out) *rpp_out = rpp;
  *rpb = 32 * rpp;
  *nblk = ceil_div(rows, *rpb);
}

int bn_bwd_partial_rows(long long rows, int C, int dt) {
  int cpb, rpb, nblk;
  bwd_geometry(rows, C, bn_vec(dt, C), &cpb, &rpb, &nblk);
  return nblk;
}

template <class T, int V4, int NB>
static void run_bn_bwd_reduce(const void* dZ, const void* Zmask, const unsigned* Zbits, const void* YA, const BnCoef& A, const void* YB,
                              const BnCoef& B, float* partials, long long set_stride, long long rows, int C, hipStream_t s) {
  int cpb, rpb, nblk;
  bwd_geometry(rows, C, 4 * V4, &cpb, &rpb, &nblk);
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, V4, NB>), dim3(nblk, col_blocks(C, 4 * V4, cpb)), dim3(256), 0, s, static_cast<const T*>(dZ),
                     static_cast<const T*>(Zmask), Zbits, static_cast<const T*>(YA), A, static_cast<const T*>(YB), B, partials, set_stride,
                     rows, C, cpb, rpb);
}

static int launch_bn_bwd_reduce(const void* dZ, const void* Zmask, const unsigned* Zbits, const void* Y, const BnCoef& A, float* partials,
                                long long rows, int C, int dt, hipStream_t s) {
  R3M_REQUIRE(is_pow2(C) && C >= 4, "bn_bwd_reduce: C=%d must be a power of two >= 4", C);
  R3M_REQUIRE(!Zmask || bn_vec(dt, C) == 4, "bn_bwd_reduce(bf16): pass the 1-bit mask (zbits) or no mask; a bf16 zmask tensor is not supported");
  BN_DISPATCH(dt, bn_vec(dt, C), "bn_bwd_reduce", (run_bn_bwd_reduce<T, V4, 1>(dZ, Zmask, Zbits, Y, A, nullptr, A, partials, 0, rows, C, s)));
  return check_launch("bn_bwd_reduce");
}

__global__ __launch_bounds__(64 * SG) void bn_bwd_finalize_kernel(const double* __restrict__ acc, int S, double inv_count,
                                                               int use_batch_stats, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, float* __restrict__ c1,
                                                               float* __restrict__ c2, int accumulate, int C,
                                                               const float* __restrict__ second_sum_scale) {
  int c;
  double sg, sgy;
  if (!slice_totals(acc, S, C, &c, &sg, &sgy)) return;
  if (second_sum_scale) sgy *= (double)second_sum_scale[c];    // EPI_BNRED partials carry sum(g (y - mean)): x invstd = sum(g yhat)
  const float db = (float)sg, dg = (float)sgy;
  dbeta[c] = accumulate ? dbeta[c] + db : db;
  dgamma[c] = accumulate ? dgamma[c] + dg : dg;
  c1[c] = use_batch_stats ? (float)(sg * inv_count) : 0.f;
  c2[c] = use_batch_stats ? (float)(sgy * inv_count) : 0.f;
}

static int launch_bn_bwd_finalize_rows(const double* acc, int stat_rows, long long count, int use_batch_stats, const BnBwdOut& o, int C,
                                       hipStream_t s, const float* second_sum_scale) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(C, 64)), dim3(64 * SG), 0, s, acc, reduce_slices(stat_rows, C),
                     1.0 / (double)count, use_batch_stats, o.dgamma, o.dbeta, o.c1, o.c2, o.accumulate, C, second_sum_scale);
  return check_launch("bn_bwd_finalize");
}

int bn_bwd_combine(const float* partial, int prow, long long count, int use_batch_stats, const BnBwdOut& o, const float* second_sum_scale,
                   int C, double* acc, hipStream_t s) {
  TRY(launch_bn_stats_reduce(partial, prow, C, acc, s));
  return launch_bn_bwd_finalize_rows(acc, prow, count, use_batch_stats, o, C, s, second_sum_scale);
}

// one BatchNorm's pass-2 coefficients of a thread's V channels
template <int V4>
struct BnApplyRegs {
  f32x4 sc[V4], mu[V4], is[V4], k1[V4], k2[V4];
  __device__ __forceinline__ void load(const BnCoef& K, int c) {
    ldc(K.scale + c, sc); ldc(K.mean + c, mu); ldc(K.invstd + c, is); ldc(K.c1 + c, k1); ldc(K.c2 + c, k2);
  }
  __device__ __forceinline__ void dy(const f32x4 (&y)[V4], const f32x4 (&g)[V4], f32x4 (&o)[V4]) const {
#pragma unroll
    for (int k = 0; k < V4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float yh = (y[k][e] - mu[k][e]) * is[k][e];
        o[k][e] = sc[k][e] * (g[k][e] - k1[k][e] - yh * k2[k][e]);
      }
  }
};

// pass 2. NB = 2 is bits-only and loads no `shift`.
template <class T, int V4, int NB>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dZ, const T* __restrict__ Zmask,
                                                            const unsigned* __restrict__ Zbits, const T* __restrict__ YA, BnCoef A,
                                                            T* __restrict__ dYA, const T* __restrict__ YB, BnCoef B, T* __restrict__ dYB,
                                                            long long n, int cvmask, int span) {
  constexpr int V = 4 * V4;
  long long i = (long long)BN_BID(4) * span + threadIdx.x;   // span consecutive items per block, see bn_act_fwd_kernel
  if (i >= n) return;
  const long long end = min((long long)(BN_BID(4) + 1) * span, n);
  const int c = ((int)(i & cvmask)) * V;
  BnApplyRegs<V4> a, b;
  f32x4 sh[V4];
  a.load(A, c);
  if (NB == 1) ldc(A.shift + c, sh);
  if (NB == 2) b.load(B, c);
  for (; i < end; i += 256) {
    f32x4 ya[V4], yb[V4], dz[V4], g[V4], o[V4];
    ldv_stream<V4>(YA + i * V, ya);
    if (NB == 2) ldv_stream<V4>(YB + i * V, yb);
    ldv_stream<V4>(dZ + i * V, dz);
    relu_grad<T, V4, NB == 2>(Zmask, Zbits, i * V, dz, ya, a.sc, sh, g);
    a.dy(ya, g, o);
    stv<V4>(dYA + i * V, o, true);
    if (NB == 2) {
      b.dy(yb, g, o);
      stv<V4>(dYB + i * V, o, true);
    }
  }
}

template <class T, int V4, int NB>
static void run_bn_bwd_apply(const void* dZ, const void* Zmask, const unsigned* Zbits, const void* YA, const BnCoef& A, void* dYA,
                             const void* YB, const BnCoef& B, void* dYB, long long rows, int C, hipStream_t s) {
  const int span = apply_span(4 * V4, C);
  const long long n = bn_items(rows, C, 4 * V4);
  hipLaunchKernelGGL((bn_bwd_apply_kernel<T, V4, NB>), dim3(span_grid(n, span)), dim3(256), 0, s, static_cast<const T*>(dZ),
                     static_cast<const T*>(Zmask), Zbits, static_cast<const T*>(YA), A, static_cast<T*>(dYA), static_cast<const T*>(YB), B,
                     static_cast<T*>(dYB), n, C / (4 * V4) - 1, span);
}

static int launch_bn_bwd_apply(const void* dZ, const void* Zmask, const unsigned* Zbits, const void* Y, const BnCoef& A, void* dY,
                               long long rows, int C, int dt, hipStream_t s) {
  R3M_REQUIRE(is_pow2(C) && C >= 4, "bn_bwd_apply: C=%d must be a power of two >= 4", C);
  BN_DISPATCH(dt, Zmask ? 4 : bn_vec(dt, C), "bn_bwd_apply",   // a Zmask source is 4-wide; launch_bn_bwd_reduce has refused it for bf16 by now
              (run_bn_bwd_apply<T, V4, 1>(dZ, Zmask, Zbits, Y, A, dY, nullptr, A, nullptr, rows, C, s)));
  return check_launch("bn_bwd_apply");
}

static int launch_bn_bwd_reduce2(const void* dZ, const unsigned* Zbits, const void* YA, const BnCoef& A, const void* YB, const BnCoef& B,
                                 float* partials, long long set_stride, long long rows, int C, int dt, hipStream_t s) {
  R3M_REQUIRE(is_pow2(C) && bn_vec(dt, C) == 8 && Zbits, "bn_bwd_reduce2: bf16 plans with mask bits only (C=%d dtype=%d)", C, dt);
  R3M_REQUIRE((long long)bn_bwd_partial_rows(rows, C, dt) * 2 * C <= set_stride, "bn_bwd_reduce2: partial sets overlap");
  run_bn_bwd_reduce<bf16_t, 2, 2>(dZ, nullptr, Zbits, YA, A, YB, B, partials, set_stride, rows, C, s);
  return check_launch("bn_bwd_reduce2");
}

static int launch_bn_bwd_apply2(const void* dZ, const unsigned* Zbits, const void* YA, const BnCoef& A, void* dYA, const void* YB,
                                const BnCoef& B, void* dYB, long long rows, int C, int dt, hipStream_t s) {
  R3M_REQUIRE(is_pow2(C) && C >= 8 && Zbits, "bn_bwd_apply2: C=%d must be a power of two >= 8 and the mask must come as bits", C);
  if (bn_vec(dt, C) == 8) {
    run_bn_bwd_apply<bf16_t, 2, 2>(dZ, nullptr, Zbits, YA, A, dYA, YB, B, dYB, rows, C, s);
  } else {
    R3M_REQUIRE(dt == DT_F32, "bn_bwd_apply2: dtype %d", dt);
    run_bn_bwd_apply<float, 1, 2>(dZ, nullptr, Zbits, YA, A, dYA, YB, B, dYB, rows, C, s);
  }
  return check_launch("bn_bwd_apply2");
}

// ---- the backward sequences (common.h): what the engine's step and the C ABI's bn_bwd entry points both run ----
// b's sums: its first pass into w.partial, or the `fused_rows` EPI_BNRED rows a dgrad left in `fused`, then the combine
static int bn_bwd_sums(const void* dZ, const void* Zmask, const unsigned* Zbits, const BnBwdSide& b, const float* fused, int fused_rows,
                       long long rows, int C, int use_batch_stats, const BnScratch& w, int dt, hipStream_t s) {
  if (fused_rows) return bn_bwd_combine(fused, fused_rows, rows, use_batch_stats, b.out, b.K.invstd, C, w.acc, s);
  TRY(launch_bn_bwd_reduce(dZ, Zmask, Zbits, b.Y, b.K, w.partial, rows, C, dt, s));
  return bn_bwd_combine(w.partial, bn_bwd_partial_rows(rows, C, dt), rows, use_batch_stats, b.out, nullptr, C, w.acc, s);
}

int bn_bwd(const void* dZ, const void* Zmask, const unsigned* Zbits, const BnBwdSide& b, const float* fused, int fused_rows, bool apply,
           long long rows, int C, int use_batch_stats, const BnScratch& w, int dt, hipStream_t s) {
  if (b.sums) TRY(bn_bwd_sums(dZ, Zmask, Zbits, b, fused, fused_rows, rows, C, use_batch_stats, w, dt, s));
  if (!apply) return 0;
  return launch_bn_bwd_apply(dZ, Zmask, Zbits, b.Y, b.apply_coef(), b.dY, rows, C, dt, s);
}

int bn_bwd_pair(const void* dZ, const unsigned* Zbits, const BnBwdSide& a, const BnBwdSide& b, const float* fused_a, int fused_rows_a,
                bool apply, long long set_stride, long long rows, int C, int use_batch_stats, const BnScratch& w, int dt, hipStream_t s) {
  if (!fused_rows_a && bn_vec(dt, C) == 8) {
    // both first passes are stand-alone and the joint kernel exists (bf16, C a multiple of 8): one launch, two partial sets, then the
    // two combines one after the other (one accumulator)
    const int prow = bn_bwd_partial_rows(rows, C, dt);
    TRY(launch_bn_bwd_reduce2(dZ, Zbits, a.Y, a.K, b.Y, b.K, w.partial, set_stride, rows, C, dt, s));
    if (a.sums) TRY(bn_bwd_combine(w.partial, prow, rows, use_batch_stats, a.out, nullptr, C, w.acc, s));
    if (b.sums) TRY(bn_bwd_combine(w.partial + set_stride, prow, rows, use_batch_stats, b.out, nullptr, C, w.acc, s));
  } else {
    if (a.sums) TRY(bn_bwd_sums(dZ, nullptr, Zbits, a, fused_a, fused_rows_a, rows, C, use_batch_stats, w, dt, s));
    if (b.sums) TRY(bn_bwd_sums(dZ, nullptr, Zbits, b, nullptr, 0, rows, C, use_batch_stats, w, dt, s));
  }
  if (!apply) return 0;
  return launch_bn_bwd_apply2(dZ, Zbits, a.Y, a.apply_coef(), a.dY, b.Y, b.apply_coef(), b.dY, rows, C, dt, s);
}

// What the launchers above pick for a [rows][C] tensor, without launching anything (r3m_debug_bn_geometry; the index names are in
// include/r3m_hip.h). Every figure comes from the helper the launcher itself calls.
int bn_debug_geometry(long long rows, int C, int dt, int* out, int cap) {
  R3M_REQUIRE(out && cap >= 14, "debug_bn_geometry: the output buffer needs 14 ints");
  R3M_REQUIRE(rows >= 1 && is_pow2(C) && C >= 4 && (dt == DT_F32 || dt == DT_BF16), "debug_bn_geometry: rows=%lld C=%d dtype=%d", rows, C, dt);
  const int vec = bn_vec(dt, C);
  int cpb, rpb, nblk, rpp;
  bwd_geometry(rows, C, vec, &cpb, &rpb, &nblk, &rpp);
  out[0] = vec;
  out[1] = fwd_span(vec, C);
  out[2] = span_grid(bn_items(rows, C, vec), out[1]);
  out[3] = vec;
  out[4] = rpb;
  out[5] = rpp;
  out[6] = col_blocks(C, vec, cpb);
  out[7] = nblk;
  out[8] = vec;
  out[9] = apply_span(vec, C);
  out[10] = span_grid(bn_items(rows, C, vec), out[9]);
  out[11] = reduce_slices(nblk, C);
  out[12] = reduce_slices(rows > 0x7fffffffLL ? 0x7fffffff : (int)rows, C);
  out[13] = slice_cap(C);
  return 0;
}

}  // namespace r3m
