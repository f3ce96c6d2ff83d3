// r3m_amd — the way out of (and the gradient's way back into) the encoder's private NHWC arena: stage outputs as fp32 NCHW tensors.
//
//   feature_export_kernel   : out[n][c][p] = (float) z[n][p][c]                       z fp32 / bf16 NHWC, out fp32 NCHW
//   feature_grad_add_kernel : g[n][p][c]   = store(load(g[n][p][c]) + d[n][c][p])      d fp32 NCHW, g fp32 / bf16 NHWC
//
// Reference semantics: the output of torchvision's layer1..layer4 (the convnet of models_r3m.py:44-52), i.e. z.permute(0,3,1,2)
// .float(), and autograd's sum of the gradients that reach that output. Both are HBM-bound passes: every element is read once and
// written once, no atomics, one writer per element.
//
// Per frame this is the transpose [HW][C] -> [C][HW] (and back). A block owns 64 channels x up to 64 pixels:
//   * channel side (NHWC): C is a multiple of 64, so every 16-byte access (4 fp32 / 8 bf16 channels) is aligned.
//   * pixel side (NCHW): the row of channel c starts at byte 4 * HW * c — 196 c for HW = 49 — so it is only dword-aligned. It is
//     accessed with dwords, consecutive lanes on consecutive (c, p) of the tile: one contiguous run of `valid` floats per channel,
//     and when the tile holds all pixels (HW <= 64) the 64 channels are ONE contiguous span of 64 * HW floats.
//   * pixel tiles are balanced: ceil(HW / 64) tiles of ceil(HW / tiles) pixels (HW = 49 -> one tile of 49, 196 -> 4 x 49,
//     784 -> 13 x 61, 3136 -> 49 x 64), so no frame ends in a nearly empty tile.
//   * HW = 1: NHWC and NCHW are the same bytes; the transpose is the identity and both operations run as plain 16-byte
//     element-wise kernels without LDS.
//
// LDS tile: float tile[64 channels][65] (16.6 KB static), element (c, p) at dword 65 c + p, bank (c + p) % 32 for the dword
// accesses used on both sides (ds_read_b32 / ds_write_b32: 32 banks, conflicts only inside a 32-lane half).
//   * channel side: a lane holds V = 4 (fp32) / 8 (bf16) channels of one pixel. A half wave is 32 / V lanes along the channels
//     (k) x V pixels (p): dword j of the lane goes to bank (V k + j + p) % 32 with k < 32 / V, p < V — V k + p runs through
//     0..31 exactly once: 0 conflicts. (In HBM the half wave covers V runs of 128 bytes, the two halves of a wave adjoining.)
//   * pixel side: 32 consecutive (c, p) of the tile. A half inside one row: 32 consecutive pixels, 0 conflicts. A half that
//     straddles rows c (pixels a..r-1) and c + 1 (pixels 0..b) of r pixels: (c, p) and (c + 1, p') share a bank when
//     p = p' + 1 (only possible for r <= 32) or p = p' + 33 (r >= 34, a row longer than the 32 banks wraps them). So rows of
//     33 pixels are conflict-free, rows of 34..64 pixels at most 2-way on the straddling halves (HW = 49: a half on pixels
//     40..48 of row c and 0..22 of row c + 1 has nine 2-way pairs, 40..48 against 7..15), and rows of r <= 32 pixels (maps of
//     at most 32 pixels) min(r, ceil(32 / r))-way, at most 6-way (r = 6).
// Streamed operands (z, the running gradient) use the read-once loads of bn_dev.h; the gradient is stored with the cached
// policy, the next kernel (the block's BatchNorm backward) reads it back.
#include "bn_dev.h"

namespace r3m {

constexpr int FEAT_C = 64;        // channels per tile
constexpr int FEAT_P = 64;        // pixels per tile, at most
constexpr int FEAT_LD = 65;       // dwords between the tile rows of two channels
constexpr int FEAT_THREADS = 256;

template <class T>
struct FeatVec { static constexpr int V = 4; };      // channels of one 16-byte access
template <>
struct FeatVec<bf16_t> { static constexpr int V = 8; };

static inline int feat_tiles(int HW) { return ceil_div(HW, FEAT_P); }
static inline int feat_tile_pixels(int HW) { return ceil_div(HW, feat_tiles(HW)); }

// channel side: the pixel (of the block's first pass) and the first channel of this thread; a pass of the block covers 4 V pixels
template <int V>
__device__ __forceinline__ void feat_lane(int* p, int* c) {
  constexpr int KH = 32 / V;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  *c = ((lane & (KH - 1)) + KH * (lane >> 5)) * V;
  *p = wave * V + ((lane / KH) & (V - 1));
}

template <class T>
__global__ __launch_bounds__(FEAT_THREADS) void feature_export_kernel(const T* __restrict__ z, float* __restrict__ out, int HW, int C,
                                                                       int tp) {
  constexpr int V = FeatVec<T>::V, V4 = V / 4, PASS = 4 * V, NP = FEAT_P / PASS;
  __shared__ float tile[FEAT_C * FEAT_LD];
  const int p0 = blockIdx.x * tp, c0 = blockIdx.y * FEAT_C;
  const int valid = min(tp, HW - p0);
  if (valid <= 0) return;
  const T* zf = z + ((long long)blockIdx.z * HW + p0) * C + c0;
  float* of = out + ((long long)blockIdx.z * C + c0) * HW + p0;
  int pl, cl;
  feat_lane<V>(&pl, &cl);
  f32x4 v[NP][V4];
#pragma unroll
  for (int i = 0; i < NP; ++i)
    if (pl + i * PASS < valid) ldv_stream<V4>(zf + (long long)(pl + i * PASS) * C + cl, v[i]);
#pragma unroll
  for (int i = 0; i < NP; ++i)
    if (pl + i * PASS < valid) {
#pragma unroll
      for (int j = 0; j < V; ++j) tile[(cl + j) * FEAT_LD + pl + i * PASS] = v[i][j / 4][j % 4];
    }
  __syncthreads();
  // consecutive threads on consecutive (c, p) of the tile; (c, p) advances by 256 elements without a division per element
  const int dc = FEAT_THREADS / valid, dp = FEAT_THREADS - dc * valid;
  int c = threadIdx.x / valid, p = threadIdx.x - c * valid;
  for (; c < FEAT_C; c += dc) {
    of[(long long)c * HW + p] = tile[c * FEAT_LD + p];
    p += dp;
    if (p >= valid) { p -= valid; ++c; }
  }
}

template <class T>
__global__ __launch_bounds__(FEAT_THREADS) void feature_grad_add_kernel(const float* __restrict__ d, T* __restrict__ g, int HW, int C,
                                                                         int tp) {
  constexpr int V = FeatVec<T>::V, V4 = V / 4, PASS = 4 * V, NP = FEAT_P / PASS;
  __shared__ float tile[FEAT_C * FEAT_LD];
  const int p0 = blockIdx.x * tp, c0 = blockIdx.y * FEAT_C;
  const int valid = min(tp, HW - p0);
  if (valid <= 0) return;
  const float* df = d + ((long long)blockIdx.z * C + c0) * HW + p0;
  T* gf = g + ((long long)blockIdx.z * HW + p0) * C + c0;
  int pl, cl;
  feat_lane<V>(&pl, &cl);
  f32x4 v[NP][V4];               // the running gradient: in flight while the tile fills
#pragma unroll
  for (int i = 0; i < NP; ++i)
    if (pl + i * PASS < valid) ldv_stream<V4>(gf + (long long)(pl + i * PASS) * C + cl, v[i]);
  const int dc = FEAT_THREADS / valid, dp = FEAT_THREADS - dc * valid;
  int c = threadIdx.x / valid, p = threadIdx.x - c * valid;
  for (; c < FEAT_C; c += dc) {
    tile[c * FEAT_LD + p] = df[(long long)c * HW + p];
    p += dp;
    if (p >= valid) { p -= valid; ++c; }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NP; ++i)
    if (pl + i * PASS < valid) {
#pragma unroll
      for (int j = 0; j < V; ++j) v[i][j / 4][j % 4] += tile[(cl + j) * FEAT_LD + pl + i * PASS];
      stv<V4>(gf + (long long)(pl + i * PASS) * C + cl, v[i], false);
    }
}

// HW = 1: [N][1][C] and [N][C][1] are the same layout
template <class T>
__global__ __launch_bounds__(FEAT_THREADS) void feature_export_flat_kernel(const T* __restrict__ z, float* __restrict__ out, long long nvec) {
  constexpr int V = FeatVec<T>::V, V4 = V / 4;
  const long long i = (long long)blockIdx.x * FEAT_THREADS + threadIdx.x;
  if (i >= nvec) return;
  f32x4 v[V4];
  ldv_stream<V4>(z + i * V, v);
#pragma unroll
  for (int k = 0; k < V4; ++k) st4(out + i * V + 4 * k, v[k]);
}

template <class T>
__global__ __launch_bounds__(FEAT_THREADS) void feature_grad_add_flat_kernel(const float* __restrict__ d, T* __restrict__ g, long long nvec) {
  constexpr int V = FeatVec<T>::V, V4 = V / 4;
  const long long i = (long long)blockIdx.x * FEAT_THREADS + threadIdx.x;
  if (i >= nvec) return;
  f32x4 v[V4];
  ldv_stream<V4>(g + i * V, v);
#pragma unroll
  for (int k = 0; k < V4; ++k) v[k] += ld4(d + i * V + 4 * k);
  stv<V4>(g + i * V, v, false);
}

static int feat_check(const char* what, const void* nhwc, const void* nchw, int N, int H, int W, int C, int dt) {
  R3M_REQUIRE(dt == DT_F32 || dt == DT_BF16, "%s: dtype %d (0 = fp32, 1 = bf16)", what, dt);
  R3M_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: N=%d, H=%d, W=%d must all be >= 1", what, N, H, W);
  R3M_REQUIRE(C >= FEAT_C && C % FEAT_C == 0, "%s: C=%d must be a positive multiple of %d", what, C, FEAT_C);
  R3M_REQUIRE((long long)N * H * W * C <= 0x7fffffffLL && C / FEAT_C <= 65535 && N <= 65535,
              "%s: [%d,%d,%d,%d] is outside the supported range (fewer than 2^31 elements, N and C / %d at most 65535)", what, N, H, W, C,
              FEAT_C);
  R3M_REQUIRE(nhwc && nchw, "%s: null argument", what);
  // the NHWC side is always accessed 16 bytes at a time; the NCHW side only in the HW = 1 kernels
  R3M_REQUIRE(reinterpret_cast<uintptr_t>(nhwc) % 16 == 0 && (H * W > 1 || reinterpret_cast<uintptr_t>(nchw) % 16 == 0),
              "%s: the NHWC tensor (and, for H * W = 1, the NCHW tensor) must be 16-byte aligned", what);
  return 0;
}

int launch_feature_export(const void* z_nhwc, float* out_nchw, int N, int H, int W, int C, int dt, hipStream_t s) {
  if (int e = feat_check("feature_export", z_nhwc, out_nchw, N, H, W, C, dt)) return e;
  const int HW = H * W;
  DT_DISPATCH(dt, "feature_export", {
    if (HW == 1) {
      const long long nvec = (long long)N * C / FeatVec<T>::V;
      hipLaunchKernelGGL((feature_export_flat_kernel<T>), dim3(ceil_div(nvec, FEAT_THREADS)), dim3(FEAT_THREADS), 0, s,
                         static_cast<const T*>(z_nhwc), out_nchw, nvec);
    } else {
      hipLaunchKernelGGL((feature_export_kernel<T>), dim3(feat_tiles(HW), C / FEAT_C, N), dim3(FEAT_THREADS), 0, s,
                         static_cast<const T*>(z_nhwc), out_nchw, HW, C, feat_tile_pixels(HW));
    }
  });
  return check_launch("feature_export");
}

int launch_feature_grad_add(const float* d_nchw, void* g_nhwc, int N, int H, int W, int C, int dt, hipStream_t s) {
  if (int e = feat_check("feature_grad_add", g_nhwc, d_nchw, N, H, W, C, dt)) return e;
  const int HW = H * W;
  DT_DISPATCH(dt, "feature_grad_add", {
    if (HW == 1) {
      const long long nvec = (long long)N * C / FeatVec<T>::V;
      hipLaunchKernelGGL((feature_grad_add_flat_kernel<T>), dim3(ceil_div(nvec, FEAT_THREADS)), dim3(FEAT_THREADS), 0, s, d_nchw,
                         static_cast<T*>(g_nhwc), nvec);
    } else {
      hipLaunchKernelGGL((feature_grad_add_kernel<T>), dim3(feat_tiles(HW), C / FEAT_C, N), dim3(FEAT_THREADS), 0, s, d_nchw,
                         static_cast<T*>(g_nhwc), HW, C, feat_tile_pixels(HW));
    }
  });
  return check_launch("feature_grad_add");
}

}  // namespace r3m
