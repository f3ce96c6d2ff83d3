// r3m_amd — what the stem kernels share (stem.hip: fp32 at 224 x 224, stem_bf16.hip: the bf16 MFMA at 224 x 224, stem_gen.hip: any
// H x W, stem_dgrad.hip: the 224 x 224 input gradient): the K layout and workspace constants, the 224 pre-pass body, the fp32-MFMA
// forward and weight-gradient pieces, the input gradient's GEMM step, and the host tail of every weight gradient. Each kernel keeps
// its own staging (register prefetch, DMA ring or plain copy: DESIGN.md §4.5); what it computes on the staged rows is here, once.
#pragma once
#include "common.h"
#include "conv_dev.h"
#include "augment_dev.h"
#include <cstring>

namespace r3m {

// ---- constants ----
// Geometry trick: for a fixed kernel row kh the 7 x 3 (kw, c) taps of one output pixel are 21 CONSECUTIVE elements of an interleaved
// [x][c] image row, starting at 6*ox. The fp32 MFMA walks K as 7 x 22 (j = 21 multiplies a zero weight): 154 instead of 147 MACs.
constexpr int ST_K = 154;               // 7 kernel rows x 22
constexpr int ST_KS = 155;              // LDS weight row stride (odd: conflict-free fragment reads)
constexpr int ST_DW = 160;              // fp32-MFMA weight-gradient partial: [64][160], five k tiles of 32 (columns 154.. unused)
constexpr int ST_DW16 = 224;            // bf16-MFMA weight-gradient partial: [64][7][32] (taps 21.. unused)
// persistent weight-gradient blocks. fp32: the kernel holds 130 VGPRs + 48 AGPRs -> TWO blocks per CU; 768 blocks (round 1) ran as
// one and a half rounds of resident blocks with equal work each, i.e. the last third of the time at half occupancy
#ifndef R3M_STEM_WG_BLOCKS
#define R3M_STEM_WG_BLOCKS 512
#endif
constexpr int STEM_WG_BLOCKS = R3M_STEM_WG_BLOCKS;   // stem.hip and stem_gen.hip (one workspace serves both)
constexpr int STEM_WG16_BLOCKS = 768;                // stem_bf16.hip
// workspace of a weight gradient: one partial per block, then the reduced image the unpack kernel reads
constexpr size_t stem_ws_partials(int blocks, int row) { return (size_t)blocks * 64 * row; }
constexpr size_t stem_ws_floats(int blocks, int row) { return stem_ws_partials(blocks, row) + 64 * row; }
constexpr int SD_WH = 1056;             // input gradient: LDS floats per (kh, channel half): 32 channels x 32 columns + 32 (the two
                                        // halves of a wave read banks 32 apart: conflict-free)
constexpr int SD_WK = 2 * SD_WH;        // per kernel row

// ---- pre-passes: frames 0..255 -> normalised, channel-interleaved rows (the reference's (x/255 - mean)/std with IEEE divisions,
// done once per frame). A value source hands out one frame's reader: `src.frame(f)(c, iy, ix)` is channel c of pixel (iy, ix). ----
struct StemFrames {                     // NCHW fp32 frames [F,3,224,224]
  const float* x;
  struct Frame {
    const float* x;
    long long f;
    __device__ __forceinline__ float operator()(int c, int iy, int ix) const { return x[((f * 3 + c) * 224 + iy) * 224 + ix]; }
  };
  __device__ __forceinline__ Frame frame(long long f) const { return Frame{x, f}; }
};
// the RAW clips through their crop boxes (rc / rctraj on the GPU): the cropped fp32 frames [F,3,224,224] are
// never written — one gather-bilinear pass from uint8 (or float) straight into the normalised image
template <class T>
struct StemCrop {
  const T* raw;
  const int* boxes;
  int Hi, Wi, fpb;
  struct Frame {
    const T* raw;
    long long f;
    int Hi, Wi, top, left, bh, bw;
    __device__ __forceinline__ float operator()(int c, int iy, int ix) const {
      return bilinear_sample(raw + (f * 3 + c) * (long long)Hi * Wi, Wi, top, left, bh, bw, iy, ix, 0, 0, 224, 224);
    }
  };
  __device__ __forceinline__ Frame frame(long long f) const {
    const int* b = boxes + (f / fpb) * 4;
    return Frame{raw, f, Hi, Wi, b[0], b[1], b[2], b[3]};
  }
  StemCrop(const FrameSource& s) : raw(static_cast<const T*>(s.frames)), boxes(s.boxes), Hi(s.Hi), Wi(s.Wi), fpb(s.frames_per_box) {}
};

// plain fp32 image xn[f][iy][ix*3 + c] of 224 x 224 frames (stem.hip; the general stem's pre-pass, with run-time H x W, is stem_gen.hip's own)
template <class Src>
__global__ __launch_bounds__(256) void stem_prep_kernel(const Src src, float* __restrict__ xn, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // one thread per (f, iy, ix)
  if (i >= total) return;
  const int ix = (int)(i % 224);
  const long long t = i / 224;
  const int iy = (int)(t % 224);
  const auto px = src.frame(t / 224);
  float* o = xn + i * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = stem_normalize(px(c, iy, ix), c);
}
template <class Src>
inline int launch_stem_prep_body(const Src& src, float* xn, int F, hipStream_t s, const char* what) {
  const long long total = (long long)F * 224 * 224;
  hipLaunchKernelGGL((stem_prep_kernel<Src>), dim3(ceil_div(total, 256)), dim3(256), 0, s, src, xn, total);
  return check_launch(what);
}

// ---- forward on the fp32 MFMA: 256 x 64 tiles, wave w owns pixels 64 w .. 64 w + 63 of the tile, lane = (lrow, lh) ----
// LDS weight image wl[n * ST_KS + kh * 22 + j] = w[n][kh][j] (j < 21), 0 (j = 21). Its fill is the one piece the two forward kernels
// do NOT share: stem.hip unrolls it over 4 threads per output channel, stem_gen.hip walks one flat loop (and rounds to bf16 for
// bf16 plans); either form in the other kernel changes that kernel's registers.
__device__ __forceinline__ void stem_fwd_b_base(int (&b_base)[2], int lrow, int lh) {
#pragma unroll
  for (int t = 0; t < 2; ++t) b_base[t] = (t * 32 + lrow) * ST_KS + lh;
}
// one kernel row kh of the K loop: 11 steps of v_mfma_f32_32x32x2_f32, A from the two patch rows pa0 / pa1 of this lane's pixels
__device__ __forceinline__ void stem_fwd_krow(const float* pa0, const float* pa1, const float* wl, const int (&b_base)[2], int kh,
                                              f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int jp = 0; jp < 11; ++jp) {
    const float a[2] = {pa0[2 * jp], pa1[2 * jp]};
    float b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) b[t] = wl[b_base[t] + kh * 22 + 2 * jp];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
  }
}
// conv1's output as the shared epilogue sees it: [F * Ho * Wo, 64], dense rows
inline GatherGemmParams stem_fwd_params(void* y, float* stats, int dt, int F, int Ho, int Wo) {
  GatherGemmParams p;
  memset(&p, 0, sizeof p);
  p.out = static_cast<float*>(y); p.stats = stats; p.dtype = dt;
  p.M = F * Ho * Wo; p.Nc = 64; p.os = 1;
  p.Hg = Ho; p.Wg = Wo; p.Ho = Ho; p.Wo = Wo;
  return p;
}
// profiling bracket of a stem GEMM over M output pixels (closed by prof_end): 2 M 64 147 flops, the image read + M x 64 elements; the
// forward (KC_GEMM_NARROW) also reads conv1's fp32 weights and, with `stats`, writes one statistics row per 256 output pixels
inline void stem_prof_begin(int kclass, int M, double image_bytes, int dt, hipStream_t s, const float* stats = nullptr) {
  prof_begin(kclass, 2.0 * (double)M * 64.0 * 147.0, M, 64, 147, 1, s);
  double b = image_bytes + (double)M * 64 * (dt == DT_BF16 ? 2 : 4);
  if (kclass == KC_GEMM_NARROW) b += 4.0 * 64 * 147 + (stats ? 8.0 * ceil_div(M, 256) * 64 : 0.0);
  prof_bytes(b);
}

// ---- weight gradient on the fp32 MFMA: dW[co][kh*22 + j] partial of one block = sum over its output image rows of
// dY[m][co] * patch(m, kh, j). One output row per iteration: the dY row [pixel][64] and 7 input rows at stride PSW in LDS, per-lane
// bases plus immediates (pixel step = 6 floats of the interleaved row). Waves: 2 (co halves) x 2 (k tiles {0,1,2} / {3,4}). ----
struct StemWgLane {
  int wi, wj, lrow, lh, jt0, a_base;
  int b_base[3];
};
// patch row stride: PSW_CT, or psw when PSW_CT = 0
template <int PSW_CT>
__device__ __forceinline__ StemWgLane stem_wg_lane(int psw) {
  const int PSW = PSW_CT ? PSW_CT : psw;
  StemWgLane L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  L.wi = wave >> 1; L.wj = wave & 1;
  L.lrow = lane & 31; L.lh = lane >> 5;
  L.jt0 = L.wj ? 3 : 0;
  L.a_base = L.lh * 64 + L.wi * 32 + L.lrow;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    int j = (L.jt0 + t) * 32 + L.lrow;
    if (j >= ST_K) j = 0;                       // columns 154..159 (and the unused third tile of the second wave column)
    const int kh = j / 22, jj = j - kh * 22;
    L.b_base[t] = kh * PSW + jj + 6 * L.lh;
  }
  return L;
}
// one pixel pair q of the staged row against this wave's NT k tiles (dys and patch: disjoint LDS regions, read only)
template <int NT>
__device__ __forceinline__ void stem_wg_pair(const float* __restrict__ dys, const float* __restrict__ patch, const StemWgLane& L, int q,
                                             f32x16 (&acc)[3]) {
  const float a = dys[L.a_base + q * 128];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, patch[L.b_base[t] + q * 12], acc[t], 0, 0, 0);
}
template <int NT, int NP>
__device__ __forceinline__ void stem_wg_pairs(const float* __restrict__ dys, const float* __restrict__ patch, const StemWgLane& L,
                                              int npairs, f32x16 (&acc)[3]) {
  if constexpr (NP != 0) {
#pragma unroll
    for (int q = 0; q < NP; ++q) stem_wg_pair<NT>(dys, patch, L, q, acc);
  } else {
    for (int q = 0; q < npairs; ++q) stem_wg_pair<NT>(dys, patch, L, q, acc);
  }
}
// one staged row: two-level summation — `acc` covers the row's pixel pairs (NP of them, unrolled, or npairs when NP = 0), `tot`
// adds the rows: short fp32 chains
template <int NP>
__device__ __forceinline__ void stem_wg_row(const float* __restrict__ dys, const float* __restrict__ patch, const StemWgLane& L,
                                            int npairs, f32x16 (&tot)[3]) {
  f32x16 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  if (L.wj == 0) stem_wg_pairs<3, NP>(dys, patch, L, npairs, acc);
  else stem_wg_pairs<2, NP>(dys, patch, L, npairs, acc);
#pragma unroll
  for (int t = 0; t < 3; ++t) tot[t] += acc[t];
}
__device__ __forceinline__ void stem_wg_store(float* partial, const StemWgLane& L, const f32x16 (&tot)[3]) {
  float* out = partial + (long long)blockIdx.x * 64 * ST_DW;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (t == 2 && L.wj) continue;               // the second wave column owns k tiles 3 and 4 only
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = L.wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * L.lh;
      out[co * ST_DW + (L.jt0 + t) * 32 + L.lrow] = tot[t][r];
    }
  }
}

// host tail of every stem weight gradient: dw147[n][kh*21 + j] (+)= sum over the nb partials of ws of [n][kh * KROW + j]
template <int ROW, int KROW>
__global__ void stem_unpack_kernel(const float* __restrict__ dw, float* __restrict__ dw147, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 64 * 147) return;
  const int n = i / 147, k = i - n * 147;
  const int kh = k / 21, j = k - kh * 21;
  // (n * ROW + kh * KROW + j, in the association each parent kernel had: the bf16 partial is [n][7][32], the fp32 one [n][160])
  const float v = ROW % KROW == 0 ? dw[(n * (ROW / KROW) + kh) * KROW + j] : dw[n * ROW + kh * KROW + j];
  dw147[i] = accumulate ? dw147[i] + v : v;
}
template <int ROW, int KROW>
inline int stem_wgrad_finish(float* ws /* stem_ws_floats(blocks, ROW) */, int nb, int blocks, float* dw147, int accumulate,
                             hipStream_t s, const char* what) {
  float* dw = ws + stem_ws_partials(blocks, ROW);
  if (int e = launch_wgrad_reduce(ws, dw, 64 * ROW, nb, 0, s)) return e;
  hipLaunchKernelGGL((stem_unpack_kernel<ROW, KROW>), dim3(ceil_div(64 * 147, 256)), dim3(256), 0, s, dw, dw147, accumulate);
  return check_launch(what);
}

// ---- input gradient: per input row h, U[ox, (kw,c)] = sum_{kh: h+3-kh even, co} dZ[(h+3-kh)/2, ox, co] * W[co, kh, kw, c]
// (M = pixels of one dZ row, N = 21 (kw, c) columns padded to 32, K = (3 or 4 kh) x 64 co), then a col2im gather of U out of LDS ----
__device__ __forceinline__ f32x4 stem_load4(const float* p) { return ldg4(p); }
__device__ __forceinline__ f32x4 stem_load4(const bf16_t* p) {      // bf16 dZ is widened on load
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
               __uint_as_float(u.y & 0xffff0000u)};
}
// the NK = 3 (P = 0) or 4 (P = 1) kernel rows kh = (1 - P) + 2 kk that reach input rows of parity P: smem[kk][co half][co & 31][n]
template <int P>
__device__ __forceinline__ void stem_dgrad_weights(float* smem, const float* w) {
  constexpr int NK = P ? 4 : 3;
  for (int i = (int)threadIdx.x; i < NK * 64 * 32; i += 256) {
    const int n = i & 31, co = (i >> 5) & 63, kk = i >> 11;
    const int kh = (1 - P) + 2 * kk;
    smem[kk * SD_WK + (co >> 5) * SD_WH + (co & 31) * 32 + n] = n < 21 ? w[co * 147 + kh * 21 + n] : 0.f;
  }
}
// four of the 64 channels of one (kernel row, M tile): a = channels 4 j .. 4 j + 3 of this lane's half against
// B = W[co][kh][n = lane & 31] at wb[32 (co & 31)]; a and acc travel by value (by reference the 224 kernel spilled)
__device__ __forceinline__ f32x16 stem_dgrad_mfma4(f32x4 a, const float* wb, f32x16 acc) {
#pragma unroll
  for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], wb[32 * e], acc, 0, 0, 0);
  return acc;
}
// d(normalised)/d(frame value) of channel c: 1 / (255 std_c)
__device__ __forceinline__ float stem_dgrad_scale(int c) {
  return c == 0 ? 1.f / (255.f * 0.229f) : (c == 1 ? 1.f / (255.f * 0.224f) : 1.f / (255.f * 0.225f));
}

}  // namespace r3m
