// r3m_amd — input gradient of the stem: d/d(frames) of x/255 -> Normalize -> conv1 7x7/2 pad 3 (3 -> 64), the adjoint of what the
// forward runs (/root/reference/r3m/models/models_r3m.py:96-99 into torchvision's conv1). Pre-training never needs it (the
// engine's backward stops at the stem's weight gradient); a frozen encoder used as a differentiable reward / perceptual loss
// needs nothing else.
//
//   dX[n,c,h,w] = 1/(255 std_c) * sum_{co,kh,kw} W[co,kh,kw,c] * dZ[n, (h+3-kh)/2, (w+3-kw)/2, co]     (exact divisions, in range)
//
// dZ: conv1's output gradient, NHWC [F,112,112,64] fp32 or bf16 (what BatchNorm backward of the stem leaves in the plan); W: the
// fp32 master weights OHWI [64][7][7][3]; dX: fp32 NCHW [F,3,224,224]. fp32 accumulation throughout (bf16 dZ is widened on load).
//
// Form: the output channels are only 3, so a direct GEMM would leave the MFMA 3/32 busy. Instead, per input row h,
//     U[ox, (kw,c)] = sum_{kh: h+3-kh even, co} dZ[(h+3-kh)/2, ox, co] * W[co, kh, kw, c]
// is a GEMM with M = 112 pixels of one dZ row position, N = 21 (kw, c) columns (padded to 32) and K = (3 or 4 kh) x 64 co on
// v_mfma_f32_32x32x2_f32, and dX[h, w, c] = sum over the <= 4 kw with (w+3-kw) even of U[(w+3-kw)/2, kw, c] is a col2im gather of
// U out of LDS. Rows of one parity share their kh set: a block takes 8 rows of ONE parity (4 waves x 2 rows = 7 M tiles of 32 per
// wave, no padding on M), stages the 3 or 4 kernel rows of W it needs in LDS, and reads its A operands straight from dZ: per (kernel
// row, M tile) each lane loads the 32 consecutive channels it owns of one pixel (one whole cache line; a first version that walked
// the channels in 4-channel steps across all 7 tiles re-fetched every line 8 times and ran 11x slower than the stem forward),
// prefetched one tile ahead of the 32 MFMAs that consume it (B comes from LDS, one read per MFMA). The weight staging, that MFMA step,
// the bf16 widening and the per-channel scale are stem_dev.h's, shared with the general form (stem_gen.hip stem_dgrad_gen_kernel).
#include "stem_dev.h"

namespace r3m {

namespace {

constexpr int SD_U = 224 * 21;          // LDS floats of one wave's U (2 rows x 112 pixels x 21 columns)
constexpr int SD_LDS = 4 * SD_U > 4 * SD_WK ? 4 * SD_U : 4 * SD_WK;   // U aliases the weights (dead after the K loop)

template <int P, class T>
__device__ __forceinline__ void stem_dgrad_item(const T* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx,
                                                long long f, int g, int accumulate, float* smem) {
  constexpr int NK = P ? 4 : 3;          // kernel rows with h + 3 - kh even: kh = (1 - P) + 2 kk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lrow = lane & 31, lh = lane >> 5;
  stem_dgrad_weights<P>(smem, w);
  // this wave's two input rows: h_r = 2 (2q + r) + P, q = 4 g + wave (0..55)
  const int q = 4 * g + wave;
  int h_of[2];
  h_of[0] = 2 * (2 * q) + P;
  h_of[1] = 2 * (2 * q + 1) + P;
  // per M tile: this lane's pixel (row r, column ox)
  int row_r[7], ox_t[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int m = 32 * t + lrow;
    row_r[t] = m >= 112 ? 1 : 0;
    ox_t[t] = m - 112 * row_r[t];
  }
  // A of (kk, t): channels lh*32 .. lh*32+31 of this lane's pixel (oy, ox), oy = (h + 3 - kh) / 2 — one whole 128-byte line per
  // lane, read once; zero when oy leaves [0, 112)
  auto load_a = [&](f32x4* a, int kk, int t) __attribute__((always_inline)) {
    const int kh = (1 - P) + 2 * kk;
    const int oy = (h_of[row_r[t]] + 3 - kh) >> 1;
    const bool ok = (unsigned)oy < 112u;
    const T* src = dz + ((f * 112 + (ok ? oy : 0)) * 112 + ox_t[t]) * 64 + lh * 32;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = ok ? stem_load4(src + 4 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  f32x16 acc[7];
#pragma unroll
  for (int t = 0; t < 7; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  f32x4 cur[8], nxt[8];
  load_a(cur, 0, 0);
  __syncthreads();                       // weights staged
  for (int kk = 0; kk < NK; ++kk) {
    const float* wb = smem + kk * SD_WK + lh * SD_WH + lrow;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      if (t < 6) load_a(nxt, kk, t + 1);
      else if (kk + 1 < NK) load_a(nxt, kk + 1, 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[t] = stem_dgrad_mfma4(cur[j], wb + 128 * j, acc[t]);
#pragma unroll
      for (int j = 0; j < 8; ++j) cur[j] = nxt[j];
    }
  }
  __syncthreads();                       // every wave is done with the weights: U takes their place
  float* U = smem + wave * SD_U;
  if (lrow < 21) {
#pragma unroll
    for (int t = 0; t < 7; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;   // C/D row of register r
        U[m * 21 + lrow] = acc[t][r];
      }
  }
  __syncthreads();
  // col2im: lane l < 56 owns w = 4l .. 4l+3 of both rows and all three channels; kw runs over the parity (w + 1) & 1
  if (lane < 56) {
    const int w0 = 4 * lane;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const float* Ur = U + r * 112 * 21;
      const int h = h_of[r];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int wcol = w0 + j;
          float sum = 0.f;
#pragma unroll
          for (int kw = (j + 1) & 1; kw < 7; kw += 2) {      // (w0 even) parity of w + 1 == parity of j + 1
            const int ox = (wcol + 3 - kw) >> 1;
            if ((unsigned)ox < 112u) sum += Ur[ox * 21 + kw * 3 + c];
          }
          v[j] = sum * stem_dgrad_scale(c);
        }
        f32x4* o = reinterpret_cast<f32x4*>(dx + ((f * 3 + c) * 224 + h) * 224 + w0);
        if (accumulate) v += *o;
        *o = v;
      }
    }
  }
}

// one block per (frame, parity, group of 8 rows of that parity): F x 2 x 14 blocks; two waves per SIMD (the B values the compiler
// would otherwise keep in registers across the 7 tiles are re-read from LDS instead)
template <class T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void stem_dgrad_kernel(const T* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx,
                                                          int accumulate) {
  __shared__ __attribute__((aligned(16))) float smem[SD_LDS];
  const long long item = blockIdx.x;
  const long long f = item / 28;
  const int rem = (int)(item - f * 28);
  if (rem & 1) stem_dgrad_item<1, T>(dz, w, dx, f, rem >> 1, accumulate, smem);
  else stem_dgrad_item<0, T>(dz, w, dx, f, rem >> 1, accumulate, smem);
}

}  // namespace

int launch_stem_input_grad(const void* dz, int dt, const float* w147, float* dx, int F, int accumulate, hipStream_t s) {
  R3M_REQUIRE(F >= 1, "stem_input_grad: frames=%d", F);
  R3M_REQUIRE(dt == DT_F32 || dt == DT_BF16, "stem_input_grad: dtype %d (0 = fp32, 1 = bf16)", dt);
  const dim3 grid((unsigned)(F * 28LL));
  if (dt == DT_BF16)
    hipLaunchKernelGGL((stem_dgrad_kernel<bf16_t>), grid, dim3(256), 0, s, static_cast<const bf16_t*>(dz), w147, dx, accumulate);
  else
    hipLaunchKernelGGL((stem_dgrad_kernel<float>), grid, dim3(256), 0, s, static_cast<const float*>(dz), w147, dx, accumulate);
  return check_launch("stem_input_grad");
}

}  // namespace r3m
