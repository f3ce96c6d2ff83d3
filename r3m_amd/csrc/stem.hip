// r3m_amd — the fp32 stem for 224 x 224 frames, gfx950 (MI355X): x/255 -> Normalize -> conv1 7x7 / stride 2 / pad 3, 3 -> 64 channels,
// forward and weight gradient on the f32-input MFMA straight from the frames (no im2col matrix in HBM: that cost 8 MB written +
// 16 MB re-read per frame; the reference's first three steps, /root/reference/r3m/models/models_r3m.py:97-99 into torchvision's conv1).
//
//   stem_prep_kernel<Src> (stem_dev.h)         NCHW frames (or the raw clips through their crop boxes) -> normalised interleaved rows
//   stem_fwd_kernel                            persistent 256 x 64 tiles, fp32 or bf16 output, optional BatchNorm statistics
//   stem_wgrad_kernel + stem_wgrad_finish      per-block partials over output rows (reduced by wgrad.hip's launch_wgrad_reduce) -> dW
// Both kernels are their register prefetch around the MFMA loops of stem_dev.h, which stem_gen.hip (other frame sizes) shares; bf16
// plans run stem_bf16.hip; the input gradient is stem_dgrad.hip.
//
// With the (normalised, zero-padded) input rows staged in LDS as patch[y][(ix+3)*3 + c], the MFMA A-fragment of output pixel
// (oy, ox) for k = (kh, j) is patch[2*oy + kh][6*ox + j]: a per-lane base plus an immediate — no address arithmetic in the K loop.
#include "stem_dev.h"

namespace r3m {

constexpr int ST_PS = 692;      // patch row stride (forward): 230 pixels x 3 channels (+2 pad)
constexpr int ST_PSW = 694;     // patch row stride (weight gradient): == 22 (mod 32). There 32 lanes read patch[kh * stride + jj] for 32
                                // CONSECUTIVE k = 22 kh + jj, which cross a kernel-row boundary; with 692 (== 20 mod 32) the lanes of
                                // the next kernel row landed on the banks of jj = 20, 21 (2-way conflict on every B read: PMC
                                // lds_conflict_frac 0.44, round 2); with 694 the bank is k mod 32 — conflict-free

int launch_stem_prep_crop(const FrameSource& src, float* xn, int F, hipStream_t s) {
  if (src.is_u8) return launch_stem_prep_body(StemCrop<unsigned char>(src), xn, F, s, "stem_prep_crop");
  return launch_stem_prep_body(StemCrop<float>(src), xn, F, s, "stem_prep_crop");
}

int launch_stem_prep(const float* x_nchw, float* xn, int F, hipStream_t s) {
  return launch_stem_prep_body(StemFrames{x_nchw}, xn, F, s, "stem_prep");
}

template <int EPI, class OT>
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ xn, const float* __restrict__ w,
                                                        const GatherGemmParams p, int ntiles) {
  constexpr int SMEM = 13 * ST_PS + 64 * ST_KS;
  __shared__ __attribute__((aligned(16))) float smem[SMEM];
  float* patch = smem;                 // also the epilogue's scratch (8704 floats < 13*ST_PS): the weights behind it survive
  float* wl = smem + 13 * ST_PS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {   // weights once per (persistent) block
    const int n = tid >> 2, q = tid & 3;            // 4 threads per output channel
#pragma unroll
    for (int kh = 0; kh < 7; ++kh)
      for (int j = q; j < 22; j += 4) wl[n * ST_KS + kh * 22 + j] = (j < 21) ? w[n * 147 + kh * 21 + j] : 0.f;
  }
  const int lrow = lane & 31, lh = lane >> 5;
  int b_base[2];
  stem_fwd_b_base(b_base, lrow, lh);

  // Round 3: register prefetch — the 13 input rows of the NEXT tile (2184 float4, 9 per thread) are requested before this tile's
  // MFMAs and written to LDS after its epilogue (whose slabs alias the patch), so their latency rides under the matrix work.
  constexpr int PQ = (13 * 168 + 255) / 256;
  f32x4 pre[PQ];
  auto request = [&](int blk) __attribute__((always_inline)) {
    const long long f = blk / 49;
    const int iy0 = 2 * (((blk - (int)f * 49) * 256) / 112) - 3;
#pragma unroll
    for (int k = 0; k < PQ; ++k) {
      const int i = tid + 256 * k;
      const int y = i / 168, q = i - y * 168;
      const int iy = iy0 + y;
      pre[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < 13 * 168 && (unsigned)iy < 224u) pre[k] = ldg4(xn + ((f * 224 + iy) * 224) * 3 + q * 4);
    }
  };
  auto commit = [&]() __attribute__((always_inline)) {
    for (int i = tid; i < 13 * 20; i += 256) {       // zero borders: the epilogue's slabs overwrote them
      const int y = i / 20, e = i - y * 20;
      patch[y * ST_PS + (e < 9 ? e : 672 + e)] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < PQ; ++k) {
      const int i = tid + 256 * k;
      if (i < 13 * 168) {
        const int y = i / 168, q = i - y * 168;
        float* d = patch + y * ST_PS + 9 + q * 4;     // 9-float left border: not 16-byte aligned -> scalar LDS stores
        d[0] = pre[k][0]; d[1] = pre[k][1]; d[2] = pre[k][2]; d[3] = pre[k][3];
      }
    }
  };
  if ((int)blockIdx.x < ntiles) {
    request(blockIdx.x);
    commit();
  }
  for (int blk = blockIdx.x; blk < ntiles; blk += gridDim.x) {
    const long long f = blk / 49;
    const int lm0 = (blk - (int)f * 49) * 256;    // first output pixel of this tile inside its frame (12544 = 49 * 256)
    const int oy0 = lm0 / 112;
    __syncthreads();                              // the patch of this tile (and, first time, the weights) is in LDS
    const int nblk = blk + gridDim.x;
    if (nblk < ntiles) request(nblk);
    int a_base[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int lm = lm0 + wave * 64 + t * 32 + lrow;
      const int oy = lm / 112, ox = lm - oy * 112;
      a_base[t] = 2 * (oy - oy0) * ST_PS + 6 * ox + lh;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 7; ++kh) stem_fwd_krow(patch + a_base[0] + kh * ST_PS, patch + a_base[1] + kh * ST_PS, wl, b_base, kh, acc);
    __syncthreads();
    gg_epilogue<256, 64, 4, 1, EPI, 13 * ST_PS, OT>(p, acc, smem, blk * 256, 0, blk);
    __syncthreads();   // the epilogue slabs alias the patch that is refilled now
    if (nblk < ntiles) commit();
  }
}

int launch_stem_fwd(const float* x_nchw, const float* w147, void* y, float* stats, int F, int dt, hipStream_t s) {
  const GatherGemmParams p = stem_fwd_params(y, stats, dt, F, 112, 112);
  stem_prof_begin(KC_GEMM_NARROW, p.M, (double)F * 224 * 224 * 3 * 4, dt, s, stats);
  const int ntiles = F * 49;
  const int grid = ntiles < 512 ? ntiles : 512;   // persistent blocks (2 per CU): the 39 KB weight image is staged once per block
  if (dt == DT_BF16) {
    if (stats) hipLaunchKernelGGL((stem_fwd_kernel<EPI_STATS, bf16_t>), dim3(grid), dim3(256), 0, s, x_nchw, w147, p, ntiles);
    else hipLaunchKernelGGL((stem_fwd_kernel<0, bf16_t>), dim3(grid), dim3(256), 0, s, x_nchw, w147, p, ntiles);
  } else {
    if (stats) hipLaunchKernelGGL((stem_fwd_kernel<EPI_STATS, float>), dim3(grid), dim3(256), 0, s, x_nchw, w147, p, ntiles);
    else hipLaunchKernelGGL((stem_fwd_kernel<0, float>), dim3(grid), dim3(256), 0, s, x_nchw, w147, p, ntiles);
  }
  prof_end(s);
  return check_launch("stem_fwd");
}

// weight gradient (stem_dev.h): one output image row (112 pixels = 56 K pairs) per iteration
template <class T>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ x, const T* __restrict__ dY,
                                                          float* __restrict__ partial, int total_rows) {
  __shared__ __attribute__((aligned(16))) float smem[112 * 64 + 7 * ST_PSW];
  float* dys = smem;                  // 16-byte aligned (float4 stores); the patch takes scalar stores
  float* patch = smem + 112 * 64;
  const int tid = threadIdx.x;
  const StemWgLane L = stem_wg_lane<ST_PSW>(0);
  f32x16 tot[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[t][r] = 0.f;

  // Round 3: register prefetch. The next output row's operands (7 input rows = 1176 float4, the dY row = 1792 float4: 5 + 7 per
  // thread) are requested BEFORE this row's MFMAs and written to LDS after them, so their global latency (~2 us of the ~6.5 us a
  // row took) rides under the matrix work instead of in front of it. The zero borders of the patch rows never change: written once.
  constexpr int PQ = (7 * 168 + 255) / 256, DQ = 112 * 16 / 256;     // 5, 7
  f32x4 pre_p[PQ], pre_d[DQ];
  auto request = [&](int row) __attribute__((always_inline)) {
    const long long f = row / 112;
    const int iy0 = 2 * (row - (int)f * 112) - 3;
#pragma unroll
    for (int k = 0; k < PQ; ++k) {
      const int i = tid + 256 * k;
      const int y = i / 168, q = i - y * 168;
      const int iy = iy0 + y;
      pre_p[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < 7 * 168 && (unsigned)iy < 224u) pre_p[k] = ldg4(x + ((f * 224 + iy) * 224) * 3 + q * 4);
    }
    const T* src = dY + (long long)row * 112 * 64;
#pragma unroll
    for (int k = 0; k < DQ; ++k) pre_d[k] = ld4t(src + (tid + 256 * k) * 4);
  };
  auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < PQ; ++k) {
      const int i = tid + 256 * k;
      if (i < 7 * 168) {
        const int y = i / 168, q = i - y * 168;
        float* d = patch + y * ST_PSW + 9 + q * 4;     // 9-float left border: not 16-byte aligned -> scalar LDS stores
        d[0] = pre_p[k][0]; d[1] = pre_p[k][1]; d[2] = pre_p[k][2]; d[3] = pre_p[k][3];
      }
    }
#pragma unroll
    for (int k = 0; k < DQ; ++k) *reinterpret_cast<f32x4*>(dys + (tid + 256 * k) * 4) = pre_d[k];
  };
  {
    constexpr int TAIL = ST_PSW - 681;
    for (int i = tid; i < 7 * (9 + TAIL); i += 256) {
      const int y = i / (9 + TAIL), e = i - y * (9 + TAIL);
      patch[y * ST_PSW + (e < 9 ? e : 672 + e)] = 0.f;
    }
  }
  int row = blockIdx.x;
  if (row < total_rows) {
    request(row);
    commit();
  }
  __syncthreads();
  for (; row < total_rows; row += gridDim.x) {
    const int next = row + gridDim.x;
    if (next < total_rows) request(next);
    stem_wg_row<56>(dys, patch, L, 0, tot);
    __syncthreads();                      // every wave is done reading this row's tiles
    if (next < total_rows) commit();
    __syncthreads();
  }
  stem_wg_store(partial, L, tot);
}

size_t stem_wgrad_ws_floats() { return stem_ws_partials(STEM_WG_BLOCKS, ST_DW); }

int launch_stem_wgrad(const float* x_nchw, const void* dY, float* dw147, float* ws /* stem_wgrad_ws_floats() + 64*160 */, int F,
                      int accumulate, int dt, hipStream_t s) {
  const int total_rows = F * 112;
  const int nb = total_rows < STEM_WG_BLOCKS ? total_rows : STEM_WG_BLOCKS;
  stem_prof_begin(KC_WGRAD_NARROW, F * 12544, (double)F * 224 * 224 * 3 * 4, dt, s);
  if (dt == DT_BF16)
    hipLaunchKernelGGL((stem_wgrad_kernel<bf16_t>), dim3(nb), dim3(256), 0, s, x_nchw, static_cast<const bf16_t*>(dY), ws, total_rows);
  else
    hipLaunchKernelGGL((stem_wgrad_kernel<float>), dim3(nb), dim3(256), 0, s, x_nchw, static_cast<const float*>(dY), ws, total_rows);
  prof_end(s);
  if (int e = check_launch("stem_wgrad")) return e;
  return stem_wgrad_finish<ST_DW, 22>(ws, nb, STEM_WG_BLOCKS, dw147, accumulate, s, "stem_unpack_dw22");
}

}  // namespace r3m
