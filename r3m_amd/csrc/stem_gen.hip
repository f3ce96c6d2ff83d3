// r3m_amd — the stem for frames of any H x W in [32, 512]: x/255 -> Normalize -> conv1 7x7/2 pad 3 (3 -> 64), its weight gradient and
// its input gradient. torchvision's ResNet takes any input size (every layer uses floor((H + 2p - k) / s) + 1); the reference feeds the
// frames at their own size when obs_shape is the default (/root/reference/r3m/models/models_r3m.py:84-100). The 224 x 224 kernels
// (stem.hip, stem_bf16.hip, stem_dgrad.hip) stay what 224 frames run; these general forms take every other size, and 224 too
// under r3m_debug_set_generic_stem (tests, A/B).
//
// Normalised image: xn[f][iy][ix * 3 + c], fp32 for fp32 plans and bf16 for bf16 plans (the bf16 stem's operand rounding: the normalised
// value rounded once). Both precisions run the exact fp32 MFMA (v_mfma_f32_32x32x2_f32): with bf16 operands every product is exact in
// fp32, so the bf16 path computes what a bf16 MFMA with fp32 accumulation computes, up to the order of the fp32 sums.
//
// Forward: the 224 kernel's geometry (stem.hip stem_fwd_kernel; the K loop is stem_dev.h's, shared with it; the weight-image fill is
// this kernel's own flat loop) with the row width and the tile's row span made general. A tile is 256
// consecutive output pixels of the flattened [F, Ho, Wo] index; it may span several output rows, and the end of one frame and the start
// of the next (Ho * Wo >= 256 for H, W >= 32, so at most two frames). It stages, per frame part, the 2 r + 5 input rows its r output
// rows touch, at a padded width of (W + 6) * 3 floats (9 leading zeros, zeros behind the data): the MFMA A operand of pixel (oy, ox)
// for k = (kh, j) is patch[2 (oy - oy_first) + kh][6 ox + j] — a per-lane base plus an immediate, no vector work in the K loop.
// Pixels past M read a valid pixel and their accumulators are cleared after the K loop (the BatchNorm partials then see zeros).
//
// Weight gradient: stem_dev.h's lane geometry, row GEMM and partial layout (shared with stem.hip stem_wgrad_kernel, whose workspace
// and block count it takes) with one output row of Wo pixels per iteration (K = pixels, rounded up to even with zero dY), 7 staged
// input rows at a row stride == 22 (mod 32) as ST_PSW documents.
//
// Input gradient: stem_dgrad.hip's per-row GEMM (M = pixels of one dZ row, N = 21 (kw, c) columns, K = kernel rows x 64 channels; weight
// staging, MFMA step and scale in stem_dev.h) with M tails, followed by the col2im gather out of LDS; one wave per input row, four rows
// of one parity per block.
#include "stem_dev.h"
#include <algorithm>

namespace r3m {

namespace {

constexpr int SG_EPI = 4 * 32 * 68;    // floats the shared epilogue's slabs take (gg_epilogue<256, 64, 4, 1>)

struct StemGeo {
  int F, H, W, Ho, Wo;
  int PS;          // staged row stride (floats)
  int rows;        // forward: most input rows one tile stages
  int wl_off;      // forward: LDS offset of the weight image
  int Wo2;         // weight gradient: Wo rounded up to even
};

__device__ __forceinline__ float sg_ld(const float* p) { return *p; }
__device__ __forceinline__ float sg_ld(const bf16_t* p) { return static_cast<float>(*p); }

// smallest stride >= len with stride == r (mod 32)
static int sg_stride(int len, int r) { return len + ((r - len % 32) % 32 + 32) % 32; }

static StemGeo stem_geo(int F, int H, int W) {
  StemGeo g;
  g.F = F; g.H = H; g.W = W;
  g.Ho = (H + 6 - 7) / 2 + 1;
  g.Wo = (W + 6 - 7) / 2 + 1;
  g.Wo2 = (g.Wo + 1) & ~1;
  // forward: a row must hold the 9 + 3 W staged floats and every A read, up to 6 (Wo - 1) + 1 + 20; == 20 (mod 32) as ST_PS
  g.PS = sg_stride(std::max(3 * W + 9, 6 * g.Wo + 16), 20);
  const int nr = (g.Wo + 254) / g.Wo + 1;                       // output rows 256 consecutive pixels of one frame can touch
  const bool straddle = F > 1 && (g.Ho * g.Wo) % 256 != 0;      // a tile may hold the end of one frame and the start of the next
  g.rows = 2 * nr + (straddle ? 10 : 5);
  g.wl_off = std::max(g.rows * g.PS, SG_EPI);
  g.wl_off = (g.wl_off + 3) & ~3;
  return g;
}
static int stem_fwd_lds_bytes(const StemGeo& g) { return (g.wl_off + 64 * ST_KS) * 4; }
static int stem_wgrad_psw(const StemGeo& g) { return sg_stride(std::max(3 * g.W + 9, 6 * g.Wo2 + 16), 22); }
static int stem_wgrad_lds_bytes(const StemGeo& g) { return (g.Wo2 * 64 + 7 * stem_wgrad_psw(g)) * 4; }
static int stem_dgrad_lds_bytes(const StemGeo& g) { return (4 * SD_WK + 4 * g.Wo * 21) * 4; }

// ---- pre-pass: NCHW fp32 0..255 -> xn[f][iy][ix*3 + c] (the reference's (x/255 - mean)/std with IEEE divisions). Its own kernel, not an
// instantiation of stem_dev.h's stem_prep_kernel: that one measured 2 % slower here (profiles/stem_share_ab.txt) ----
template <class OT>
__global__ __launch_bounds__(256) void stem_prep_gen_kernel(const float* __restrict__ x, OT* __restrict__ xn, int H, int W, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // one thread per (f, iy, ix)
  if (i >= total) return;
  const int ix = (int)(i % W);
  const long long t = i / W;
  const int iy = (int)(t % H);
  const long long f = t / H;
  OT* o = xn + i * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = static_cast<OT>(stem_normalize(x[((f * 3 + c) * H + iy) * (long long)W + ix], c));
}

// ---- forward ----
template <int EPI, class IT, class OT>
__global__ __launch_bounds__(256) void stem_fwd_gen_kernel(const IT* __restrict__ xn, const float* __restrict__ w, const GatherGemmParams p,
                                                            const StemGeo g, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* patch = smem;                 // also the epilogue's scratch (SG_EPI floats <= wl_off): the weights behind it survive
  float* wl = smem + g.wl_off;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 64 * ST_K; i += 256) {      // this kernel's own fill (not shared with stem.hip: one flat loop)
    const int n = i / ST_K, k = i - n * ST_K;
    const int kh = k / 22, j = k - kh * 22;
    float v = j < 21 ? w[n * 147 + kh * 21 + j] : 0.f;
    if (sizeof(IT) == 2) v = static_cast<float>(static_cast<bf16_t>(v));   // bf16 plans: the bf16 weight operand
    wl[n * ST_KS + k] = v;
  }
  const int lrow = lane & 31, lh = lane >> 5;
  int b_base[2];
  stem_fwd_b_base(b_base, lrow, lh);
  const int HWo = g.Ho * g.Wo;
  const int PS = g.PS;
  const int rowlen = 3 * g.W;

  for (int blk = blockIdx.x; blk < ntiles; blk += gridDim.x) {
    const int m0 = blk * 256;
    const int mlast = min(m0 + 255, p.M - 1);
    const int fA = m0 / HWo, oyA0 = (m0 - fA * HWo) / g.Wo;
    const int fL = mlast / HWo, oyL = (mlast - fL * HWo) / g.Wo;
    const int oyA1 = fL != fA ? g.Ho - 1 : oyL;
    const int nA = 2 * (oyA1 - oyA0) + 7;
    const int nrows = nA + (fL != fA ? 2 * oyL + 7 : 0);
    __syncthreads();                   // the previous tile's epilogue slabs (aliasing the patch) are drained
    for (int i = tid; i < nrows * PS; i += 256) {
      const int y = i / PS, e = i - y * PS;
      const int f = y < nA ? fA : fA + 1;
      const int iy = y < nA ? 2 * oyA0 - 3 + y : y - nA - 3;
      const int d = e - 9;
      float v = 0.f;
      if ((unsigned)iy < (unsigned)g.H && (unsigned)d < (unsigned)rowlen) v = sg_ld(xn + ((long long)f * g.H + iy) * rowlen + d);
      patch[i] = v;
    }
    int a_base[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int m = min(m0 + wave * 64 + t * 32 + lrow, mlast);   // pixels past M read a valid pixel; cleared after the K loop
      const int f = m / HWo, rem = m - f * HWo;
      const int oy = rem / g.Wo, ox = rem - oy * g.Wo;
      const int y0 = f == fA ? 2 * (oy - oyA0) : nA + 2 * oy;
      a_base[t] = y0 * PS + 6 * ox + lh;
    }
    __syncthreads();
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 7; ++kh) stem_fwd_krow(patch + a_base[0] + kh * PS, patch + a_base[1] + kh * PS, wl, b_base, kh, acc);
    if (m0 + 256 > p.M) {              // the last tile: rows past M must hold zeros (BatchNorm partials)
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wave * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (m >= p.M) { acc[tm][0][r] = 0.f; acc[tm][1][r] = 0.f; }
        }
    }
    __syncthreads();
    gg_epilogue<256, 64, 4, 1, EPI, SG_EPI, OT>(p, acc, smem, m0, 0, blk);
  }
}

// ---- weight gradient: dW[co][kh*22 + j] partial of one block, one output row per iteration ----
template <class IT, class T>
__global__ __launch_bounds__(256) void stem_wgrad_gen_kernel(const IT* __restrict__ xn, const T* __restrict__ dY, float* __restrict__ partial,
                                                              const StemGeo g, int PSW, int total_rows) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dys = smem;                   // [Wo2][64]
  float* patch = smem + g.Wo2 * 64;    // 7 rows at stride PSW
  const int tid = threadIdx.x;
  const StemWgLane L = stem_wg_lane<0>(PSW);
  f32x16 tot[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[t][r] = 0.f;
  const int rowlen = 3 * g.W;
  const int npairs = g.Wo2 / 2;
  for (int row = blockIdx.x; row < total_rows; row += gridDim.x) {
    const int f = row / g.Ho;
    const int iy0 = 2 * (row - f * g.Ho) - 3;
    __syncthreads();                            // every wave is done reading the previous row's tiles
    for (int i = tid; i < 7 * PSW; i += 256) {
      const int y = i / PSW, e = i - y * PSW;
      const int iy = iy0 + y, d = e - 9;
      float v = 0.f;
      if ((unsigned)iy < (unsigned)g.H && (unsigned)d < (unsigned)rowlen) v = sg_ld(xn + ((long long)f * g.H + iy) * rowlen + d);
      patch[i] = v;
    }
    const T* src = dY + (long long)row * g.Wo * 64;
    for (int i = tid; i < g.Wo2 * 16; i += 256) {
      const int px = i >> 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (px < g.Wo) v = ld4t(src + i * 4);
      *reinterpret_cast<f32x4*>(dys + i * 4) = v;
    }
    __syncthreads();
    stem_wg_row<0>(dys, patch, L, npairs, tot);
  }
  stem_wg_store(partial, L, tot);
}

// ---- input gradient: one wave per input row h (four rows of parity P per block) ----
template <int P, class T>
__device__ __forceinline__ void stem_dgrad_gen_item(const T* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx,
                                                    const StemGeo& g, int f, int grp, int accumulate, float* smem) {
  constexpr int NK = P ? 4 : 3;          // kernel rows with h + 3 - kh even: kh = (1 - P) + 2 kk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lrow = lane & 31, lh = lane >> 5;
  stem_dgrad_weights<P>(smem, w);
  float* U = smem + 4 * SD_WK + wave * g.Wo * 21;
  const int h = 2 * (4 * grp + wave) + P;
  const bool valid = h < g.H;            // wave-uniform
  __syncthreads();                       // weights staged
  if (valid) {
    const int ntm = (g.Wo + 31) / 32;
    for (int t = 0; t < ntm; ++t) {
      const int ox = 32 * t + lrow;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int kh = (1 - P) + 2 * kk;
        const int oy = (h + 3 - kh) >> 1;
        const bool ok = (unsigned)oy < (unsigned)g.Ho && ox < g.Wo;
        const T* src = dz + (((long long)f * g.Ho + (ok ? oy : 0)) * g.Wo + (ok ? ox : 0)) * 64 + lh * 32;
        f32x4 a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = ok ? stem_load4(src + 4 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
        const float* wb = smem + kk * SD_WK + lh * SD_WH + lrow;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = stem_dgrad_mfma4(a[j], wb + 128 * j, acc);
      }
      if (lrow < 21) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;   // C/D row of register r
          if (m < g.Wo) U[m * 21 + lrow] = acc[r];
        }
      }
    }
  }
  __syncthreads();                       // U complete
  if (valid) {
    for (int wcol = lane; wcol < g.W; wcol += 64) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float sum = 0.f;
        for (int kw = (wcol + 1) & 1; kw < 7; kw += 2) {
          const int ox = (wcol + 3 - kw) >> 1;
          if ((unsigned)ox < (unsigned)g.Wo) sum += U[ox * 21 + kw * 3 + c];
        }
        float* o = dx + (((long long)f * 3 + c) * g.H + h) * g.W + wcol;
        const float v = sum * stem_dgrad_scale(c);
        *o = accumulate ? *o + v : v;
      }
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void stem_dgrad_gen_kernel(const T* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx,
                                                              const StemGeo g, int groups, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int item = blockIdx.x;
  const int f = item / (2 * groups);
  const int rem = item - f * 2 * groups;
  if (rem & 1) stem_dgrad_gen_item<1, T>(dz, w, dx, g, f, rem >> 1, accumulate, smem);
  else stem_dgrad_gen_item<0, T>(dz, w, dx, g, f, rem >> 1, accumulate, smem);
}

}  // namespace

int stem_gen_check(int F, int H, int W) {
  R3M_REQUIRE(H >= STEM_GEN_MIN && W >= STEM_GEN_MIN && H <= STEM_GEN_MAX && W <= STEM_GEN_MAX,
              "stem: frames %d x %d outside [%d, %d] (the general stem's LDS staging bounds the width at %d)", H, W, STEM_GEN_MIN,
              STEM_GEN_MAX, STEM_GEN_MAX);
  R3M_REQUIRE(F >= 1, "stem: frames=%d", F);
  // the GEMM row count F Ho Wo and the tile origin are ints: the output [F, Ho, Wo, 64] and the frames stay below 2^31 elements
  const long long out = (long long)F * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * 64;
  R3M_REQUIRE(out < 0x80000000LL && (long long)F * 3 * H * W < 0x80000000LL,
              "stem: %d frames of %d x %d give %lld output elements (limit 2^31 - 1: 32-bit row and tile indices)", F, H, W, out);
  return 0;
}

int launch_stem_prep_gen(const float* x_nchw, float* xn, int F, int H, int W, int dt, hipStream_t s) {
  if (int e = stem_gen_check(F, H, W)) return e;
  const long long total = (long long)F * H * W;
  if (dt == DT_BF16)
    hipLaunchKernelGGL((stem_prep_gen_kernel<bf16_t>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x_nchw,
                       reinterpret_cast<bf16_t*>(xn), H, W, total);
  else
    hipLaunchKernelGGL((stem_prep_gen_kernel<float>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x_nchw, xn, H, W, total);
  return check_launch("stem_prep_gen");
}

int launch_stem_fwd_gen(const float* xn, const float* w147, void* y, float* stats, int F, int H, int W, int dt, hipStream_t s) {
  if (int e = stem_gen_check(F, H, W)) return e;
  const StemGeo g = stem_geo(F, H, W);
  const GatherGemmParams p = stem_fwd_params(y, stats, dt, F, g.Ho, g.Wo);
  const int ntiles = ceil_div(p.M, 256);
  const int grid = ntiles < 512 ? ntiles : 512;
  const int lds = stem_fwd_lds_bytes(g);
  stem_prof_begin(KC_GEMM_NARROW, p.M, (double)F * H * W * 3 * (dt == DT_BF16 ? 2 : 4), dt, s, stats);
#define SG_FWD(E, IT, OT)                                                                                                     \
  do {                                                                                                                        \
    static DynLdsOptIn oi;                                                                                                    \
    if (int e = ensure_dyn_lds(oi, reinterpret_cast<const void*>(stem_fwd_gen_kernel<E, IT, OT>), lds, "stem_fwd_gen")) return e; \
    hipLaunchKernelGGL((stem_fwd_gen_kernel<E, IT, OT>), dim3(grid), dim3(256), lds, s, reinterpret_cast<const IT*>(xn), w147, p, g, \
                       ntiles);                                                                                               \
  } while (0)
  if (dt == DT_BF16) {
    if (stats) SG_FWD(EPI_STATS, bf16_t, bf16_t);
    else SG_FWD(0, bf16_t, bf16_t);
  } else {
    if (stats) SG_FWD(EPI_STATS, float, float);
    else SG_FWD(0, float, float);
  }
#undef SG_FWD
  prof_end(s);
  return check_launch("stem_fwd_gen");
}

int launch_stem_wgrad_gen(const float* xn, const void* dY, float* dw147, float* ws, int F, int H, int W, int accumulate, int dt,
                          hipStream_t s) {
  if (int e = stem_gen_check(F, H, W)) return e;
  const StemGeo g = stem_geo(F, H, W);
  const int PSW = stem_wgrad_psw(g);
  const int total_rows = F * g.Ho;
  const int nb = total_rows < STEM_WG_BLOCKS ? total_rows : STEM_WG_BLOCKS;
  const int lds = stem_wgrad_lds_bytes(g);
  stem_prof_begin(KC_WGRAD_NARROW, F * g.Ho * g.Wo, (double)F * H * W * 3 * (dt == DT_BF16 ? 2 : 4), dt, s);
#define SG_WG(IT, T)                                                                                                          \
  do {                                                                                                                        \
    static DynLdsOptIn oi;                                                                                                    \
    if (int e = ensure_dyn_lds(oi, reinterpret_cast<const void*>(stem_wgrad_gen_kernel<IT, T>), lds, "stem_wgrad_gen")) return e; \
    hipLaunchKernelGGL((stem_wgrad_gen_kernel<IT, T>), dim3(nb), dim3(256), lds, s, reinterpret_cast<const IT*>(xn),           \
                       static_cast<const T*>(dY), ws, g, PSW, total_rows);                                                    \
  } while (0)
  if (dt == DT_BF16) SG_WG(bf16_t, bf16_t);
  else SG_WG(float, float);
#undef SG_WG
  prof_end(s);
  if (int e = check_launch("stem_wgrad_gen")) return e;
  return stem_wgrad_finish<ST_DW, 22>(ws, nb, STEM_WG_BLOCKS, dw147, accumulate, s, "stem_gen_unpack");
}
size_t stem_wgrad_gen_ws_floats() { return stem_ws_floats(STEM_WG_BLOCKS, ST_DW); }

int launch_stem_input_grad_gen(const void* dz, int dt, const float* w147, float* dx, int F, int H, int W, int accumulate, hipStream_t s) {
  if (int e = stem_gen_check(F, H, W)) return e;
  R3M_REQUIRE(F >= 1, "stem_input_grad_gen: frames=%d", F);
  R3M_REQUIRE(dt == DT_F32 || dt == DT_BF16, "stem_input_grad_gen: dtype %d (0 = fp32, 1 = bf16)", dt);
  const StemGeo g = stem_geo(F, H, W);
  const int groups = ceil_div((H + 1) / 2, 4);          // blocks per (frame, parity): four rows of that parity each
  const dim3 grid((unsigned)(F * 2LL * groups));
  const int lds = stem_dgrad_lds_bytes(g);
  if (dt == DT_BF16) {
    static DynLdsOptIn oi;
    if (int e = ensure_dyn_lds(oi, reinterpret_cast<const void*>(stem_dgrad_gen_kernel<bf16_t>), lds, "stem_input_grad_gen")) return e;
    hipLaunchKernelGGL((stem_dgrad_gen_kernel<bf16_t>), grid, dim3(256), lds, s, static_cast<const bf16_t*>(dz), w147, dx, g, groups, accumulate);
  } else {
    static DynLdsOptIn oi;
    if (int e = ensure_dyn_lds(oi, reinterpret_cast<const void*>(stem_dgrad_gen_kernel<float>), lds, "stem_input_grad_gen")) return e;
    hipLaunchKernelGGL((stem_dgrad_gen_kernel<float>), grid, dim3(256), lds, s, static_cast<const float*>(dz), w147, dx, g, groups, accumulate);
  }
  return check_launch("stem_input_grad_gen");
}

// LDS bytes of the three general kernels at H x W (the CPU tests check the 160 KiB bound over the supported range)
int stem_gen_lds(int F, int H, int W, int* fwd, int* wgrad, int* dgrad) {
  if (int e = stem_gen_check(F, H, W)) return e;
  const StemGeo g = stem_geo(F, H, W);
  if (fwd) *fwd = stem_fwd_lds_bytes(g);
  if (wgrad) *wgrad = stem_wgrad_lds_bytes(g);
  if (dgrad) *dgrad = stem_dgrad_lds_bytes(g);
  return 0;
}

}  // namespace r3m
