// r3m_amd — internal declarations shared by the HIP translation units.
// gfx950 (MI355X / CDNA4) only: wave = 64 lanes, fp32-input MFMA, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

// ---- experiment switches -------------------------------------------------------------------------------------
// The SHIPPED library (r3m_amd/csrc/build.sh) has one code path per shape: it reads no environment variables and contains
// none of the timing probes (some of which deliberately produce wrong results). Builds with -DR3M_PROBES
// (tools/build_ab.sh none probes) bring both back so the A/B measurements quoted in DESIGN.md can be repeated.
#ifdef R3M_PROBES
#include <cstdlib>
#define R3M_ENV_INT(name, dflt) ([]() -> int { static const int v_ = []() { const char* e_ = getenv(name); return e_ ? atoi(e_) : (dflt); }(); return v_; }())
#define R3M_PROBE(p) ((p).debug)
#else
#define R3M_ENV_INT(name, dflt) (dflt)
#define R3M_PROBE(p) 0
#endif

namespace r3m {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- error plumbing (thread-local message, C-ABI returns non-zero on failure) ----
void set_last_error(const char* fmt, ...);
int  check_launch(const char* what);  // hipGetLastError() -> 0 / code (+ message)

#define R3M_REQUIRE(cond, ...)                  \
  do {                                          \
    if (!(cond)) {                              \
      r3m::set_last_error(__VA_ARGS__);         \
      return 1;                                 \
    }                                           \
  } while (0)
#define TRY(x)                   \
  do {                           \
    if (int e_ = (x)) return e_; \
  } while (0)

static inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// Opt-in for > 64 KiB of dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize), cached per call site AND per device:
// function attributes belong to a device, and launches arrive from several host threads (forward: caller, backward: autograd
// engine). The cache is a plain int per device — a racing pair of threads sets the same attribute twice, which is idempotent.
struct DynLdsOptIn { int bytes[32] = {0}; };
int ensure_dyn_lds(DynLdsOptIn& cache, const void* fn, int bytes, const char* what);

// ---- epilogue flags of the gather-GEMM (conv fwd / dgrad / linear) ----
enum : int {
  EPI_STATS      = 1,   // emit per-(row-block, column) sum / sum-of-squares partials (BatchNorm statistics)
  EPI_ACCUM      = 2,   // out = acc + out_old
  EPI_MASKED_ADD = 4,   // out = acc + add0 * (add1 > 0)   (residual gradient joining a dgrad)
  EPI_BIAS       = 8,   // out = acc + bias[col]
  EPI_RELU       = 16,  // out = max(out, 0)
  EPI_MASK_OUT   = 32,  // out = (add1 > 0) ? acc : 0        (ReLU backward fused into a Linear dgrad)
  EPI_BNRED      = 64,  // dgrad only: the result IS the gradient dz entering a BatchNorm(+ReLU) whose pre-normalisation output is
                        // bn_y — also emit that BatchNorm's backward partials per 64 result rows: sum(g), sum(g * (y - mean)),
                        // g = dz * [relu mask] (mask: bn_bits, or recomputed as fma(y, bn_scale, bn_shift) > 0). Replaces the
                        // stand-alone first pass of BatchNorm backward (one read of dz and of y saved per layer).
  EPI_AFFINE     = 128, // forward only (round 6, the inference path): out = acc * bn_scale[col] + bn_shift[col] — eval-mode BatchNorm
                        // (running statistics) applied where the convolution result is stored; then EPI_ACCUM (+ the residual already
                        // in `out`) and EPI_RELU in that order: relu(bn(conv(x)) + identity) of a block tail in ONE store.
  EPI_GELU       = 256, // few-row Linear only (conv_small.hip), with EPI_BIAS: out = gelu(acc + bias[col]), the exact form (gelu_erf)
};

// the exact GELU 0.5 v (1 + erf(v / sqrt 2)): bias_gelu_kernel (text.hip) and the EPI_GELU store (conv_small.hip) share this arithmetic
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// rows of the EPI_BNRED partial buffer one launch writes ([rows][2][Nc] floats): one per 64 GEMM rows, tile-independent
static inline int bnred_partial_rows(long long M) { return (int)((M + 63) / 64); }

constexpr int MAX_TAPS = 49;

// activation storage type of a launch / an encoder plan
enum : int { DT_F32 = 0, DT_BF16 = 1 };

// One launch of the gather-GEMM:  out[row(m), :] = sum_t  in[pix(m) + (dy_t, dx_t), :] * B[:, wt_t, :]^T
struct GatherGemmParams {
  const float* A;      // input activations, NHWC [N, Hi, Wi, Ci]
  const float* B;      // weights [Nc][T][Ci]  (row = output column, K contiguous)
  float* out;          // output activations, NHWC [N, Ho, Wo, Nc]
  const float* add0;   // EPI_MASKED_ADD: gradient tensor, same shape as out
  const float* add1;   // EPI_MASKED_ADD / EPI_MASK_OUT: mask source (post-ReLU activation), same shape as out
  const unsigned* addbits;  // EPI_MASKED_ADD: optional 1-bit/element ReLU mask of that activation (used instead of add1)
  const float* bias;   // EPI_BIAS: [Nc]
  float* stats;        // EPI_STATS: [gridM][2][Nc];  EPI_BNRED: [bnred_partial_rows(M)][2][Nc]
  const float* bn_y;        // EPI_BNRED: the consumer BatchNorm's input (conv output), same shape / storage type as out
  const unsigned* bn_bits;  // EPI_BNRED: 1-bit ReLU mask of the BatchNorm(+residual) output, or null -> recompute from bn_y
  const float* bn_scale;    // EPI_BNRED: [Nc] forward coefficients (mask recomputation)
  const float* bn_shift;
  const float* bn_mean;     // EPI_BNRED: [Nc] batch (or running) mean
  int N, Hi, Wi, Ci;
  int Hg, Wg;          // GEMM row grid per image: m = (n*Hg + gy)*Wg + gx
  int Ho, Wo, Nc;      // output tensor dims (Nc = GEMM N)
  int is;              // input pixel = (gy*is + dy_t, gx*is + dx_t)
  int os, ooy, oox;    // output pixel = (gy*os + ooy, gx*os + oox)
  int M;               // N*Hg*Wg
  int T;               // taps in the weight tensor (B row stride = T*Ci)
  int ntaps;           // taps visited by this launch
  int flags;
  int simple_rows;     // 1: 1x1 / stride 1 / no padding -> input row offset = m*Ci (no pixel decode)
  int debug;           // timing probes (R3M_GG_DEBUG), 0 in production
  int dtype;           // DT_F32: A/B/out/add0/add1 are fp32; DT_BF16: they address bf16 tensors (stats/bias stay fp32)
  unsigned* tile_ctr;  // persistent kernels (conv_pw.hip): 8 zeroed counters = per-XCD tile queues, or null -> static tile assignment
  signed char dy[MAX_TAPS];
  signed char dx[MAX_TAPS];
  unsigned char wt[MAX_TAPS];
  int tap[MAX_TAPS];   // packed by the launcher: (dy & 255) | (dx & 255) << 8 | wt << 16  (dword table -> scalar loads)
};

struct WgradParams {
  const float* dY;   // [M][Co]  (NHWC rows of the conv output gradient)
  const float* X;    // conv input, NHWC [N, Hi, Wi, Ci]
  float* out;        // [splitK][Co][T][Ci] partials (or the gradient itself when splitK == 1)
  int N, Hi, Wi, Ci;
  int Ho, Wo, Co;
  int KH, KW, stride, pad;
  int M;               // N*Ho*Wo
  int simple_rows;     // 1x1 stride-1: X row offset = m*Ci
  int dtype;           // DT_F32 / DT_BF16 storage of dY and X (out is always fp32)
  // copied from the launch's WgradPlan by launch_wgrad:
  int rows_per_split;  // multiple of 32
  int tilesN;          // ceil(Ci / BN)
  int gx;              // (co tile, ci tile, tap group) blocks per split; the launch is 1-D: gx * split blocks
  int xcd;             // 1: XCD-aware block order — all blocks of one split (same dY / X rows) run on ONE XCD and share its L2
  int debug;           // timing probes (probe builds, R3M_WG_DEBUG: 1 no DMA at all, 2 no X pieces, 4 no dY pieces); 0 in production
};

// ---- launchers (conv.hip): fp32 forward / input-gradient gather-GEMM, dgrad weight transposes ----
int debug_occupancy(int* out4);
int launch_gather_gemm(const GatherGemmParams& p, hipStream_t s);
double gather_gemm_alg_bytes(const GatherGemmParams& p, int elem_bytes);
bool gather_gemm_fuses_affine(const GatherGemmParams& p);   // inference forward: the launch's kernel has the EPI_AFFINE epilogues
int gather_gemm_grid_m(int M, int Nc);   // number of row blocks the launcher will use (stats partial rows)
// The engine hands the NEXT launch_gather_gemm of this thread 8 zeroed device counters (dynamic tile queues of the persistent
// kernel: a block that finds its CU shared with another stream's kernel — RCCL during an overlapped all-reduce — simply takes
// fewer tiles). Consumed (and cleared) by that launch whether or not it uses them; launches without it assign tiles statically.
void gg_set_tile_counters(unsigned* ctr8, int sets = 1);
int gg_set_dynamic_tiles(int on);        // diagnostic switch (r3m_debug_set_dynamic_tiles): 0 = ignore the counters, assign statically
void gg_route_record_begin(int* out, int cap);   // dry run on this thread: launch_gather_gemm records its kernel family and launches nothing
int gg_route_record_end();                       // -> launches seen since begin
struct WtEntry { long long w_off, wt_off; int Co, T, Ci, pad_; };
int launch_transpose_w_all(const float* params, void* wt, const WtEntry* tab, const int* tile0, int n, int tiles, int dt, hipStream_t s);
int launch_transpose_w(const float* W, float* Wt, int Co, int T, int Ci, hipStream_t s);

// ---- launchers (conv_pw.hip): persistent kernel for 1x1 / stride-1 launches and dense or parity-strided gathers (fp32) ----
bool pw_gemm_eligible(const GatherGemmParams& p);
int pw_gemm_form(const GatherGemmParams& p);            // 0 none, 1 pointwise, 2 gather, 3 gather with strided output rows
int launch_pw_gemm(const GatherGemmParams& p, hipStream_t s);

// ---- the weight gradients behind the stem (wgrad.hip, wgrad_win.hip, wgrad_bf16.hip; shared device code: wgrad_dev.h) ----
// One value per kernel form; public (r3m_debug_wgrad_route), numbered apart from the conv routes (1 - 33).
enum : int {
  WG_TAPS_SIMPLE = 40,   // fp32, one tap per block, rows linear in m (1x1 / stride 1)          wgrad_glds_kernel<.., 32, 1, 0, 1>
  WG_TAPS_GATHER = 41,   // fp32, one tap per block, gathered rows (strided, 7x7, ...)          wgrad_glds_kernel<.., 32, 1, IL, 0>
  WG_ROWS        = 42,   // fp32, one kernel row (three taps) per block                         wgrad_glds_kernel<.., 16, 3, IL>
  WG_WINDOW      = 43,   // fp32 3x3 "same": kernel row from one shared input window            wgrad_rowwin_kernel
  WG16_TAPS      = 50,   // bf16, one tap per block                                             wgrad_bf16_kernel<.., bk>
  WG16_ROWS      = 51,   // bf16, one kernel row per block, 128 x 128 tile                      wgrad_bf16_kernel<128, 128, 32, 3, fast>
  WG16_ALL_TAPS  = 52,   // bf16 3x3 "same" at widths that are multiples of 8: nine taps        wgrad3x3_halo_bf16_kernel
};
// What one launch runs. Template variants inside a form follow from tile (128: IL = 1 on the fp32 gathered / kernel-row forms), bk, fast.
struct WgradPlan {
  int route, tile, bk;           // kernel form, tile width (128 | 64), rows per K step
  int fast;                      // WG16_ROWS: the division-free coordinate walk is enough
  int split, rows_per_split;     // split-K factor, GEMM rows per split
  int tilesN, gx;                // ci tiles, blocks per split: the grid is gx * split
  int lds_bytes;                 // dynamic LDS (0: the kernel's LDS is static)
  int xcd, debug;                // probe-build switches handed to the kernels (WgradParams)
};
WgradPlan wgrad_plan(const WgradParams& p);   // pure: geometry + dtype (+ the switches in probe builds); launches nothing, checks nothing
int launch_wgrad(const WgradParams& p, const WgradPlan& r, hipStream_t s);   // requirements -> switch (r.route) -> one profiler / check_launch tail
int launch_wgrad_reduce(const float* partial, float* dW, long long n, int splitK, int accumulate, hipStream_t s);
int wgrad_debug_occupancy(int* out);     // debug_occupancy's fourth output
// predicates (called from wgrad_plan only) and "launch this instantiation with this plan" helpers (called from launch_wgrad only)
bool wgrad_rowwin_eligible(const WgradParams& p);      // wgrad_win.hip: 3x3 / stride 1 / pad 1, fp32, whole 64- or 128-wide tiles
int wgrad_rowwin_lds_bytes(int tile);
int launch_wgrad_rowwin(const WgradParams& p, const WgradPlan& r, hipStream_t s);
bool wgrad_halo_eligible(const WgradParams& p);        // wgrad_bf16.hip: 3x3 / stride 1 / pad 1 at widths that are multiples of 8
int wgrad_halo_lds_bytes(int W);
int launch_wgrad_bf16(const WgradParams& p, const WgradPlan& r, hipStream_t s);   // the three bf16 forms

// ---- launchers (conv_bf16.hip): bf16 forward / input-gradient gather-GEMM, the bf16 weight images ----
int launch_gather_gemm_bf16(const GatherGemmParams& p, hipStream_t s);
bool gg16_route_builds(int route, int flags);           // whether bf16 route `route` has a kernel for epilogue `flags`
int gg16_route(const GatherGemmParams& p);              // kernel family of a bf16 launch (r3m_debug_conv_route): 30 gather, 31 halo, 32 kernel-row, 33 probe-build persistent kernel
int launch_convert_bf16(const float* src, void* dst, long long n, hipStream_t s);
int launch_transpose_w_bf16(const float* W, void* Wt, int Co, int T, int Ci, hipStream_t s);

// ---- launchers (conv_row16.hip, round 6): persistent kernel-row kernel of the 128-multiple-wide / 64-wide bf16 3x3 / stride-1 launches ----
bool row16_eligible(const GatherGemmParams& p);
int launch_conv3x3_row_bf16(const GatherGemmParams& p, hipStream_t s);
int row16_set_mode(int mode);                           // diagnostic (r3m_debug_set_conv3x3_bf16): 0 = per-tile halo kernels; returns the old value

// ---- launchers (conv_pw16.hip): persistent warp-specialised kernel of the bf16 plans (dense / parity-strided output rows), probe builds ----
#ifdef R3M_PROBES
int pw16_form(const GatherGemmParams& p);               // 0 none, 1 pointwise, 2 gather, 3 gather with strided output rows
int launch_pw16(const GatherGemmParams& p, hipStream_t s);
int pw16_set_mode(int mode);                            // diagnostic (r3m_debug_set_pw16): 0 = per-tile kernels everywhere; returns the old value
#else                                                   // shipped library: the experiment is not compiled in
static inline int pw16_form(const GatherGemmParams&) { return 0; }
static inline int launch_pw16(const GatherGemmParams&, hipStream_t) { return 1; }
static inline int pw16_set_mode(int) { return -1; }
#endif

// ---- launchers of the stem (x/255 -> Normalize -> conv1 7x7/2 pad 3, 3 -> 64): three kernel sets, one device header (stem_dev.h);
// the engine picks the set once per call (engine.hip, struct Stem). w147 / dw147: conv1's weights OHWI [64][7][7][3] ----
struct FrameSource;   // augment_dev.h: raw clips + crop boxes
// stem.hip: fp32 MFMA, 224 x 224 frames; xn = [F][224][224*3] fp32 normalised frames; y / dY fp32 or bf16 (dt)
int launch_stem_prep(const float* x_nchw, float* xn, int F, hipStream_t s);
int launch_stem_prep_crop(const FrameSource& src, float* xn, int F, hipStream_t s);
int launch_stem_fwd(const float* xn, const float* w147, void* y, float* stats, int F, int dt, hipStream_t s);
size_t stem_wgrad_ws_floats();           // the partials only: ws holds 64 * 160 floats more
int launch_stem_wgrad(const float* xn, const void* dY, float* dw147, float* ws, int F, int accumulate, int dt, hipStream_t s);
// stem_bf16.hip: bf16 MFMA, 224 x 224 frames, from a padded bf16 image of the normalised frames
size_t stem_xn16_bytes(int F);
int launch_stem_prep16(const float* x_nchw, void* xn16, int F, hipStream_t s);
int launch_stem_prep16_crop(const FrameSource& src, void* xn16, int F, hipStream_t s);
int launch_stem_fwd16(const void* xn16, const float* w147, void* y, float* stats, int F, hipStream_t s);
size_t stem_wgrad16_ws_floats();
int launch_stem_wgrad16(const void* xn16, const void* dY, float* dw147, float* ws, int F, int accumulate, hipStream_t s);
// stem_dgrad.hip: input gradient at 224 x 224, dz [F,112,112,64] fp32 / bf16 -> dx [F,3,224,224] fp32 NCHW (= or +=)
int launch_stem_input_grad(const void* dz, int dt, const float* w147, float* dx, int F, int accumulate, hipStream_t s);
// stem_gen.hip: frames of any H x W in [STEM_GEN_MIN, STEM_GEN_MAX]; xn = [F][H][W*3] normalised frames, fp32 (dt = DT_F32) or bf16
// (DT_BF16) behind a float pointer
constexpr int STEM_GEN_MIN = 32, STEM_GEN_MAX = 512;
int stem_gen_check(int F, int H, int W);
int launch_stem_prep_gen(const float* x_nchw, float* xn, int F, int H, int W, int dt, hipStream_t s);
int launch_stem_fwd_gen(const float* xn, const float* w147, void* y, float* stats, int F, int H, int W, int dt, hipStream_t s);
size_t stem_wgrad_gen_ws_floats();
int launch_stem_wgrad_gen(const float* xn, const void* dY, float* dw147, float* ws, int F, int H, int W, int accumulate, int dt,
                          hipStream_t s);
int launch_stem_input_grad_gen(const void* dz, int dt, const float* w147, float* dx, int F, int H, int W, int accumulate, hipStream_t s);
int stem_gen_lds(int F, int H, int W, int* fwd, int* wgrad, int* dgrad);

// ---- BatchNorm (bn.hip; the pooled stem tail: bn_pool.hip) ----
// activation tensors are void*: fp32 (dt = DT_F32) or bf16 (DT_BF16); coefficients / partials / statistics are fp32
// One BatchNorm's per-channel vectors, [C] floats each. A by-value kernel argument: the field order is fixed.
struct BnCoef { const float* scale; const float* shift; const float* mean; const float* invstd; const float* c1; const float* c2; };
struct BnCoefOut { float* mean; float* invstd; float* scale; float* shift; };             // what a forward's coefficient pass writes
struct BnBwdOut { float* dgamma; float* dbeta; float* c1; float* c2; int accumulate; };   // what a backward's combine writes (accumulate: sums +=)
// A layer's coefficient block [6][C] = {mean, invstd, scale, shift, c1, c2}: these three know the row order, nobody else does
static inline BnCoef bn_coef_block(const float* k, int C) { return {k + 2LL * C, k + 3LL * C, k, k + C, k + 4LL * C, k + 5LL * C}; }
__host__ __device__ static inline BnCoefOut bn_coef_out(float* k, int C) { return {k, k + C, k + 2LL * C, k + 3LL * C}; }
static inline BnBwdOut bn_bwd_out(float* dgamma, float* dbeta, float* k, int C, int accumulate) {
  return {dgamma, dbeta, k + 4LL * C, k + 5LL * C, accumulate};
}
struct BnScratch { float* partial; double* acc; };   // partial rows [bn_bwd_partial_rows][2][C] (two sets for a pair), acc: bn_acc_bytes(C)
// one BatchNorm of a backward: its input Y, coefficients, where the sums go, dY, and whether the sums are wanted at all
struct BnBwdSide {
  const void* Y; BnCoef K; BnBwdOut out; void* dY; bool sums;
  BnCoef apply_coef() const { BnCoef k = K; k.c1 = out.c1; k.c2 = out.c2; return k; }   // the second pass reads c1 / c2 where the combine wrote them
};
size_t bn_acc_bytes(int C);   // fp64 slice accumulator: [slices <= max(64, min(256, 131072 / C))][2][C]
int bn_bwd_partial_rows(long long rows, int C, int dt);
int bn_debug_geometry(long long rows, int C, int dt, int* out, int cap);   // r3m_debug_bn_geometry: what the launchers pick, nothing launched
int launch_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                          const BnCoefOut& o, int C, hipStream_t s);
// every BatchNorm of a plan at once: offsets into the flat parameter / running-statistics buffers and the arena (floats); a by-value
// kernel argument
struct BnEvalEntry { long long gamma_off, beta_off, rm_off, rv_off, coef_off; int C, blk0; };
struct BnEvalTable { BnEvalEntry e[56]; int n, blocks; };
int launch_bn_eval_coeffs_table(const float* params, const float* bufs, float* arena, const BnEvalTable& t, float eps, hipStream_t s);
// Z = [relu](bn(Y) [+ R]); K2 != null: R is a second raw conv output with its own BatchNorm, Z = [relu](bn(Y) + bn2(R))
int launch_bn_act_fwd(const void* Y, const BnCoef& K, const void* R, const BnCoef* K2, void* Z, long long rows, int C, int relu,
                      unsigned* maskbits, int dt, hipStream_t s);
// The host sequences, one per operation: the engine and the C ABI both run these and launch no backward pass themselves.
// training coefficients: statistics partials of a forward conv -> stats-reduce -> finalize (+ running-statistics update)
int bn_train_coeffs(const float* stats, int stats_rows, long long count, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float momentum, float eps, const BnCoefOut& o, int C, double* acc, hipStream_t s);
// partial rows [prow][2][C] -> dgamma / dbeta / c1 / c2. second_sum_scale = invstd for a dgrad epilogue's rows (EPI_BNRED: sum(g (y - mean)))
int bn_bwd_combine(const float* partial, int prow, long long count, int use_batch_stats, const BnBwdOut& o, const float* second_sum_scale,
                   int C, double* acc, hipStream_t s);
// one BatchNorm(+ReLU / residual mask) backward: first pass (or, fused_rows > 0, the EPI_BNRED rows in `fused`) -> combine -> second
// pass. b.sums / apply: a BatchNorm whose dY nobody reads only forms its sums, one without wanted sums only applies
int bn_bwd(const void* dZ, const void* Zmask, const unsigned* Zbits, const BnBwdSide& b, const float* fused, int fused_rows, bool apply,
           long long rows, int C, int use_batch_stats, const BnScratch& w, int dt, hipStream_t s);
// the two BatchNorms of a downsample block's tail (same masked gradient): one first pass into two partial sets `set_stride` floats
// apart where the kernel exists (bf16, no fused rows), else one after the other; ONE second pass. The joint launches run as long as
// either side needs them (the wanted side sees the kernels of a full backward); the other side only loses its combine.
int bn_bwd_pair(const void* dZ, const unsigned* Zbits, const BnBwdSide& a, const BnBwdSide& b, const float* fused_a, int fused_rows_a,
                bool apply, long long set_stride, long long rows, int C, int use_batch_stats, const BnScratch& w, int dt, hipStream_t s);

// ---- the pooling family (bn_pool.hip) ----
// stem tail fused (Z0 / dZ0 never materialised)
int launch_bn_relu_maxpool_fwd(const void* Y, const BnCoef& K, void* P, unsigned char* amax, int N, int Hi, int Wi, int C, int dt,
                               hipStream_t s);
int bn_bwd_pool_partial_rows(int N, int Hi, int Wi, int C);
int pool_debug_geometry(int N, int Hi, int Wi, int C, int dt, int* out, int cap);   // r3m_debug_pool_geometry: what the launchers pick, nothing launched
// the stem's BatchNorm backward with dZ gathered through the max-pool: reduce_pool -> combine -> apply_pool (b.sums / apply as bn_bwd)
int bn_bwd_pool(const void* dP, const unsigned char* amax, const BnBwdSide& b, bool apply, int N, int Hi, int Wi, int C,
                int use_batch_stats, const BnScratch& w, int dt, hipStream_t s);
int launch_maxpool_fwd(const void* Z, void* P, unsigned char* amax, int N, int Hi, int Wi, int C, int dt, hipStream_t s);
int launch_maxpool_bwd(const void* dP, const unsigned char* amax, void* dZ, int N, int Hi, int Wi, int C, int dt, hipStream_t s);
int launch_avgpool_fwd(const void* X, float* H, int N, int HW, int C, int dt, hipStream_t s);
int launch_avgpool_bwd(const float* dH, void* dX, int N, int HW, int C, int dt, hipStream_t s);

// ---- launchers (feat.hip): stage outputs out of / their gradients into the NHWC arena, fp32 NCHW on the caller's side ----
// out[n][c][p] = (float) z[n][p][c]; g[n][p][c] = store(load(g[n][p][c]) + d[n][c][p]). C a multiple of 64, any H x W.
int launch_feature_export(const void* z_nhwc, float* out_nchw, int N, int H, int W, int C, int dt, hipStream_t s);
int launch_feature_grad_add(const float* d_nchw, void* g_nhwc, int N, int H, int W, int C, int dt, hipStream_t s);

// ---- losses (loss.hip) and optimizers (adam.hip) ----
// N = the reference's num_negatives, 0..16; loss_refused: 0, or 1 with the message set (no HIP call); the launchers do not check again
size_t loss_workspace_floats(int B, int N);
size_t loss_finalize_floats(int B);                          // the leading part of the workspace that launch_loss_finalize reads
int loss_refused(const char* what, int B, int D, int N, float tcnw);
int launch_tcn_lp_loss(const float* alle, const int* perm, const int* iperm, float* dalle, float* ws, int B, int D, int N, int l2dist,
                       float l2w, float l1w, float tcnw, hipStream_t s);
int launch_lang_infonce(const float* scores, const float* mask, float* dscore, float* ws, int B, int N, float langw, hipStream_t s);
int launch_loss_finalize(float* ws, int B, int have_lang, float* metrics, float l2w, float l1w, float tcnw, float langw,
                         hipStream_t s);
// What one optimizer call steps: n disjoint, sorted [off, off + count) ranges of the flat buffers with a step count each (host arrays;
// offsets and counts multiples of 4), and a learning rate and a weight decay per range (lrs / wds) or, where those are null, lr / wd
// for every range. `what` names the call in messages. clip_coef: null, or a device scalar that the gradient is multiplied by.
struct StepRanges {
  const long long *off, *count, *step;
  int n;
  const double *lrs, *wds;
  double lr, wd;
};
int launch_adam(const char* what, float* p, const float* g, float* m, float* v, const StepRanges& r, double beta1, double beta2, double eps,
                int decoupled, float grad_scale, const float* clip_coef, hipStream_t s);
int launch_sgd(const char* what, float* p, const float* g, float* momentum_buf, const StepRanges& r, double momentum, double dampening,
               int nesterov, float grad_scale, const float* clip_coef, hipStream_t s);
// deterministic fp64 sum of squares of the gradients over ranges -> *sqnorm (device), and the clip coefficient from it
size_t grad_sqnorm_workspace_bytes();
int launch_grad_sqnorm_ranges(const float* g, const long long* off, const long long* count, int n_ranges, double* sqnorm, int accumulate,
                              double* ws, hipStream_t s);
int launch_clip_coef(const double* sqnorm, double max_norm, float grad_scale, float* coef_norm, hipStream_t s);

// ---- augmentation (augment.hip) ----
int launch_crop_resize(const void* in, int in_is_u8, const int* boxes, float* out, long long N, int C, int Hi, int Wi, int Ho,
                       int Wo, int frames_per_box, hipStream_t s);
int launch_resize_crop(const void* in, int in_is_u8, float* out, long long N, int C, int Hi, int Wi, int full_Ho, int full_Wo,
                       int top, int left, int Ho, int Wo, hipStream_t s);
int launch_resize_crop_backward(const float* dout, float* din, long long N, int C, int Hi, int Wi, int full_Ho, int full_Wo, int top,
                                int left, int Ho, int Wo, int accumulate, hipStream_t s);

// ---- language-reward head (lang.hip) ----
long long langrew_num_params(int D, int H, int LD);
// the batched step: (6 + 3N) B rows, N = num_negatives; langrew_batch_refused: 0, or 1 with the message set (no HIP call); the two
// launchers below do not check again
int langrew_batch_refused(const char* what, int B, int D, int H, int LD, int N);
size_t langrew_ws_floats(int B, int D, int H, int LD, int N);
int langrew_forward(const float* alle, const float* feats, const int* perm, const float* params, float* scores, float* ws, int B,
                    int D, int H, int LD, int N, int dt, hipStream_t s);
int langrew_backward(const float* dscore, const int* iperm, const float* params, float* grads, float* dalle, float* ws, int B, int D,
                     int H, int LD, int N, int accumulate, int dt, hipStream_t s);
size_t langrew_call_ws_floats(int R, int D, int H, int LD);
int langrew_call_forward(const float* e0, const float* eg, const float* le, const float* params, float* score, float* ws, int R,
                         int D, int H, int LD, hipStream_t s);
int langrew_call_backward(const float* dscore, const float* params, float* grads, float* de0, float* deg, float* dle, float* ws,
                          int R, int D, int H, int LD, int accumulate, hipStream_t s);
// one evaluation without a backward on the few-row kernel (R0: rows of e0 / le, R or 1); the workspace in bytes, 0 for refused dims
size_t langrew_infer_ws_bytes(int R, int D, int H, int LD);
int langrew_infer(const float* e0, const float* eg, const float* le, const float* params, float* score, void* workspace, int R, int R0,
                  int D, int H, int LD, hipStream_t s);

// ---- optional per-kernel-class HIP-event timing (bench.py roofline; off by default, zero cost when off) ----
enum { KC_GEMM_WIDE = 0, KC_GEMM_NARROW = 1, KC_WGRAD_WIDE = 2, KC_WGRAD_NARROW = 3, KC_COUNT = 4 };
void prof_begin(int kclass, double flops, int M, int N, int K, int taps, hipStream_t s);   // start event (no-op when disabled)
void prof_bytes(double bytes);                               // algorithmic HBM bytes of the launch just opened (roofline of the HBM-bound path)
void prof_end(hipStream_t s);                                // records the stop event
bool prof_open();                                            // this thread has a bracket open (the byte count is worth computing)
void prof_abandon();                                         // error path between begin and end: the open bracket is dropped, nothing is counted

}  // namespace r3m
