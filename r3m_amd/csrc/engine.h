// r3m_amd — internal interface of the encoder engine (engine.hip): the plan, its forward / backward, and the convolution launch
// helpers that the C ABI (capi.hip) and the language head (lang.hip) call directly. Not installed; include/r3m_hip.h is the
// public surface.
#pragma once
#include "common.h"

namespace r3m {

// torchvision's output size of a k x k / stride / pad layer, per dimension
static inline int out_dim(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }

// One convolution over N images: input [N,Hi,Wi,Ci] NHWC, weights [Co][k][k][Ci], output [N,Ho(),Wo(),Co]
struct ConvGeom {
  int N, Hi, Wi, Ci, Co, k, stride, pad;
  int Ho() const { return out_dim(Hi, k, stride, pad); }
  int Wo() const { return out_dim(Wi, k, stride, pad); }
  int M() const { return N * Ho() * Wo(); }                                  // rows of the forward GEMM
  long long w_elems() const { return (long long)Co * k * k * Ci; }
  int simple_rows() const { return (k == 1 && stride == 1 && pad == 0) ? 1 : 0; }
};

// EPI_BNRED request of a dgrad (conv_dgrad_launch): the result is the dz of a BatchNorm whose input is Y (same shape as dX);
// partial rows -> `partial`, count -> rows_out
struct BnRedArgs {
  const float* Y;
  const unsigned* bits;      // 1-bit ReLU mask of the BatchNorm(+residual) output, or null: recompute from Y, scale, shift
  const float* scale;
  const float* shift;
  const float* mean;
  float* partial;
  int rows_out;              // partial rows written (all launches of the dgrad)
};

// A stride-2 dgrad runs one launch per output parity class (py, px) of the [Hi][Wi] input-gradient image, each over a dense Hg x Wg
// grid of pixels; a class without pixels (a 1-wide image) has no launch. f(py, px, Hg, Wg) returns non-zero to stop with that value.
template <class F>
static inline int for_each_parity_class(int Hi, int Wi, F&& f) {
  for (int py = 0; py < 2; ++py)
    for (int px = 0; px < 2; ++px) {
      const int Hg = (Hi - py + 1) / 2, Wg = (Wi - px + 1) / 2;
      if (Hg <= 0 || Wg <= 0) continue;
      if (int e = f(py, px, Hg, Wg)) return e;
    }
  return 0;
}

// ---- convolution launches ----
// X / W / Y (and dY / Wt / dX / add0 / add1) are fp32 tensors, or bf16 tensors behind float-typed pointers when dt == DT_BF16
int conv_forward_launch(const float* X, const float* W, float* Y, float* stats, const float* bias, const ConvGeom& c, int flags, int dt,
                        hipStream_t s);
// Inference forward (round 6): the convolution stores [relu]( acc * scale[co] + shift[co] [+ what `out` already holds] ) — eval-mode
// BatchNorm, the residual join and the ReLU in the conv's own store (flags: EPI_AFFINE [| EPI_ACCUM] [| EPI_RELU]).
int conv_forward_launch_affine(const float* X, const float* W, float* out, const float* scale, const float* shift, const ConvGeom& c,
                               int flags, int dt, hipStream_t s);
bool conv_forward_affine_fusable(const ConvGeom& c, int flags, int dt);   // whether that launch's kernel has these epilogues
// dX[N,Hi,Wi,Ci] = dgrad of the convolution given dY[N,Ho,Wo,Co] and Wt[Ci][k*k][Co]; br: also the EPI_BNRED partials
int conv_dgrad_launch(const float* dY, const float* Wt, float* dX, const float* add0, const float* add1, const unsigned* addbits,
                      const ConvGeom& c, int flags, int dt, hipStream_t s, BnRedArgs* br = nullptr);
int conv_wgrad_launch(const float* X, const float* dY, float* dW, float* partial_ws, const ConvGeom& c, int accumulate, int dt,
                      hipStream_t s);
size_t conv_wgrad_ws_floats(const ConvGeom& c, int dt);     // split-K scratch of that launch: plan.split slabs
WgradPlan conv_wgrad_plan(const ConvGeom& c, int dt);       // what conv_wgrad_launch would run (r3m_debug_wgrad_route)

// ---- the small-M split-K forward (conv_small.hip): inference stores only, fp32. A Linear over few rows is the launch of the 1 x 1
// geometry (M, 1, 1, K, N, 1, 1, 0) with a Linear flag set (EPI_BIAS, EPI_BIAS | EPI_RELU, EPI_BIAS | EPI_GELU): `shift` is its bias,
// `scale` is not read. One rule, one planner: the same refusals, take, tile, S and grid for both families (the per-launch A/B of the
// head's and the text model's Linears, profiles/reward_latency.txt, asked for no tighter rule: every launch it takes is faster). ----
constexpr int SMALL_CONV_ROWS_MAX = 1 << 16;   // rows the entry accepts at all
constexpr int SMALL_CONV_SPLIT_MAX = 32;       // most K slices (the last arriver reads that many slabs of its tile serially)
constexpr int SMALL_CONV_TAKE_TILES = 256;     // the routing rule: the launch's tiles fit the 256 CUs in one round (S keeps the grid there) ...
constexpr int SMALL_CONV_TAKE_CHUNKS = 4;      // ... and K is at least this many chunks of 32 (below, a 1 x 1 over 64 channels, both kernels tie)
// What one launch runs: a pure function of the geometry, the flags and the forced split (0 = the rule's). take: the routing rule sends
// this launch here (all zero: the kernel does not take the shape at all). grid = tiles_m * tiles_n * S blocks; slice s covers chunks
// [s * cps, min((s + 1) * cps, nch)) of the taps * Ci / 32 chunks of 32 k.
struct SmallConvPlan { int take, bm, bn, tiles_m, tiles_n, S, cps, nch, grid; };
SmallConvPlan small_conv_plan(const ConvGeom& c, int flags, int split);
int small_conv_max_split(const ConvGeom& c);
bool small_linear_flags(int flags);                                      // one of the three Linear flag sets
const char* small_conv_refuses(const ConvGeom& c, int flags);            // null, or why the kernel does not take the launch at all
// ctr: the launch's zeroed tickets, slabs: its slab area (both may be null when the plan has one slice)
int launch_conv_small(const float* x, const float* w, float* out, const float* scale, const float* shift, const ConvGeom& c, int flags,
                      int split, unsigned* ctr, float* slabs, hipStream_t s);

int launch_bias_gelu(float* x, const float* bias, long long rows, int C, hipStream_t s);   // text.hip: x = gelu(x + bias[col]) in place

// The split-K workspace of ONE call (a forward of the encoder, of the reward head, of the text model, or a single launch): the ordered
// list of the call's launches, run `reps` times over (the text model's four Linears, once per layer). The rule, stated here once:
//   [ticket blocks in launch order: repetition 0's entries, repetition 1's, ...][one slab area]
// a ticket block (one ticket per tile, padded to 256 bytes) belongs to exactly one launch, reset() zeroes all of them with ONE memset
// ahead of the first launch, and the slab area is shared, sized for the largest launch: the launches are ordered on the stream.
// An entry the set does not run on the kernel has no ticket block and leaves the slab size alone; its caller runs the ordinary kernel.
// Plain data of fixed capacity: building one on the stack per call allocates nothing.
// SmallRoute says which entries run on the kernel: those the routing rule takes (small_conv_plan(...).take), every one the kernel accepts at all (the
// single-launch C entries), or none (the caller's ordinary path through the same code)
enum SmallRoute { SMALL_BY_RULE = 0, SMALL_FORCED = 1, SMALL_NEVER = 2 };
struct SmallLaunchSet {
  static constexpr int CAP = 56;                      // a ResNet-50 has 53 convolutions (BnEvalTable has the same room)
  struct Entry { ConvGeom g; int flags, split; bool run; int S; size_t ctr, ctr_off; };   // run: on the kernel, in S slices, with ctr ticket bytes
  Entry e[CAP];
  int n = 0, reps = 1;
  size_t ctr_bytes = 0, slab_bytes = 0;               // tickets of one repetition; the slab area
  // appends a launch and returns its index; past CAP entries it returns -1 and the launch is not run here
  int add(const ConvGeom& g, int flags, int split = 0, SmallRoute route = SMALL_BY_RULE);
  bool runs(int i) const { return i >= 0 && i < n && e[i].run; }
  size_t ticket_bytes() const { return ctr_bytes * reps; }
  size_t bytes() const { return ticket_bytes() + slab_bytes; }
  // the single memset (none when no entry has tickets); non-zero when it fails, the caller names the call in its error
  int reset(void* base, hipStream_t s) const;
  // entry i of repetition rep on the kernel, with its own ticket block and the shared slab area; flags >= 0: another store of the
  // same family than the entry was planned with (the plan does not depend on which)
  int launch(int i, int rep, void* base, const float* x, const float* w, float* out, const float* scale, const float* shift,
             hipStream_t s, int flags = -1) const;
  // y = store(x w^T + bias) of Linear entry i: launch() when the set runs it, else the ordinary launches — conv_forward_launch with
  // the entry's flags, and for EPI_BIAS | EPI_GELU the plain GEMM followed by launch_bias_gelu
  int linear(int i, int rep, void* base, const float* x, const float* w, const float* bias, float* y, hipStream_t s) const;
};

// ---- the plan ----
struct Plan;
struct FrameSource;   // augment_dev.h: raw clips + crop boxes
Plan* plan_create(int size, int F, int dtype, int H, int W);
void plan_destroy(Plan* P);
// frames come either as [F,3,H,W] fp32 0..255 (x_nchw, crop == nullptr) or as raw clips + crop boxes (crop: rc / rctraj resampled
// inside the stem pre-pass; 224 x 224 plans only)
// feats (optional): feats[k-1] != null receives torchvision layer`k`'s output as fp32 NCHW [F, C_k, H_k, W_k] (plan_feature_info),
// exported right behind the stage's last block on s; frames through x_nchw only
int plan_forward(Plan& P, const float* x_nchw, const FrameSource* crop, const float* params, float* bufs, float* arena, float* h_out,
                 int training, hipStream_t s, float* const* feats = nullptr);
// prepared inference (engine.hip): coefficients (bf16: weight image) once, then forwards without the per-layer coefficient launches;
// flags bit 0: no launch goes to conv_small.hip
int plan_inference_prepare(Plan& P, const float* params, const float* bufs, float* arena, hipStream_t s);
long long plan_inference_workspace_bytes(Plan* P);
int plan_forward_prepared(Plan& P, const float* x_nchw, const float* params, float* arena, void* workspace, float* h_out, float* const* feats,
                          int flags, hipStream_t s);
// dh == nullptr: the embedding received no gradient. dfeats (optional): dfeats[k-1] != null is the gradient w.r.t. that output of
// the forward, fp32 NCHW; every staged call carries the same array, the stage that owns an entry (stage 4 - k) reads it
int plan_backward(Plan& P, const float* dh, const float* params, float* grads, float* arena, int stage_begin, int stage_end,
                  int accumulate, hipStream_t s, float* dx, int dx_accumulate, const float* const* dfeats = nullptr);
int plan_feature_info(Plan* P, int layer, int* C, int* H, int* W);
int plan_out_dim(Plan* P);
int plan_input_hw(Plan* P, int* H, int* W);
int plan_num_convs(Plan* P);
int plan_conv_info(Plan* P, int i, int* geo10);
long long plan_coef_offset(Plan* P, int i);   // arena offset (floats) of convolution i's coefficient block [6][Co]
int plan_dtype(Plan* P);
long long plan_num_params(Plan* P);
long long plan_num_buffers(Plan* P);
long long plan_arena_floats(Plan* P);
int plan_num_tensors(Plan* P);
int plan_tensor_info(Plan* P, int i, char* name, int cap, int* kind, long long* offset, int* ndim, int* shape4);
int plan_stage_range(Plan* P, int stage, long long* off, long long* count);
// partial freeze: one byte per tensor (plan_tensor_info order; nullptr = all trainable), and the per-convolution work of a backward
// under it (BW_* bits) from the predicate plan_backward executes
enum { BW_BN_SUMS = 1, BW_BN_APPLY = 2, BW_DGRAD = 4, BW_WGRAD = 8 };
int plan_set_trainable(Plan* P, const unsigned char* mask, int n);
int plan_debug_backward(Plan* P, int want_dx, int* flags_out, int cap);
// per-plan options; each returns the old value
int plan_set_bn_pair(Plan* P, int on);      // the two tail BatchNorms of a downsample block share their backward passes
int plan_set_fuse_bnred(Plan* P, int on);   // 1 = BatchNorm-backward partials from the dgrad epilogues (EPI_BNRED), 0 = stand-alone reduce passes

// ---- process-wide diagnostic switches (r3m_debug_set_*); each returns the old value ----
int engine_set_generic_stem(int on);      // 1 = 224 x 224 frames run the general stem kernels too (tests, A/B)
int engine_set_fused_inference(int on);   // 0 = inference forwards run the unfused eval sequence (A/B, tests)

}  // namespace r3m
