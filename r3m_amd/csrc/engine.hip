// r3m_amd — the ResNet-18/34/50 encoder engine: a native plan (layer table + HBM arena layout) and the forward /
// backward launch sequences, all on one caller-supplied HIP stream. This is the from-scratch counterpart of what the
// reference obtains from torchvision.models.resnet{18,34,50}(pretrained=False) with fc = Identity, driven by
// R3M.forward (/root/reference/r3m/models/models_r3m.py:44-52,62,84-100) and autograd's backward
// (/root/reference/r3m/trainer.py:157). Architecture restated from SURVEY.md Appendix A (torchvision 0.8.2 is not
// vendored): stem 7x7/2 + BN + ReLU + maxpool 3x3/2, BasicBlock [2,2,2,2] / [3,4,6,3] or Bottleneck v1.5 [3,4,6,3],
// global average pool, flatten.
//
// HBM layout: activations NHWC fp32 in ONE arena owned by the caller (offsets fixed at plan creation, sized for the
// frame count F); parameters and gradients are two flat fp32 buffers in torchvision parameter order with conv weights
// stored OHWI (= logical OIHW tensors with channels_last strides, so state-dict interchange needs no copy kernels).
//
// File order: the layer table and Plan (layout, options, RunState) -> plan_create -> the convolution launch helpers of engine.h ->
// Ctx (one call's view of plan + buffers) and the tile-counter guard -> forward (stem_forward, block_forward, block_forward_fused,
// plan_forward, forward_sequence; prepared inference: plan_inference_prepare, plan_forward_prepared) -> backward (BatchNorm / dgrad / wgrad helpers, SideStream, block_backward, stem_backward, plan_backward) -> accessors.
// The BatchNorm helpers only pick pointers, gradient destinations and work bits: the launch sequences themselves (bn_train_coeffs, bn_bwd,
// bn_bwd_pair, bn_bwd_pool) are in bn.hip / bn_pool.hip, shared with the C ABI.
#include "engine.h"
#include "augment_dev.h"
#ifndef R3M_BN_PAIR_DEFAULT
#define R3M_BN_PAIR_DEFAULT 1     // A/B builds: tools/build_ab.sh none variant nopair -DR3M_BN_PAIR_DEFAULT=0
#endif
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace r3m {

struct ConvSpec {
  std::string name;      // e.g. "layer1.0.conv1" ; BatchNorm is name_bn
  std::string bn_name;
  int Ci, Co, k, stride, pad;
  int Hi, Wi, Ho, Wo;
  long long w_off, gamma_off, beta_off;   // flat parameter / gradient buffer (floats)
  long long rm_off, rv_off;               // flat running-statistics buffer (floats)
  long long Y_off;                        // arena: raw conv output [F,Ho,Wo,Co]
  long long Z_off;                        // arena: activated output, -1 when the block epilogue produces it
  long long coef_off;                     // arena: mean, invstd, scale, shift, c1, c2  (6*Co floats)
  int stats_rows;                         // row blocks of the forward GEMM (BatchNorm partials)
  long long wt_off = 0;                   // dgrad weight image [Ci][k*k][Co] inside the plan's Wt region (elements of the activation type)
  ConvGeom geom(int F) const { return {F, Hi, Wi, Ci, Co, k, stride, pad}; }
};

struct BlockSpec {
  int conv[3];
  int nconv;
  int ds;                 // downsample conv index or -1
  long long in_off;       // arena offset of the block input
  long long out_off;      // arena offset of the block output
  long long mask_off;     // arena offset of the block output's 1-bit ReLU mask (rows*C/32 words)
  int Ho, Wo, Co;
  int stage;              // 0..3 = layer1..layer4
};

struct TensorInfo {
  std::string name;
  int kind;               // 0 conv weight, 1 bn weight, 2 bn bias, 3 running_mean, 4 running_var
  long long offset;       // floats, in the params buffer (kind 0-2) or the buffers buffer (kind 3-4)
  int shape[4];           // logical shape (conv: O, I, kh, kw)
  int ndim;
};

struct Ctx;

// The opt-in side stream of a backward: wgrad(L) only needs dY_L and the saved activations, and nothing on the critical path needs its
// result before the optimizer. It runs on a side stream, ordered by events so that it overlaps ONLY with the HBM-bound
// BatchNorm-backward passes of the next layer down (reduce / apply: ~6 TB/s, no MFMA) and never with the MFMA-bound dgrad:
//     main:  bn_bwd(L) -> [wait wgrad(L+1)] -> dgrad(L) -> bn_bwd(L-1) -> [wait wgrad(L)] -> dgrad(L-1) -> ...
//     side:                                    wgrad(L)  (starts when dgrad(L) has finished)
// A bandwidth-bound and a matrix-bound kernel share the CUs without stealing each other's bottleneck resource, and the
// per-launch timings of the dominant kernel class (gather-GEMM on the main stream) stay unperturbed. Each stage ends with
// a join. Off by default (probe builds: R3M_SIDE_STREAM=1 enables it, 2 = wgrad(L) runs beside dgrad(L)): measured neutral, see init().
// Every method does nothing (wgrad_async: launches on the main stream) while it is off.
struct SideStream {
  int init();                                   // reads the mode once; creates the stream and events when it is on
  void begin(hipStream_t s, bool have_grads) { main = s; on = mode && side && have_grads; }   // per plan_backward call
  void restart() { pending[0] = pending[1] = false; }                                         // stage 0: nothing in flight
  int mark_dy();                                // the side stream waits for what the main stream has enqueued so far (dY_L)
  int wgrad_async(Ctx& c, const ConvSpec& L, const float* X, const float* dY, int ai);   // right AFTER dgrad(L) was enqueued; dY is A[ai]
  int acquire(int ai);                          // before the main stream overwrites A[ai], the wgrad that last read it must be done
  int wait_wgrads();                            // before an MFMA-bound kernel goes to the main stream: every wgrad in flight must have finished
  int join();                                   // the main stream waits for everything on the side stream
  void destroy();
 private:
  int mode = -1;
  bool on = false;
  hipStream_t main = nullptr, side = nullptr;
  hipEvent_t ev_dy = nullptr, ev_wg[2] = {nullptr, nullptr}, ev_join = nullptr;
  bool pending[2] = {false, false};             // a wgrad reading A0 / A1 is in flight
};

// What forward and backward change on a plan. Backward stages carry state from one r3m_resnet_backward call to the next (buffer
// roles, the running output gradient and — with EPI_BNRED — BatchNorm partials waiting in the shared partial buffer for the NEXT
// block). They are only valid in the order 0,1,2,3 after ONE forward.
struct RunState {
  int last_training = 1;
  int last_crop = 0;        // the last forward read raw clips through crop boxes (r3m_resnet_forward_crop): no frames to differentiate
  int stem_gen = 0;         // the last forward ran the general stem (stem_gen.hip): its backward must too (the normalised image layout)
  int next_stage = -1;      // what the following backward call must begin with (0 = a backward may (re)start, -1 = no forward has run yet)
  int roles[5] = {0, 1, 2, 3, 4};   // which G buffer is D (block output grad), A0 / A1 (dY, alternating), B, C: rotated per block
  int a_next = 0;           // which of A0/A1 the next dY goes to
  int dout_fused_rows = 0;  // > 0: the dgrad that wrote the running output gradient also wrote the BatchNorm-backward partials of the
                            // block that consumes it next (EPI_BNRED): that many partial rows wait in the partial buffer
  std::vector<int> work;    // BW_* bits per convolution of the running backward (backward_work, fixed by the call that ran stage 0)
  std::vector<unsigned char> mask;   // the trainable mask that backward runs under (one byte per tensor; empty: all trainable)
  WtEntry* d_wt_tab = nullptr;      // device copies of wt_tab / wt_tile0, made at the first backward (plan creation needs no GPU)
  int* d_wt_tile0 = nullptr;
  SideStream side;
  const float* prepared = nullptr;   // the arena whose coefficient blocks (bf16: weight image too) plan_inference_prepare filled and no
                                     // other forward of this plan has touched since; null: plan_forward_prepared refuses
};

// Layout (set by plan_create; forward and backward see it const), two options, and the run state.
struct Plan {
  int size, F, D;
  int H = 224, W = 224;   // input frames [F,3,H,W]
  int H1 = 112, W1 = 112; // stem output (conv1), the maxpool's input
  int Hp = 56, Wp = 56;   // maxpool output, layer1's input
  int dtype = DT_F32;     // activation storage: fp32, or bf16 (bf16 conv operands, fp32 accumulation / statistics / gradients of weights)
  long long w16_off = 0;  // arena: bf16 image of the flat parameter buffer (DT_BF16 only)
  std::vector<ConvSpec> convs;
  std::vector<BlockSpec> blocks;
  std::vector<TensorInfo> tensors;
  long long n_params = 0, n_buffers = 0;
  long long stage_param_begin[5];  // params of stem+layer1 | layer2 | layer3 | layer4 boundaries (see stage_range)
  // arena offsets (floats)
  long long col_off, P0_off, amax_off, partial_off, acc_off, wt_off, wgp_off;
  long long ctr_off = 0;    // per-XCD tile queues of the persistent kernel (TileCounters)
  long long G_off[5];     // gradient ping-pong buffers: D (block output grad), A0/A1 (dY, alternating), B, C
  long long E_off = -1;   // dY of a downsample block's downsample BatchNorm: written with the block's last BatchNorm backward (one pass
                          // for both, bn_backward_pair), read by the downsample dgrad / wgrad at the END of the block (-1: no such block)
  long long arena_floats = 0;
  long long gmax = 0;
  long long gsc_off = 0;  // arena: [2][2048] BatchNorm parameter-gradient sums of a backward without parameter gradients (grads == NULL)
  // dgrad weight images of all layers, rebuilt by ONE launch at the start of each backward (launch_transpose_w_all)
  std::vector<WtEntry> wt_tab;
  std::vector<int> wt_tile0;
  long long wt_elems = 0;
  // options (plan_set_*)
  int fuse_bnred = 1;       // BatchNorm-backward partials from the producing dgrad's epilogue (EPI_BNRED); 0: stand-alone reduce pass
  // the small-M kernel (conv_small.hip) in a prepared forward: entry i is convolution i, on the caller's workspace (fp32 plans; empty otherwise)
  SmallLaunchSet small;
  std::vector<unsigned char> trainable;   // plan_set_trainable: one byte per tensor, empty = all trainable (read by the next stage 0)
  int bn_pair = R3M_BN_PAIR_DEFAULT;   // the two tail BatchNorms of a downsample block share their backward passes (bn_backward_pair); 0: separate passes
  RunState run;
};

static long long align64(long long x) { return (x + 63) / 64 * 64; }

static int add_conv(Plan& P, const std::string& name, const std::string& bn, int Ci, int Co, int k, int stride, int pad,
                    int Hi, int Wi) {
  ConvSpec c;
  c.name = name; c.bn_name = bn;
  c.Ci = Ci; c.Co = Co; c.k = k; c.stride = stride; c.pad = pad; c.Hi = Hi; c.Wi = Wi;
  c.Ho = out_dim(Hi, k, stride, pad);
  c.Wo = out_dim(Wi, k, stride, pad);
  c.w_off = P.n_params;
  P.n_params += (long long)Co * Ci * k * k;
  c.gamma_off = P.n_params; P.n_params += Co;
  c.beta_off = P.n_params; P.n_params += Co;
  c.rm_off = P.n_buffers; P.n_buffers += Co;
  c.rv_off = P.n_buffers; P.n_buffers += Co;
  TensorInfo t;
  t.name = name + ".weight"; t.kind = 0; t.offset = c.w_off; t.ndim = 4;
  t.shape[0] = Co; t.shape[1] = Ci; t.shape[2] = k; t.shape[3] = k;
  P.tensors.push_back(t);
  t.ndim = 1; t.shape[0] = Co; t.shape[1] = t.shape[2] = t.shape[3] = 1;
  t.name = bn + ".weight"; t.kind = 1; t.offset = c.gamma_off; P.tensors.push_back(t);
  t.name = bn + ".bias"; t.kind = 2; t.offset = c.beta_off; P.tensors.push_back(t);
  t.name = bn + ".running_mean"; t.kind = 3; t.offset = c.rm_off; P.tensors.push_back(t);
  t.name = bn + ".running_var"; t.kind = 4; t.offset = c.rv_off; P.tensors.push_back(t);
  c.Y_off = c.Z_off = c.coef_off = -1;
  c.stats_rows = 0;
  P.convs.push_back(c);
  return (int)P.convs.size() - 1;
}

static int g_generic_stem = 0;      // r3m_debug_set_generic_stem
int engine_set_generic_stem(int on) { const int old = g_generic_stem; g_generic_stem = on ? 1 : 0; return old; }

// ---- the stem: the kernel set one call runs, its image and workspace sizes, and its four operations ----
// 224 x 224 frames run stem.hip (fp32 plans) or stem_bf16.hip (bf16 plans) with stem_dgrad.hip; every other size, and 224 under
// r3m_debug_set_generic_stem, the general kernels of stem_gen.hip. The sets keep different normalised images (xn), so the backward
// runs the set its forward chose (RunState::stem_gen).
enum StemSet { STEM_224_F32, STEM_224_BF16, STEM_GEN };
struct Stem {
  StemSet set;
  int F, H, W, dt;
  hipStream_t s;
  Stem(const Plan& P, int dt, bool gen, hipStream_t s)
      : set(gen ? STEM_GEN : dt == DT_BF16 ? STEM_224_BF16 : STEM_224_F32), F(P.F), H(P.H), W(P.W), dt(dt), s(s) {}
  // arena floats of the normalised image: fp32 channel-interleaved rows, the padded bf16 image of stem_bf16.hip, or the general
  // stem's plain [F][H][W*3] rows in the plan's precision
  static long long image_floats(StemSet set, long long F, int H, int W, int dt) {
    if (set == STEM_224_BF16) return (long long)((stem_xn16_bytes((int)F) + 3) / 4);
    return set == STEM_GEN && dt == DT_BF16 ? (F * 3 * H * W + 1) / 2 : F * 3 * H * W;
  }
  static long long wgrad_ws_floats(StemSet set) {
    if (set == STEM_GEN) return (long long)stem_wgrad_gen_ws_floats();
    return set == STEM_224_BF16 ? (long long)stem_wgrad16_ws_floats() : (long long)stem_wgrad_ws_floats() + 64 * 160;
  }
  // what a plan reserves: the larger of what the sets it may run need — the general set always (at 224 under
  // r3m_debug_set_generic_stem), the 224 set of the plan's precision at 224
  static long long plan_image_floats(bool is224, long long F, int H, int W, int dt) {
    const long long n = image_floats(STEM_GEN, F, H, W, dt);
    return is224 ? std::max(n, image_floats(dt == DT_BF16 ? STEM_224_BF16 : STEM_224_F32, F, H, W, dt)) : n;
  }
  static long long plan_wgrad_ws_floats(bool is224, int dt) {
    const long long n = wgrad_ws_floats(STEM_GEN);
    return is224 ? std::max(n, wgrad_ws_floats(dt == DT_BF16 ? STEM_224_BF16 : STEM_224_F32)) : n;
  }
  // frames (or, 224 sets only, the raw clips through their crop boxes) -> xn
  int prep(const float* x_nchw, const FrameSource* crop, float* xn) const {
    switch (set) {
      case STEM_GEN: return launch_stem_prep_gen(x_nchw, xn, F, H, W, dt, s);
      case STEM_224_BF16: return crop ? launch_stem_prep16_crop(*crop, xn, F, s) : launch_stem_prep16(x_nchw, xn, F, s);
      default: return crop ? launch_stem_prep_crop(*crop, xn, F, s) : launch_stem_prep(x_nchw, xn, F, s);
    }
  }
  int forward(const float* xn, const float* w, float* Y, float* stats) const {
    switch (set) {
      case STEM_GEN: return launch_stem_fwd_gen(xn, w, Y, stats, F, H, W, dt, s);
      case STEM_224_BF16: return launch_stem_fwd16(xn, w, Y, stats, F, s);
      default: return launch_stem_fwd(xn, w, Y, stats, F, dt, s);
    }
  }
  int wgrad(const float* xn, const float* dY, float* dw, float* ws, int accumulate) const {
    switch (set) {
      case STEM_GEN: return launch_stem_wgrad_gen(xn, dY, dw, ws, F, H, W, accumulate, dt, s);
      case STEM_224_BF16: return launch_stem_wgrad16(xn, dY, dw, ws, F, accumulate, s);
      default: return launch_stem_wgrad(xn, dY, dw, ws, F, accumulate, dt, s);
    }
  }
  int input_grad(const float* dY, const float* w, float* dx, int accumulate) const {
    if (set == STEM_GEN) return launch_stem_input_grad_gen(dY, dt, w, dx, F, H, W, accumulate, s);
    return launch_stem_input_grad(dY, dt, w, dx, F, accumulate, s);
  }
};
static int g_fused_inference = 1;   // r3m_debug_set_fused_inference
int engine_set_fused_inference(int on) { const int old = g_fused_inference; g_fused_inference = on ? 1 : 0; return old; }

Plan* plan_create(int size, int F, int dtype, int H, int W) {
  if (size != 18 && size != 34 && size != 50) { set_last_error("resnet: unsupported size %d (18, 34, 50)", size); return nullptr; }
  if (dtype != DT_F32 && dtype != DT_BF16) { set_last_error("resnet: unsupported dtype %d (0 fp32, 1 bf16)", dtype); return nullptr; }
  if (F < 1) { set_last_error("resnet: F=%d must be >= 1", F); return nullptr; }
  if (H < STEM_GEN_MIN || W < STEM_GEN_MIN || H > STEM_GEN_MAX || W > STEM_GEN_MAX) {
    set_last_error("resnet: frames %d x %d outside the supported %d..%d per side (below %d a stem tile could span more than two "
                   "frames; above %d the general stem's staged rows leave the 160 KiB LDS of a CU)", H, W, STEM_GEN_MIN, STEM_GEN_MAX,
                   STEM_GEN_MIN, STEM_GEN_MAX);
    return nullptr;
  }
  Plan* Pp = new Plan();
  Plan& P = *Pp;
  P.size = size; P.F = F; P.dtype = dtype;
  P.H = H; P.W = W;
  P.H1 = out_dim(H, 7, 2, 3); P.W1 = out_dim(W, 7, 2, 3);
  P.Hp = out_dim(P.H1, 3, 2, 1); P.Wp = out_dim(P.W1, 3, 2, 1);
  const bool is224 = H == 224 && W == 224;
  // fp32 plans only: there the dgrad is MFMA-bound and the extra epilogue loads ride under other blocks' matrix work (A/B on one
  // box, probe build: 343.0 / 341.7 ms -> 338.5 / 339.0 ms per ResNet-50 step). bf16 plans are HBM/epilogue-bound already and
  // measured slightly SLOWER with it (ResNet-50 95.6 -> 96.2 ms, ResNet-34 97.0 -> 97.9 ms), so they keep the stand-alone reduce.
  P.fuse_bnred = dtype == DT_F32 ? 1 : 0;
  if (const int v = R3M_ENV_INT("R3M_BNRED", 1); v != 1) P.fuse_bnred = v == 2;   // probe builds: 0 = off everywhere, 2 = on for bf16 too
  const bool bottleneck = (size == 50);
  const int expansion = bottleneck ? 4 : 1;
  const int nblk[4] = {size == 18 ? 2 : 3, size == 18 ? 2 : 4, size == 18 ? 2 : 6, size == 18 ? 2 : 3};
  P.D = 512 * expansion;

  // ---- layer table in torchvision parameter order ----
  add_conv(P, "conv1", "bn1", 3, 64, 7, 2, 3, H, W);
  P.stage_param_begin[0] = 0;
  int inC = 64, Hc = P.Hp, Wc = P.Wp;
  for (int L = 0; L < 4; ++L) {
    const int planes = 64 << L;
    if (L > 0) P.stage_param_begin[L] = P.n_params;
    for (int b = 0; b < nblk[L]; ++b) {
      const int stride = (b == 0 && L > 0) ? 2 : 1;
      char pre[64];
      snprintf(pre, sizeof pre, "layer%d.%d", L + 1, b);
      const std::string p(pre);
      BlockSpec B;
      B.stage = L; B.ds = -1;
      const int Hout = out_dim(Hc, 3, stride, 1), Wout = out_dim(Wc, 3, stride, 1);   // == the 1x1 / stride downsample's
      if (bottleneck) {
        B.nconv = 3;
        B.conv[0] = add_conv(P, p + ".conv1", p + ".bn1", inC, planes, 1, 1, 0, Hc, Wc);
        B.conv[1] = add_conv(P, p + ".conv2", p + ".bn2", planes, planes, 3, stride, 1, Hc, Wc);
        B.conv[2] = add_conv(P, p + ".conv3", p + ".bn3", planes, planes * 4, 1, 1, 0, Hout, Wout);
      } else {
        B.nconv = 2;
        B.conv[0] = add_conv(P, p + ".conv1", p + ".bn1", inC, planes, 3, stride, 1, Hc, Wc);
        B.conv[1] = add_conv(P, p + ".conv2", p + ".bn2", planes, planes, 3, 1, 1, Hout, Wout);
        B.conv[2] = -1;
      }
      if (stride != 1 || inC != planes * expansion)
        B.ds = add_conv(P, p + ".downsample.0", p + ".downsample.1", inC, planes * expansion, 1, stride, 0, Hc, Wc);
      B.Ho = Hout; B.Wo = Wout; B.Co = planes * expansion;
      P.blocks.push_back(B);
      inC = planes * expansion; Hc = Hout; Wc = Wout;
    }
  }
  P.stage_param_begin[4] = P.n_params;
  if (!is224) {
    // Native-resolution plans (224 plans are as they always were). The binding 32-bit index is the GEMM row count M = F Ho Wo: an
    // int in GatherGemmParams / WgradParams, the row index of gg_epilogue and the general stem's tile origin (stem_gen.hip,
    // m0 = tile * 256, which must stay below 2^31 after rounding up to 256 rows). Element offsets are formed in 64 bits there, but
    // no kernel has run on a tensor of 2^31 elements or more (the largest 224 plan, ResNet-50 x 1280 frames, reaches 1.03e9), so
    // such plans are refused too rather than trusted.
    long long most_m = 0, most_e = (long long)F * 3 * H * W;
    std::string what_m, what_e = "the input frames";
    for (const ConvSpec& c : P.convs) {
      const long long m = (long long)F * c.Ho * c.Wo;
      const long long n = std::max((long long)F * c.Hi * c.Wi * c.Ci, m * c.Co);
      if (m > most_m) { most_m = m; what_m = c.name; }
      if (n > most_e) { most_e = n; what_e = c.name; }
    }
    if (most_m > 0x7fffffffLL - 256) {
      set_last_error("resnet: %d frames of %d x %d give %lld GEMM rows at %s: GatherGemmParams::M, WgradParams::M and the stem's "
                     "tile index are 32-bit (limit 2^31 - 257); use fewer frames per plan", F, H, W, most_m, what_m.c_str());
      delete Pp;
      return nullptr;
    }
    if (most_e > 0x7fffffffLL) {
      set_last_error("resnet: %d frames of %d x %d give %lld elements at %s: tensors of 2^31 elements or more are not supported "
                     "(32-bit index range); use fewer frames per plan", F, H, W, most_e, what_e.c_str());
      delete Pp;
      return nullptr;
    }
  }

  // ---- arena layout ----
  long long off = 0;
  auto take = [&](long long n) { long long o = off; off = align64(off + n); return o; };
  const long long Fll = F;
  // arena offsets are in floats whatever the storage type; a bf16 tensor of n elements takes n/2 of them
  auto act = [&](long long n) { return dtype == DT_BF16 ? (n + 1) / 2 : n; };
  // private normalised copy of the input frames (the stem's weight gradient re-reads it in backward)
  P.col_off = take(Stem::plan_image_floats(is224, Fll, H, W, dtype));
  long long gmax = 0, partial_max = 0, wmax = 0, wgp_max = 0;
  auto act_elems = [&](const ConvSpec& c) { return Fll * c.Ho * c.Wo * c.Co; };
  for (size_t i = 0; i < P.convs.size(); ++i) {
    ConvSpec& c = P.convs[i];
    c.Y_off = take(act(act_elems(c)));
    c.coef_off = take(6LL * c.Co);
    if (act(act_elems(c)) > gmax) gmax = act(act_elems(c));
    const int M = F * c.Ho * c.Wo;
    c.stats_rows = gather_gemm_grid_m(M, c.Co);
    long long pr = (long long)c.stats_rows * 2 * c.Co;
    if (pr > partial_max) partial_max = pr;
    pr = (long long)(i == 0 ? bn_bwd_pool_partial_rows(F, c.Ho, c.Wo, c.Co) : bn_bwd_partial_rows(M, c.Co, dtype)) * 2 * c.Co;
    if (pr > partial_max) partial_max = pr;
    pr *= 2;                                                    // two sets: the paired first pass of a downsample block's tail (bn_backward_pair)
    if (i > 0 && pr > partial_max) partial_max = pr;
    pr = ((long long)bnred_partial_rows(M) + 4) * 2 * c.Co;     // EPI_BNRED: one row per 64 result rows (+ one per stride-2 parity class)
    if (pr > partial_max) partial_max = pr;
    const long long welems = (long long)c.Co * c.k * c.k * c.Ci;
    if (welems > wmax) wmax = welems;
    if (i == 0) {
      wgp_max = std::max(wgp_max, Stem::plan_wgrad_ws_floats(is224, dtype));
    } else {
      wgp_max = std::max(wgp_max, (long long)conv_wgrad_ws_floats(c.geom(F), dtype));
    }
  }
  // stem: P0 (pooled) and the argmax bytes; the pre-pool activation Z0 is never materialised (bn_pool.hip: fused stem tail)
  P.P0_off = take(act(Fll * P.Hp * P.Wp * 64));
  P.amax_off = take((Fll * P.Hp * P.Wp * 64 + 3) / 4);
  long long cur_in = P.P0_off;
  for (auto& B : P.blocks) {
    B.in_off = cur_in;
    for (int j = 0; j < B.nconv - 1; ++j) P.convs[B.conv[j]].Z_off = take(act(act_elems(P.convs[B.conv[j]])));
    B.out_off = take(act(Fll * B.Ho * B.Wo * B.Co));
    B.mask_off = take((Fll * B.Ho * B.Wo * B.Co + 31) / 32);
    cur_in = B.out_off;
  }
  P.partial_off = take(partial_max);
  P.acc_off = take(64LL * 2 * 2048 * 2);  // doubles: 64 slices x 2 x Cmax, in float units x2
  {   // one dgrad weight image per conv layer after the stem (the stem has no input gradient)
    int tiles = 0;
    long long we = 0;
    for (size_t i = 1; i < P.convs.size(); ++i) {
      ConvSpec& c = P.convs[i];
      c.wt_off = we;
      P.wt_tab.push_back(WtEntry{c.w_off, we, c.Co, c.k * c.k, c.Ci, 0});
      P.wt_tile0.push_back(tiles);
      tiles += ceil_div(c.Ci, 32) * ceil_div(c.Co, 32) * c.k * c.k;
      we += align64((long long)c.Co * c.k * c.k * c.Ci);
    }
    P.wt_tile0.push_back(tiles);
    P.wt_elems = we;
    P.wt_off = take(dtype == DT_BF16 ? (we + 1) / 2 : we);
  }
  if (dtype == DT_BF16) P.w16_off = take((P.n_params + 1) / 2);
  P.wgp_off = take(wgp_max);
  P.gsc_off = take(2LL * 2048);
  P.ctr_off = take(5LL * (long long)P.convs.size() * 8);
  P.gmax = gmax;
  for (int g = 0; g < 5; ++g) P.G_off[g] = take(gmax);
  {
    long long emax = 0;
    for (size_t bi = 0; bi < P.blocks.size(); ++bi)
      if (P.blocks[bi].ds >= 0) emax = std::max(emax, act(Fll * P.blocks[bi].Ho * P.blocks[bi].Wo * P.blocks[bi].Co));
    if (emax > 0) P.E_off = take(emax);
  }
  P.arena_floats = off;
  if (dtype == DT_F32)   // the plan does not depend on which of the three stores the launch makes; the stem (entry 0) is never a launch of the set
    for (size_t i = 0; i < P.convs.size(); ++i) P.small.add(P.convs[i].geom(F), EPI_AFFINE | EPI_RELU, 0, i ? SMALL_BY_RULE : SMALL_NEVER);
  return Pp;
}

// ---------------------------------------------------------------------------------------------------------
static void fill_taps_fwd(GatherGemmParams& g, int k, int pad) {
  int t = 0;
  for (int kh = 0; kh < k; ++kh)
    for (int kw = 0; kw < k; ++kw) {
      g.dy[t] = (signed char)(kh - pad); g.dx[t] = (signed char)(kw - pad); g.wt[t] = (unsigned char)(kh * k + kw); ++t;
    }
  g.ntaps = t;
}

// the forward launch of convolution c; the caller adds the pointers its epilogue flags read (stats / bias, or bn_scale / bn_shift)
static void fill_forward_params(GatherGemmParams& g, const float* X, const float* W, float* out, const ConvGeom& c, int flags, int dt) {
  memset(&g, 0, sizeof g);
  g.dtype = dt;
  g.A = X; g.B = W; g.out = out;
  g.N = c.N; g.Hi = c.Hi; g.Wi = c.Wi; g.Ci = c.Ci;
  g.Hg = c.Ho(); g.Wg = c.Wo(); g.Ho = c.Ho(); g.Wo = c.Wo(); g.Nc = c.Co;
  g.is = c.stride; g.os = 1; g.ooy = 0; g.oox = 0;
  g.M = c.M();
  g.T = c.k * c.k;
  fill_taps_fwd(g, c.k, c.pad);
  g.flags = flags;
  g.simple_rows = c.simple_rows();
}
int conv_forward_launch(const float* X, const float* W, float* Y, float* stats, const float* bias, const ConvGeom& c, int flags, int dt,
                        hipStream_t s) {
  GatherGemmParams g;
  fill_forward_params(g, X, W, Y, c, flags, dt);
  g.stats = stats; g.bias = bias;
  return launch_gather_gemm(g, s);
}
int conv_forward_launch_affine(const float* X, const float* W, float* out, const float* scale, const float* shift, const ConvGeom& c,
                               int flags, int dt, hipStream_t s) {
  GatherGemmParams g;
  fill_forward_params(g, X, W, out, c, flags, dt);
  g.bn_scale = scale; g.bn_shift = shift;
  return launch_gather_gemm(g, s);
}
bool conv_forward_affine_fusable(const ConvGeom& c, int flags, int dt) {
  GatherGemmParams g;
  static const float one = 1.f;   // (the query looks at shapes, flags and whether the coefficient pointers are set — never dereferenced)
  fill_forward_params(g, nullptr, nullptr, nullptr, c, flags, dt);
  g.bn_scale = g.bn_shift = &one;
  return gather_gemm_fuses_affine(g);
}

int conv_dgrad_launch(const float* dY, const float* Wt, float* dX, const float* add0, const float* add1, const unsigned* addbits,
                      const ConvGeom& c, int flags, int dt, hipStream_t s, BnRedArgs* br) {
  const int N = c.N, Hi = c.Hi, Wi = c.Wi, k = c.k, stride = c.stride, pad = c.pad;
  R3M_REQUIRE(stride == 1 || stride == 2, "dgrad: stride %d", stride);
  GatherGemmParams g;
  memset(&g, 0, sizeof g);
  g.dtype = dt;
  if (br) {
    flags |= EPI_BNRED;
    g.bn_y = br->Y; g.bn_bits = br->bits; g.bn_scale = br->scale; g.bn_shift = br->shift; g.bn_mean = br->mean;
    g.stats = br->partial;
    br->rows_out = 0;
  }
  g.A = dY; g.B = Wt; g.out = dX; g.add0 = add0; g.add1 = add1; g.addbits = addbits;
  g.N = N; g.Hi = c.Ho(); g.Wi = c.Wo(); g.Ci = c.Co;   // the GEMM "input" is dY
  g.Ho = Hi; g.Wo = Wi; g.Nc = c.Ci;
  g.is = 1; g.T = k * k; g.flags = flags;
  if (stride == 1) {
    g.Hg = Hi; g.Wg = Wi; g.os = 1; g.ooy = g.oox = 0;
    g.M = N * Hi * Wi;
    int t = 0;
    for (int kh = 0; kh < k; ++kh)
      for (int kw = 0; kw < k; ++kw) {
        g.dy[t] = (signed char)(pad - kh); g.dx[t] = (signed char)(pad - kw); g.wt[t] = (unsigned char)(kh * k + kw); ++t;
      }
    g.ntaps = t;
    g.simple_rows = (k == 1 && pad == 0) ? 1 : 0;
    if (br) br->rows_out = bnred_partial_rows(g.M);
    return launch_gather_gemm(g, s);
  }
  // stride 2: one launch per output parity class; class (py,px) only sees taps with (py+pad-kh), (px+pad-kw) even
  return for_each_parity_class(Hi, Wi, [&](int py, int px, int Hg, int Wg) -> int {
    GatherGemmParams q = g;
    q.Hg = Hg; q.Wg = Wg;
    q.os = 2; q.ooy = py; q.oox = px;
    q.M = N * Hg * Wg;
    int t = 0;
    for (int kh = 0; kh < k; ++kh) {
      if ((py + pad - kh) & 1) continue;
      for (int kw = 0; kw < k; ++kw) {
        if ((px + pad - kw) & 1) continue;
        q.dy[t] = (signed char)((py + pad - kh) / 2); q.dx[t] = (signed char)((px + pad - kw) / 2);
        q.wt[t] = (unsigned char)(kh * k + kw); ++t;
      }
    }
    q.ntaps = t;
    q.simple_rows = 0;
    R3M_REQUIRE(!(br && t == 0), "dgrad: EPI_BNRED on a parity class without taps (1x1 stride-2) is not supported");
    if (t == 0 && (flags & EPI_ACCUM) && !(flags & EPI_MASKED_ADD)) return 0;  // nothing to add
    if (br) {                                          // every parity class appends its own partial rows
      q.stats = br->partial + (long long)br->rows_out * 2 * q.Nc;
      br->rows_out += bnred_partial_rows(q.M);
    }
    return launch_gather_gemm(q, s);
  });
}

// The weight gradient of one convolution: fill the parameters, take the plan (wgrad.hip: route, tile, split-K factor — the one
// dispatch of the family, both storage types), launch, reduce the split-K slabs.
static WgradParams wgrad_params(const float* X, const float* dY, float* partial_ws, const ConvGeom& c, int dt) {
  WgradParams w;
  memset(&w, 0, sizeof w);
  w.dtype = dt;
  w.Ho = c.Ho(); w.Wo = c.Wo();
  w.dY = dY; w.X = X; w.out = partial_ws;
  w.N = c.N; w.Hi = c.Hi; w.Wi = c.Wi; w.Ci = c.Ci; w.Co = c.Co;
  w.KH = w.KW = c.k; w.stride = c.stride; w.pad = c.pad;
  w.M = c.M();
  w.simple_rows = c.simple_rows();
  return w;
}
int conv_wgrad_launch(const float* X, const float* dY, float* dW, float* partial_ws, const ConvGeom& c, int accumulate, int dt,
                      hipStream_t s) {
  const WgradParams w = wgrad_params(X, dY, partial_ws, c, dt);
  const WgradPlan r = wgrad_plan(w);
  if (int e = launch_wgrad(w, r, s)) return e;
  return launch_wgrad_reduce(partial_ws, dW, c.w_elems(), r.split, accumulate, s);
}
WgradPlan conv_wgrad_plan(const ConvGeom& c, int dt) { return wgrad_plan(wgrad_params(nullptr, nullptr, nullptr, c, dt)); }
size_t conv_wgrad_ws_floats(const ConvGeom& c, int dt) { return (size_t)conv_wgrad_plan(c, dt).split * c.w_elems(); }

// ---------------------------------------------------------------------------------------------------------
// add_conv pushes five tensors per convolution: weight, BatchNorm weight, bias, running_mean, running_var
static size_t tensor_of(const Plan& P, const ConvSpec& L) { return 5 * (size_t)(&L - P.convs.data()); }

// one forward or backward call: the plan's layout (read-only), its run state, and the caller's buffers
struct Ctx {
  const Plan& P;
  RunState& R;
  const float* params;
  float* grads;
  float* bufs;
  float* arena;
  hipStream_t s;
  int training;
  int accumulate;
  int dt;
  bool prepared = false;            // plan_forward_prepared: the eval coefficients (and the bf16 weight image) are in the arena already
  char* small_ws = nullptr;         // plan_forward_prepared: the caller's workspace when the small-M kernel may run, else null
  // where BatchNorm backward puts d gamma / d beta of layer L: the flat gradient buffer, or plan scratch when no parameter gradient
  // is wanted (the sums themselves are still formed: train-mode dz needs c1 / c2 from the same pass)
  // (a frozen gamma / beta counts as unwanted: its range of the gradient buffer is never written)
  bool wanted(const ConvSpec& L, int which) const { return grads && (R.mask.empty() || R.mask[tensor_of(P, L) + which]); }
  float* dgamma(const ConvSpec& L) const { return wanted(L, 1) ? grads + L.gamma_off : arena + P.gsc_off; }
  float* dbeta(const ConvSpec& L) const { return wanted(L, 2) ? grads + L.beta_off : arena + P.gsc_off + 2048; }
  int bn_accumulate(const ConvSpec& L) const { return wanted(L, 1) || wanted(L, 2) ? accumulate : 0; }
  int work(const ConvSpec& L) const { return R.work[&L - P.convs.data()]; }
  float* partial() const { return arena + P.partial_off; }
  double* acc() const { return reinterpret_cast<double*>(arena + P.acc_off); }
  BnScratch bn_scratch() const { return {partial(), acc()}; }
  long long rows(const ConvSpec& L) const { return (long long)P.F * L.Ho * L.Wo; }
  BnCoef coef(const ConvSpec& L) const { return bn_coef_block(arena + L.coef_off, L.Co); }
  // layer L's part in a BatchNorm backward (bn.hip): sums into dgamma() / dbeta(), c1 / c2 into its coefficient block
  BnBwdSide bn_side(const ConvSpec& L, float* dY, int work) const {
    return {arena + L.Y_off, coef(L), bn_bwd_out(dgamma(L), dbeta(L), arena + L.coef_off, L.Co, bn_accumulate(L)), dY, (work & BW_BN_SUMS) != 0};
  }
  // gradient buffer in role r (0 = D, 1 / 2 = A0 / A1, 3 = B, 4 = C), and the A buffer the next dY goes to
  float* G(int r) const { return arena + P.G_off[R.roles[r]]; }
  float* next_A(int* ai) const { *ai = R.a_next; R.a_next ^= 1; return G(1 + *ai); }
};

// Tile queues of the persistent kernel (conv_pw.hip) for the launches of layer L: the arena holds [convs][8] counters for the forward
// launch of each conv, then [convs][4][8] for its (up to four: stride-2 parity classes) backward launches; each set serves one launch
// and is zeroed at the top of its pass. The counters are handed to "the next launch of this thread": if the launcher returns before it
// reaches launch_gather_gemm (a failed requirement), nothing later on this thread may inherit them, so the guard takes them back (sets
// a layer did not use stay unused).
struct TileCounters {
  enum Pass { FORWARD = 0, BACKWARD = 1 };
  static unsigned* slot(const Ctx& c, Pass pass, size_t layer) {
    return reinterpret_cast<unsigned*>(c.arena + c.P.ctr_off) + (pass == FORWARD ? layer : c.P.convs.size() + 4 * layer) * 8;
  }
  static int reset(const Ctx& c, Pass pass) {
    if (hipMemsetAsync(slot(c, pass, 0), 0, (pass == FORWARD ? 1 : 4) * c.P.convs.size() * 8 * sizeof(unsigned), c.s) != hipSuccess) {
      set_last_error("resnet_%s: cannot reset the tile queues", pass == FORWARD ? "forward" : "backward");
      return 1;
    }
    return 0;
  }
  TileCounters(const Ctx& c, Pass pass, const ConvSpec& L) { gg_set_tile_counters(slot(c, pass, &L - c.P.convs.data()), pass == FORWARD ? 1 : 4); }
  ~TileCounters() { gg_set_tile_counters(nullptr, 0); }
};

// ---- forward ------------------------------------------------------------------------------------------------
// forward weight operand of layer L: the fp32 master, or its slice of the bf16 image made at the top of plan_forward
static const float* fwd_weights(Ctx& c, const ConvSpec& L) {
  if (c.dt != DT_BF16) return c.params + L.w_off;
  return reinterpret_cast<const float*>(reinterpret_cast<const char*>(c.arena + c.P.w16_off) + L.w_off * 2);
}

// training: the statistics partials a forward launch left (L.stats_rows rows) -> batch coefficients (+ running-statistics update);
// eval / inference: running statistics -> coefficients
static int bn_forward_coeffs(Ctx& c, const ConvSpec& L) {
  if (c.prepared) return 0;
  const float* gamma = c.params + L.gamma_off;
  const float* beta = c.params + L.beta_off;
  const BnCoefOut o = bn_coef_out(c.arena + L.coef_off, L.Co);
  if (!c.training) return launch_bn_eval_coeffs(gamma, beta, c.bufs + L.rm_off, c.bufs + L.rv_off, 1e-5f, o, L.Co, c.s);
  return bn_train_coeffs(c.partial(), L.stats_rows, c.rows(L), gamma, beta, c.bufs + L.rm_off, c.bufs + L.rv_off, 0.1f, 1e-5f, o, L.Co, c.acc(),
                         c.s);
}

// conv -> BatchNorm coefficients (the raw output stays in Y)
static int conv_bn(Ctx& c, const ConvSpec& L, const float* X) {
  {
    TileCounters tc(c, TileCounters::FORWARD, L);
    TRY(conv_forward_launch(X, fwd_weights(c, L), c.arena + L.Y_off, c.partial(), nullptr, L.geom(c.P.F), c.training ? EPI_STATS : 0, c.dt,
                            c.s));
  }
  return bn_forward_coeffs(c, L);
}

// x/255 -> Normalize -> conv1 7x7/2 straight from the NCHW frames (Stem, above) -> BatchNorm + ReLU + MaxPool
static int stem_forward(Ctx& c, const float* x_nchw, const FrameSource* crop) {
  const Plan& P = c.P;
  const int F = P.F, dt = c.dt;
  const ConvSpec& L0 = P.convs[0];
  const bool gen = !crop && (P.H != 224 || P.W != 224 || g_generic_stem);
  c.R.stem_gen = gen ? 1 : 0;
  const Stem stem(P, dt, gen, c.s);
  // normalised, channel-interleaved copy of the frames (0.6 MB/frame): read by the stem forward now and by its weight
  // gradient in backward (the caller's tensor may be gone by then)
  float* xn = c.arena + P.col_off;
  TRY(stem.prep(x_nchw, crop, xn));
  float* Y = c.arena + L0.Y_off;
  TRY(stem.forward(xn, c.params + L0.w_off, Y, c.training ? c.partial() : nullptr));
  TRY(bn_forward_coeffs(c, L0));
  // BatchNorm + ReLU + MaxPool in one pass over Y0
  return launch_bn_relu_maxpool_fwd(Y, c.coef(L0), c.arena + P.P0_off, reinterpret_cast<unsigned char*>(c.arena + P.amax_off), F, P.H1, P.W1, 64,
                                    dt, c.s);
}

// One residual block, unfused: every conv leaves its raw output and coefficients, bn_act_fwd makes the activations and the block
// output (+ its [z > 0] bits for backward when mask != null). Writes B's output buffer.
static int block_forward(Ctx& c, const BlockSpec& B, const float* Xin, unsigned* mask) {
  const Plan& P = c.P;
  const float* cur = Xin;
  for (int j = 0; j < B.nconv; ++j) {
    const ConvSpec& L = P.convs[B.conv[j]];
    TRY(conv_bn(c, L, cur));
    if (j < B.nconv - 1) {
      TRY(launch_bn_act_fwd(c.arena + L.Y_off, c.coef(L), nullptr, nullptr, c.arena + L.Z_off, c.rows(L), L.Co, 1, nullptr, c.dt, c.s));
      cur = c.arena + L.Z_off;
    }
  }
  const ConvSpec& LL = P.convs[B.conv[B.nconv - 1]];
  const long long rows = (long long)P.F * B.Ho * B.Wo;
  if (B.ds < 0)
    return launch_bn_act_fwd(c.arena + LL.Y_off, c.coef(LL), Xin, nullptr, c.arena + B.out_off, rows, B.Co, 1, mask, c.dt, c.s);
  const ConvSpec& Ld = P.convs[B.ds];
  TRY(conv_bn(c, Ld, Xin));
  const BnCoef Kd = c.coef(Ld);
  return launch_bn_act_fwd(c.arena + LL.Y_off, c.coef(LL), c.arena + Ld.Y_off, &Kd, c.arena + B.out_off, rows, B.Co, 1, mask, c.dt, c.s);
}

// Inference: every convolution of the block stores its activated output itself — inner convs relu(bn(conv)), the downsample conv
// bn(conv), the last conv relu(bn(conv) + residual) accumulating ONTO the residual (the block input, in place, or the downsample
// result): no raw conv output, no bn_act_fwd pass, no mask bits. A block any of whose launches runs a kernel without these
// epilogues (odd shapes; never a ResNet layer) takes the unfused sequence instead.
static bool block_fusable(Ctx& c, const BlockSpec& B) {
  bool fus = true;
  for (int j = 0; j < B.nconv; ++j)
    fus = fus && conv_forward_affine_fusable(c.P.convs[B.conv[j]].geom(c.P.F),
                                             j < B.nconv - 1 ? (EPI_AFFINE | EPI_RELU) : (EPI_AFFINE | EPI_ACCUM | EPI_RELU), c.dt);
  if (B.ds >= 0) fus = fus && conv_forward_affine_fusable(c.P.convs[B.ds].geom(c.P.F), EPI_AFFINE, c.dt);
  return fus;
}
static int conv_bn_fused(Ctx& c, const ConvSpec& L, const float* X, float* out, int flags) {
  TRY(bn_forward_coeffs(c, L));
  if (const int i = (int)(&L - c.P.convs.data()); c.small_ws && c.P.small.runs(i))
    return c.P.small.launch(i, 0, c.small_ws, X, c.params + L.w_off, out, c.coef(L).scale, c.coef(L).shift, c.s, flags);
  TileCounters tc(c, TileCounters::FORWARD, L);
  return conv_forward_launch_affine(X, fwd_weights(c, L), out, c.coef(L).scale, c.coef(L).shift, L.geom(c.P.F), flags, c.dt, c.s);
}
// *out: where the block's output is (the block input, or the downsample conv's Y)
static int block_forward_fused(Ctx& c, const BlockSpec& B, float* Xin, float** out) {
  const Plan& P = c.P;
  const float* cur = Xin;
  for (int j = 0; j < B.nconv - 1; ++j) {
    const ConvSpec& L = P.convs[B.conv[j]];
    TRY(conv_bn_fused(c, L, cur, c.arena + L.Z_off, EPI_AFFINE | EPI_RELU));
    cur = c.arena + L.Z_off;
  }
  float* res = Xin;       // identity block: the sum replaces the block input
  if (B.ds >= 0) {
    const ConvSpec& Ld = P.convs[B.ds];
    res = c.arena + Ld.Y_off;
    TRY(conv_bn_fused(c, Ld, Xin, res, EPI_AFFINE));
  }
  *out = res;
  return conv_bn_fused(c, P.convs[B.conv[B.nconv - 1]], cur, res, EPI_AFFINE | EPI_ACCUM | EPI_RELU);
}

// the last block of its stage: its output is torchvision's layer`stage + 1` output
static bool ends_stage(const Plan& P, size_t bi) { return bi + 1 == P.blocks.size() || P.blocks[bi + 1].stage != P.blocks[bi].stage; }

static int forward_sequence(Ctx& c, const float* x_nchw, const FrameSource* crop, float* h_out, bool infer, bool fused, float* const* feats);

int plan_forward(Plan& P, const float* x_nchw, const FrameSource* crop, const float* params, float* bufs, float* arena, float* h_out,
                 int training, hipStream_t s, float* const* feats) {
  // training: 1 = batch statistics (+ running-statistics update), 0 = running statistics with everything a backward needs kept,
  // 2 = INFERENCE (round 6): running statistics, nothing kept — BatchNorm, residual join and ReLU ride in the convolutions' stores
  const bool infer = training == 2;
  if (infer) training = 0;
  Ctx c{P, P.run, params, nullptr, bufs, arena, s, training, 0, P.dtype};
  R3M_REQUIRE(!crop || (P.H == 224 && P.W == 224), "resnet_forward_crop: the crops are 224 x 224 but this plan takes %d x %d frames "
              "(create it for 224 x 224)", P.H, P.W);
  R3M_REQUIRE(!(crop && feats), "resnet_forward_crop: feature maps are not available on the crop-fed forward");
  c.R.prepared = nullptr;            // this forward rewrites the coefficient blocks (a bf16 plan: the weight image too)
  if (c.dt == DT_BF16) TRY(launch_convert_bf16(params, arena + P.w16_off, P.n_params, s));   // bf16 image of every weight (45 MB for ResNet-50)
  return forward_sequence(c, x_nchw, crop, h_out, infer, infer && g_fused_inference, feats);
}

// stem -> blocks -> pool on c's stream; fused: the inference sequence (block_forward_fused where every launch of the block has the stores)
static int forward_sequence(Ctx& c, const float* x_nchw, const FrameSource* crop, float* h_out, bool infer, bool fused, float* const* feats) {
  const Plan& P = c.P;
  float* arena = c.arena;
  hipStream_t s = c.s;
  c.R.last_training = c.training;
  c.R.last_crop = crop ? 1 : 0;
  c.R.next_stage = infer ? -3 : 0;   // a new forward invalidates whatever an unfinished backward left behind (-3: nothing to differentiate)
  c.R.dout_fused_rows = 0;
  TRY(TileCounters::reset(c, TileCounters::FORWARD));
  TRY(stem_forward(c, x_nchw, crop));
  float* cur = arena + P.blocks[0].in_off;
  for (size_t bi = 0; bi < P.blocks.size(); ++bi) {
    const BlockSpec& B = P.blocks[bi];
    if (fused && block_fusable(c, B)) {
      TRY(block_forward_fused(c, B, cur, &cur));
    } else {
      TRY(block_forward(c, B, cur, fused ? nullptr : reinterpret_cast<unsigned*>(arena + B.mask_off)));
      cur = arena + B.out_off;
    }
    // a requested stage output leaves here, behind the stage's last block: in the fused sequence `cur` is a block input or a
    // downsample result that the next identity block overwrites in place
    if (feats && feats[B.stage] && ends_stage(P, bi)) TRY(launch_feature_export(cur, feats[B.stage], P.F, B.Ho, B.Wo, B.Co, c.dt, s));
  }
  const BlockSpec& last = P.blocks.back();
  return launch_avgpool_fwd(cur, h_out, P.F, last.Ho * last.Wo, last.Co, c.dt, s);
}

// ---- prepared inference: the eval coefficients of every BatchNorm (bf16 plans: the weight image too) are written ONCE, by
// plan_inference_prepare; plan_forward_prepared then runs the fused inference sequence without the per-layer coefficient launches and
// without the weight conversion, and (fp32) sends the launches the routing rule of conv_small.hip takes to that kernel ----
int plan_inference_prepare(Plan& P, const float* params, const float* bufs, float* arena, hipStream_t s) {
  BnEvalTable t;
  R3M_REQUIRE(P.convs.size() <= sizeof(t.e) / sizeof(t.e[0]), "resnet_inference_prepare: %d BatchNorms do not fit the table", (int)P.convs.size());
  t.n = 0; t.blocks = 0;
  for (const ConvSpec& L : P.convs) {
    t.e[t.n++] = BnEvalEntry{L.gamma_off, L.beta_off, L.rm_off, L.rv_off, L.coef_off, L.Co, t.blocks};
    t.blocks += ceil_div(L.Co, 256);
  }
  P.run.prepared = nullptr;
  TRY(launch_bn_eval_coeffs_table(params, bufs, arena, t, 1e-5f, s));
  if (P.dtype == DT_BF16) TRY(launch_convert_bf16(params, arena + P.w16_off, P.n_params, s));
  P.run.prepared = arena;
  return 0;
}
long long plan_inference_workspace_bytes(Plan* P) { return (long long)P->small.bytes(); }
int plan_forward_prepared(Plan& P, const float* x_nchw, const float* params, float* arena, void* workspace, float* h_out, float* const* feats,
                          int flags, hipStream_t s) {
  R3M_REQUIRE(P.run.prepared && P.run.prepared == arena, "resnet_forward_prepared: this arena is not prepared for the plan (call "
              "r3m_resnet_inference_prepare first; any other forward of the plan invalidates the preparation)");
  const bool small = !(flags & 1) && P.small.ticket_bytes() > 0;
  R3M_REQUIRE(!small || workspace, "resnet_forward_prepared: the plan needs a workspace of r3m_resnet_inference_workspace_bytes");
  Ctx c{P, P.run, params, nullptr, nullptr, arena, s, 0, 0, P.dtype};
  c.prepared = true;
  c.small_ws = small ? static_cast<char*>(workspace) : nullptr;
  R3M_REQUIRE(!small || !P.small.reset(workspace, s), "resnet_forward_prepared: cannot reset the split-K tickets");
  return forward_sequence(c, x_nchw, nullptr, h_out, true, true, feats);
}

// ---- backward -----------------------------------------------------------------------------------------------
// BatchNorm(+ReLU / residual mask) backward of layer L (bn.hip, bn_bwd): dZ -> dY, parameter gradients into the flat gradient buffer.
// fused_rows > 0: the dgrad that produced dZ already wrote this BatchNorm's backward partials (EPI_BNRED) into the partial buffer:
// the stand-alone first pass is skipped
// work: BW_BN_SUMS / BW_BN_APPLY of this layer (a BatchNorm whose dY nobody reads only forms its parameter sums)
static int bn_backward(Ctx& c, const ConvSpec& L, const float* dZ, const unsigned* Zbits, float* dY, int fused_rows, int work) {
  return bn_bwd(dZ, nullptr, Zbits, c.bn_side(L, dY, work), c.partial(), fused_rows, (work & BW_BN_APPLY) != 0, c.rows(L), L.Co,
                c.R.last_training, c.bn_scratch(), c.dt, c.s);
}
// The two BatchNorms that feed a downsample block's add + ReLU (its last convolution's and the downsample convolution's) see the SAME
// masked output gradient: bn_bwd_pair (bn.hip) runs their second passes as ONE launch that reads dOut and the mask bits once.
// work / work_d: the BW_* bits of L / Ld; the joint launches run as long as either side needs them.
static int bn_backward_pair(Ctx& c, const ConvSpec& L, const ConvSpec& Ld, const float* dZ, const unsigned* Zbits, float* dY, float* dYd,
                            int fused_rows, int work, int work_d) {
  R3M_REQUIRE(L.Co == Ld.Co && L.Ho == Ld.Ho && L.Wo == Ld.Wo && Zbits, "bn_backward_pair: the two BatchNorms must have one shape and mask bits");
  const long long set = (long long)bn_bwd_partial_rows(c.rows(L), L.Co, c.dt) * 2 * L.Co;   // the second partial set right behind the first
  return bn_bwd_pair(dZ, Zbits, c.bn_side(L, dY, work), c.bn_side(Ld, dYd, work_d), c.partial(), fused_rows, ((work | work_d) & BW_BN_APPLY) != 0,
                     set, c.rows(L), L.Co, c.R.last_training, c.bn_scratch(), c.dt, c.s);
}

static int wgrad(Ctx& c, const ConvSpec& L, const float* X, const float* dY) {
  return conv_wgrad_launch(X, dY, c.grads + L.w_off, c.arena + c.P.wgp_off, L.geom(c.P.F), c.accumulate, c.dt, c.s);
}

// bn_of: the conv layer whose BatchNorm consumes dX as its dz (its Y has dX's shape), bn_bits: that BatchNorm's output mask bits
// (block outputs) or null (mask recomputed from Y). *fused_rows_out receives the partial-row count (0 = not fused).
static int dgrad(Ctx& c, const ConvSpec& L, const float* dY, float* dX, int flags, const float* add0, const unsigned* addbits,
                 const ConvSpec* bn_of = nullptr, const unsigned* bn_bits = nullptr, int* fused_rows_out = nullptr) {
  // the layer's [Ci][k*k][Co] weight image was built at the start of this backward (plan_backward, stage 0)
  float* Wt = c.dt == DT_BF16 ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(c.arena + c.P.wt_off) + L.wt_off)
                              : c.arena + c.P.wt_off + L.wt_off;
  if (fused_rows_out) *fused_rows_out = 0;
  TileCounters tc(c, TileCounters::BACKWARD, L);
  // 1x1 stride-2 dgrads leave three of four parity classes without taps (plain zero / no-op launches): not fused
  const bool fuse = bn_of && fused_rows_out && c.P.fuse_bnred && !(L.stride == 2 && L.k == 1);
  if (!fuse) return conv_dgrad_launch(dY, Wt, dX, add0, nullptr, addbits, L.geom(c.P.F), flags, c.dt, c.s);
  const BnCoef K = c.coef(*bn_of);
  BnRedArgs br{c.arena + bn_of->Y_off, bn_bits, K.scale, K.shift, K.mean, c.partial(), 0};
  TRY(conv_dgrad_launch(dY, Wt, dX, add0, nullptr, addbits, L.geom(c.P.F), flags, c.dt, c.s, &br));
  *fused_rows_out = br.rows_out;
  return 0;
}

// ---- the opt-in side stream (declared with RunState above) ----
int SideStream::init() {
  // Opt-in. Measured on ResNet-50 F=1280 (profiles/r01 notes in DESIGN.md): co-running wgrad with the BatchNorm-backward
  // passes lengthens the wgrad launches by about the BatchNorm time (the two do not overlap usefully on gfx950 even
  // though one is HBM-bound and the other MFMA-bound) -> step time unchanged (364.9 vs 364.5 ms). Kept for experiments.
  // 2 (round 5 experiment): wgrad(L) starts TOGETHER with dgrad(L) (both wait for dY_L only) and nothing on the main stream waits
  // for it before its dY buffer is rewritten: the two GEMMs fill each other's tile-quantisation tails (every launch of the
  // 1280-frame step has 490 k tiles for 512 slots).
  if (mode < 0) mode = R3M_ENV_INT("R3M_SIDE_STREAM", 0);
  if (!mode || side) return 0;
  if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) { set_last_error("side stream: create failed"); return 1; }
  for (hipEvent_t* ev : {&ev_dy, &ev_wg[0], &ev_wg[1], &ev_join})
    if (hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) { set_last_error("side stream: event create failed"); return 1; }
  return 0;
}
void SideStream::destroy() {
  if (!side) return;
  (void)hipStreamDestroy(side);
  for (hipEvent_t ev : {ev_dy, ev_wg[0], ev_wg[1], ev_join})
    if (ev) (void)hipEventDestroy(ev);
}
int SideStream::mark_dy() {
  if (hipEventRecord(ev_dy, main) != hipSuccess || hipStreamWaitEvent(side, ev_dy, 0) != hipSuccess) {
    set_last_error("side stream: event ordering failed");
    return 1;
  }
  return 0;
}
int SideStream::wgrad_async(Ctx& c, const ConvSpec& L, const float* X, const float* dY, int ai) {
  if (!c.grads) return 0;                  // frozen encoder: no weight gradient
  if (!on) return wgrad(c, L, X, dY);
  if (mode != 2) TRY(mark_dy());           // mode 1: wgrad(L) starts once the dgrad(L) just enqueued is done
  Ctx cs = c;                              // context whose launches go to the side stream
  cs.s = side;
  TRY(wgrad(cs, L, X, dY));
  if (hipEventRecord(ev_wg[ai], side) != hipSuccess) { set_last_error("side stream: record failed"); return 1; }
  pending[ai] = true;
  return 0;
}
int SideStream::acquire(int ai) {
  if (on && pending[ai]) {
    if (hipStreamWaitEvent(main, ev_wg[ai], 0) != hipSuccess) { set_last_error("side stream: wait failed"); return 1; }
    pending[ai] = false;
  }
  return 0;
}
int SideStream::wait_wgrads() {
  if (on && mode == 2) return mark_dy();      // mode 2: no wait; the dY just written is what the side stream waits for
  TRY(acquire(0));
  return acquire(1);
}
int SideStream::join() {
  if (!on) return 0;
  if (hipEventRecord(ev_join, side) != hipSuccess || hipStreamWaitEvent(main, ev_join, 0) != hipSuccess) {
    set_last_error("side stream: join failed");
    return 1;
  }
  pending[0] = pending[1] = false;
  return 0;
}

// the weights are final since the last optimizer step: all dgrad weight images in one launch, at the start of each backward
static int build_weight_images(Ctx& c) {
  const Plan& P = c.P;
  if (!c.R.d_wt_tab) {
    // failure-atomic: the plan's pointers are set only after both allocations and both uploads succeeded (a half-initialised
    // pair would make the next backward skip this block and launch transpose_w_all on a null / uninitialised table)
    const size_t tb = P.wt_tab.size() * sizeof(WtEntry), ib = P.wt_tile0.size() * sizeof(int);
    WtEntry* d_tab = nullptr;
    int* d_tile0 = nullptr;
    const bool ok = hipMalloc(reinterpret_cast<void**>(&d_tab), tb) == hipSuccess &&
                    hipMalloc(reinterpret_cast<void**>(&d_tile0), ib) == hipSuccess &&
                    hipMemcpy(d_tab, P.wt_tab.data(), tb, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemcpy(d_tile0, P.wt_tile0.data(), ib, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      if (d_tab) (void)hipFree(d_tab);
      if (d_tile0) (void)hipFree(d_tile0);
      set_last_error("resnet_backward: cannot allocate / upload the weight-image table (%zu + %zu bytes)", tb, ib);
      return 1;
    }
    c.R.d_wt_tab = d_tab;
    c.R.d_wt_tile0 = d_tile0;
  }
  return launch_transpose_w_all(c.params, c.arena + P.wt_off, c.R.d_wt_tab, c.R.d_wt_tile0, (int)P.wt_tab.size(), P.wt_tile0.back(), P.dtype,
                                c.s);
}

// Block bi: the gradient of its output (role D) -> parameter gradients and the gradient of its input (role C, then swapped into D)
static int block_backward(Ctx& c, int bi) {
  const Plan& P = c.P;
  SideStream& side = c.R.side;
  float* arena = c.arena;
  const BlockSpec& B = P.blocks[bi];
  const float* dOut = c.G(0);
  const unsigned* Out = reinterpret_cast<const unsigned*>(arena + B.mask_off);   // [out > 0] bits
  const float* Xin = arena + B.in_off;
  float* Gb = c.G(3);
  float* Gc = c.G(4);
  // last conv of the block: its BatchNorm output joined the residual add, mask comes from the block output
  const float* dz = dOut;
  const unsigned* zmask = Out;
  // partials of the BatchNorm that consumes dz, written by the dgrad that produced dz (EPI_BNRED) — 0: none
  int dz_fused = c.R.dout_fused_rows;
  c.R.dout_fused_rows = 0;
  // the block whose output gradient this block's last dgrad completes, and the BatchNorm (its last conv's) that will read it
  const BlockSpec* Bprev = bi > 0 ? &P.blocks[bi - 1] : nullptr;
  const ConvSpec* Lprev_last = Bprev ? &P.convs[Bprev->conv[Bprev->nconv - 1]] : nullptr;
  const unsigned* prev_bits = Bprev ? reinterpret_cast<const unsigned*>(arena + Bprev->mask_off) : nullptr;
  int ai = 0;
  // downsample block: both tail BatchNorms in one second pass, the downsample one's dY parked in E until the end of the block
  // (R3M_BN_PAIR=0 in probe builds: two separate passes, for A/B)
  const bool pair = B.ds >= 0 && P.E_off >= 0 && B.nconv >= 2 && P.bn_pair && R3M_ENV_INT("R3M_BN_PAIR", 1) != 0 && P.convs[B.ds].Co >= 8;
  float* const dYd_pair = pair ? arena + P.E_off : nullptr;
  // Every step below runs iff its BW_* bit is set (backward_work). The bits are monotone along the main path — a convolution without
  // work has none below it in the block — so a launch that is kept always finds its input written by a launch that was kept too.
  const int wd = B.ds >= 0 ? c.work(P.convs[B.ds]) : 0;
  float* dY = nullptr;
  for (int j = B.nconv - 1; j >= 1; --j) {
    const ConvSpec& L = P.convs[B.conv[j]];
    const ConvSpec& Lprev = P.convs[B.conv[j - 1]];
    const int w = c.work(L);
    const bool tail_pair = pair && j == B.nconv - 1;
    if ((w | (tail_pair ? wd : 0)) & BW_BN_SUMS) {
      dY = c.next_A(&ai);
      TRY(side.acquire(ai));
      if (tail_pair) TRY(bn_backward_pair(c, L, P.convs[B.ds], dz, zmask, dY, dYd_pair, dz_fused, w, wd));
      else TRY(bn_backward(c, L, dz, zmask, dY, dz_fused, w));     // HBM-bound: overlaps the previous layer's wgrad
    }
    dz_fused = 0;
    if (w & BW_DGRAD) {
      TRY(side.wait_wgrads());
      TRY(dgrad(c, L, dY, Gb, 0, nullptr, nullptr, &Lprev, nullptr, &dz_fused));   // Gb = dz of Lprev's BatchNorm + its partials
    }
    if (w & BW_WGRAD) TRY(side.wgrad_async(c, L, arena + Lprev.Z_off, dY, ai));
    dz = Gb; zmask = nullptr;   // Gb is consumed by the next bn_backward before a later dgrad rewrites it
  }
  const ConvSpec& L1 = P.convs[B.conv[0]];
  const int w1 = c.work(L1);
  float* dY1 = nullptr;
  if (w1 & BW_BN_SUMS) {
    dY1 = c.next_A(&ai);
    TRY(side.acquire(ai));
    TRY(bn_backward(c, L1, dz, zmask, dY1, dz_fused, w1));
  }
  if (w1 & BW_DGRAD) TRY(side.wait_wgrads());
  if (B.ds >= 0) {
    const ConvSpec& Ld = P.convs[B.ds];
    if (w1 & BW_DGRAD) TRY(dgrad(c, L1, dY1, Gc, 0, nullptr, nullptr));      // (DGRAD(conv1) == DGRAD(downsample): Gc is written before it is added to)
    if (w1 & BW_WGRAD) TRY(side.wgrad_async(c, L1, Xin, dY1, ai));
    if (pair) {                                     // dY of the downsample BatchNorm has been waiting in E since the block's first pass
      if (wd & BW_DGRAD) TRY(dgrad(c, Ld, dYd_pair, Gc, EPI_ACCUM, nullptr, nullptr));
      if (wd & BW_WGRAD) TRY(side.wgrad_async(c, Ld, Xin, dYd_pair, ai));      // (side stream: ordered behind conv1's wgrad, same event slot)
    } else if (wd) {
      int ad;
      float* dYd = c.next_A(&ad);
      TRY(side.acquire(ad));
      TRY(bn_backward(c, Ld, dOut, Out, dYd, 0, wd));   // overlaps wgrad(conv1); always the stand-alone reduce (second consumer of dOut)
      if (wd & BW_DGRAD) {
        TRY(side.wait_wgrads());
        TRY(dgrad(c, Ld, dYd, Gc, EPI_ACCUM, nullptr, nullptr));
      }
      if (wd & BW_WGRAD) TRY(side.wgrad_async(c, Ld, Xin, dYd, ad));
    }
  } else {
    // Gc = dgrad + masked residual gradient = the previous block's COMPLETE output gradient: also emit the partials of the
    // BatchNorm that will consume it (the previous block's last one, masked by that block's output bits)
    if (w1 & BW_DGRAD) TRY(dgrad(c, L1, dY1, Gc, EPI_MASKED_ADD, dOut, Out, Lprev_last, prev_bits, &c.R.dout_fused_rows));
    if (w1 & BW_WGRAD) TRY(side.wgrad_async(c, L1, Xin, dY1, ai));
  }
  // C becomes the gradient of the previous block's output; the old D is free (only the main stream ever read it)
  std::swap(c.R.roles[0], c.R.roles[4]);
  return 0;
}

// stem: maxpool + BN/ReLU backward (fused) -> conv1 weight gradient [-> input gradient]
// work: the stem's BW_* bits (BW_DGRAD = the input gradient)
static int stem_backward(Ctx& c, float* dx, int dx_accumulate, int work) {
  const Plan& P = c.P;
  const int F = P.F, dt = c.dt;
  const ConvSpec& L0 = P.convs[0];
  float* Gc = c.G(4);
  // MaxPool backward gathered inside both BatchNorm-backward passes (no dZ0 tensor)
  const unsigned char* am = reinterpret_cast<const unsigned char*>(c.arena + P.amax_off);
  TRY(bn_bwd_pool(c.G(0), am, c.bn_side(L0, Gc, work), (work & BW_BN_APPLY) != 0, F, P.H1, P.W1, 64, c.R.last_training, c.bn_scratch(), dt, c.s));
  TRY(c.R.side.join());   // the stem wgrad shares the split-K scratch with the side stream's wgrads
  const Stem stem(P, dt, c.R.stem_gen != 0, c.s);
  if (work & BW_WGRAD) TRY(stem.wgrad(c.arena + P.col_off, Gc, c.grads + L0.w_off, c.arena + P.wgp_off, c.accumulate));
  // Gc = conv1's output gradient; the bf16 rounding of the normalised frames is taken as identity (as autocast does)
  if (work & BW_DGRAD) TRY(stem.input_grad(Gc, c.params + L0.w_off, dx, dx_accumulate));
  return 0;
}

// THE predicate of a partial backward: which work each convolution's backward does, given which tensors want a gradient (mask: one
// byte per tensor in plan_tensor_info order, nullptr = all) and whether the input gradient is wanted. plan_backward executes these
// bits and consults nothing else; plan_debug_backward reports them. With T(L) = L's weight is trainable and Tg(L) = gamma or beta of
// L's BatchNorm is (the stem counts as "below block 0"):
//   below(block)   = dx wanted, or any trainable tensor in an earlier block or the stem
//   DGRAD(conv[0]) = DGRAD(downsample) = below(block); an identity block's masked residual add rides in DGRAD(conv[0])
//   DGRAD(conv[j]) = below(block), or any trainable tensor in conv[0..j-1] of the block               (j >= 1)
//   WGRAD(L) = T(L);  BN_APPLY(L) = DGRAD(L) | WGRAD(L) (someone reads dY);  BN_SUMS(L) = BN_APPLY(L) | Tg(L)
//   stem: DGRAD = dx wanted, the rest as above (its BatchNorm passes are the pooled ones)
// The bits are monotone: a block without work has no work below it, so the gradient of a block's output is needed iff the block
// has any bit set, and plan_backward stops at the lowest block that has.
static void backward_work(const Plan& P, const unsigned char* mask, bool want_dx, std::vector<int>& work) {
  work.assign(P.convs.size(), 0);
  auto T = [&](int ci) { return !mask || mask[5 * ci]; };                            // (tensor_of: five tensors per convolution)
  auto Tg = [&](int ci) { return !mask || mask[5 * ci + 1] || mask[5 * ci + 2]; };
  auto set = [&](int ci, bool dgrad) {
    const bool wgrad = T(ci), apply = dgrad || wgrad, sums = apply || Tg(ci);
    work[ci] = (sums ? BW_BN_SUMS : 0) | (apply ? BW_BN_APPLY : 0) | (dgrad ? BW_DGRAD : 0) | (wgrad ? BW_WGRAD : 0);
    return wgrad || Tg(ci);
  };
  bool below = set(0, want_dx) || want_dx;
  for (const BlockSpec& B : P.blocks) {
    bool d = below;
    for (int j = 0; j < B.nconv; ++j) d = set(B.conv[j], d) || d;
    if (B.ds >= 0) d = set(B.ds, below) || d;
    below = d;
  }
}
static bool block_has_work(const Plan& P, const std::vector<int>& work, const BlockSpec& B) {
  int w = B.ds >= 0 ? work[B.ds] : 0;
  for (int j = 0; j < B.nconv; ++j) w |= work[B.conv[j]];
  return w != 0;
}

// Backward stages: 0 = avgpool + layer4, 1 = layer3, 2 = layer2, 3 = layer1 + stem. The gradient w.r.t. the current
// block output lives in one of five arena buffers (roles rotate: D = dOut, A0/A1 = dY alternating, B, C); the roles are
// carried across calls so stages can be issued one by one (the data-parallel wrapper launches the RCCL all-reduce of a
// finished stage's gradient slice in between).
//
// grads == nullptr: no parameter gradient (frozen encoder) — the backward of an all-zero trainable mask with dx wanted: no
// weight-gradient launch is enqueued, the side stream stays idle and the BatchNorm parameter sums go to plan scratch.
// dx != nullptr: d/d(frames) [F,3,H,W] fp32 NCHW of the frames of the last forward (stem_dgrad.hip), written (dx_accumulate = 0)
// or added by stage 3. The call that runs stage 0 fixes the work of all four stages (backward_work) from the plan's trainable mask
// and from whether it was given dx; a stage without work enqueues nothing.
//
// Stage-output gradients (dfeats): the gradient of layer`k`'s output joins the running output gradient G(0) right before
// block_backward of that stage's last block — behind the pool's backward (or, without dh, a zero fill) for k = 4, at the top of
// stages 1..3 for k = 3..1. There G(0) is complete: its producer is the pool or a downsample block (conv1's dgrad + the downsample's
// accumulate), neither of which leaves EPI_BNRED partials, so the block's last BatchNorm runs its stand-alone first pass on the sum.
// The output is post-ReLU, so adding before the block applies its mask is autograd's sum at that node. A block without work
// (frozen prefix) drops the gradient, as autograd does.
int plan_backward(Plan& P, const float* dh, const float* params, float* grads, float* arena, int stage_begin, int stage_end,
                  int accumulate, hipStream_t s, float* dx, int dx_accumulate, const float* const* dfeats) {
  RunState& R = P.run;
  Ctx c{P, R, params, grads, nullptr, arena, s, R.last_training, accumulate, P.dtype};
  R3M_REQUIRE(stage_begin >= 0 && stage_end <= 4 && stage_begin < stage_end, "resnet_backward: stages [%d, %d) outside [0, 4)", stage_begin, stage_end);
  R3M_REQUIRE(R.next_stage != -3, "resnet_backward: the last forward on this plan ran in inference mode (training = 2): nothing was kept for a backward");
  R3M_REQUIRE(!dx || !R.last_crop, "resnet_backward: no input gradient after r3m_resnet_forward_crop (the frames were resampled from raw "
              "clips inside the stem pre-pass; pass dx = NULL)");
  R3M_REQUIRE(R.next_stage != -1, "resnet_backward: no forward has run on this plan");
  // stage 0 may always (re)start a backward over the saved activations (retain_graph); any other stage must continue the
  // sequence the previous call left off at — its inputs (running output gradient, pending EPI_BNRED partials) live in the plan
  R3M_REQUIRE(stage_begin == 0 || stage_begin == R.next_stage,
              "resnet_backward: stage %d requested but the plan expects stage %d (stages run 0..3 in order after each forward; "
              "stage 0 restarts)", stage_begin, R.next_stage);
  R.next_stage = -2;           // poisoned while in flight: after a failed call only stage 0 (a restart) is accepted
  if (stage_begin == 0) {
    R.mask = grads ? P.trainable : std::vector<unsigned char>(P.tensors.size(), 0);
    backward_work(P, R.mask.empty() ? nullptr : R.mask.data(), dx || !grads, R.work);
  }
  int stem_work = R.work[0];
  if (dx && stage_end == 4) {
    // dx given only now (every caller before the trainable mask existed): fine as long as the gradient chain reaches the stem anyway
    R3M_REQUIRE(R.work[P.blocks[0].conv[0]] & BW_DGRAD, "resnet_backward: dx asked of stage 3, but the backward planned at stage 0 stops "
                "above the stem (frozen tensors, r3m_resnet_set_trainable): pass dx to the call that runs stage 0 too");
    stem_work |= BW_DGRAD | BW_BN_APPLY | BW_BN_SUMS;
  }
  bool any_work = false;
  for (int w : R.work) any_work = any_work || w;
  TRY(R.side.init());
  R.side.begin(s, grads != nullptr);
  if (stage_begin == 0 && any_work) {
    TRY(TileCounters::reset(c, TileCounters::BACKWARD));
    TRY(build_weight_images(c));
  }
  for (int st = stage_begin; st < stage_end; ++st) {
    if (st == 0) {
      const BlockSpec& last = P.blocks.back();
      for (int r = 0; r < 5; ++r) R.roles[r] = r;
      R.a_next = 0;
      R.side.restart();
      R.dout_fused_rows = 0;     // the last block's output gradient comes from the pool: its BatchNorm runs the stand-alone reduce
      if (any_work && dh) TRY(launch_avgpool_bwd(dh, c.G(0), P.F, last.Ho * last.Wo, last.Co, c.dt, s));
      if (any_work && !dh) {       // the embedding received no gradient
        const size_t bytes = (size_t)P.F * last.Ho * last.Wo * last.Co * (c.dt == DT_BF16 ? 2 : 4);
        if (hipMemsetAsync(c.G(0), 0, bytes, s) != hipSuccess) { set_last_error("resnet_backward: cannot clear the output gradient"); return 1; }
      }
    }
    for (int bi = (int)P.blocks.size() - 1; bi >= 0; --bi) {
      const BlockSpec& B = P.blocks[bi];
      if (B.stage != 3 - st || !block_has_work(P, R.work, B)) continue;
      if (dfeats && dfeats[B.stage] && ends_stage(P, bi)) {
        R3M_REQUIRE(R.dout_fused_rows == 0, "resnet_backward: BatchNorm partials of layer%d's output gradient were formed before the "
                    "feature-map gradient joined it", B.stage + 1);
        TRY(launch_feature_grad_add(dfeats[B.stage], c.G(0), P.F, B.Ho, B.Wo, B.Co, c.dt, s));
      }
      TRY(block_backward(c, bi));
    }
    if (st == 3 && stem_work) TRY(stem_backward(c, dx, dx_accumulate, dx ? stem_work : stem_work & ~BW_DGRAD));
    TRY(R.side.join());     // a finished stage's gradients are complete on the main stream (all-reduce hook, Adam)
  }
  R.next_stage = stage_end == 4 ? 0 : stage_end;
  return 0;
}

// ---- accessors for the C ABI ----
int plan_out_dim(Plan* P) { return P->D; }
int plan_input_hw(Plan* P, int* H, int* W) {
  if (H) *H = P->H;
  if (W) *W = P->W;
  return 0;
}
int plan_num_convs(Plan* P) { return (int)P->convs.size(); }
int plan_conv_info(Plan* P, int i, int* geo10) {
  R3M_REQUIRE(i >= 0 && i < (int)P->convs.size(), "conv_info: index %d out of range [0, %d)", i, (int)P->convs.size());
  const ConvSpec& c = P->convs[i];
  const int v[10] = {c.Ci, c.Co, c.k, c.stride, c.pad, c.Hi, c.Wi, c.Ho, c.Wo, 0};
  for (int k = 0; k < 10; ++k) geo10[k] = v[k];
  return 0;
}
int plan_feature_info(Plan* P, int layer, int* C, int* H, int* W) {
  R3M_REQUIRE(layer >= 1 && layer <= 4, "feature_info: layer %d outside 1..4", layer);
  for (size_t bi = 0; bi < P->blocks.size(); ++bi) {
    const BlockSpec& B = P->blocks[bi];
    if (B.stage != layer - 1 || !ends_stage(*P, bi)) continue;
    if (C) *C = B.Co;
    if (H) *H = B.Ho;
    if (W) *W = B.Wo;
    return 0;
  }
  set_last_error("feature_info: the plan has no layer%d", layer);
  return 1;
}
long long plan_coef_offset(Plan* P, int i) { return P->convs[i].coef_off; }
int plan_dtype(Plan* P) { return P->dtype; }
long long plan_num_params(Plan* P) { return P->n_params; }
long long plan_num_buffers(Plan* P) { return P->n_buffers; }
long long plan_arena_floats(Plan* P) { return P->arena_floats; }
int plan_num_tensors(Plan* P) { return (int)P->tensors.size(); }
int plan_tensor_info(Plan* P, int i, char* name, int cap, int* kind, long long* offset, int* ndim, int* shape4) {
  R3M_REQUIRE(i >= 0 && i < (int)P->tensors.size(), "tensor_info: index %d out of range", i);
  const TensorInfo& t = P->tensors[i];
  if (name && cap > 0) { strncpy(name, t.name.c_str(), cap - 1); name[cap - 1] = 0; }
  if (kind) *kind = t.kind;
  if (offset) *offset = t.offset;
  if (ndim) *ndim = t.ndim;
  if (shape4) for (int k = 0; k < 4; ++k) shape4[k] = t.shape[k];
  return 0;
}
// backward stage s covers layer (4 - s); stage 3 also covers the stem (its params sit before layer1's)
int plan_stage_range(Plan* P, int stage, long long* off, long long* count) {
  R3M_REQUIRE(stage >= 0 && stage < 4, "stage_range: stage %d", stage);
  const int L = 3 - stage;
  const long long b = P->stage_param_begin[L], e = P->stage_param_begin[L + 1];
  if (off) *off = b;
  if (count) *count = e - b;
  return 0;
}
int plan_set_trainable(Plan* P, const unsigned char* mask, int n) {
  R3M_REQUIRE(!(P->run.next_stage >= 1 && P->run.next_stage <= 3), "resnet_set_trainable: a backward is between its stages (stage %d is next); "
              "the mask changes between backwards", P->run.next_stage);
  if (!mask) { P->trainable.clear(); return 0; }
  R3M_REQUIRE(n == (int)P->tensors.size(), "resnet_set_trainable: n=%d, the plan has %d tensors (r3m_resnet_num_tensors)", n,
              (int)P->tensors.size());
  P->trainable.resize(n);
  for (int i = 0; i < n; ++i) P->trainable[i] = mask[i] ? 1 : 0;
  return 0;
}
int plan_debug_backward(Plan* P, int want_dx, int* flags_out, int cap) {
  const int n = (int)P->convs.size();
  if (cap < n) { set_last_error("debug_backward_plan: cap=%d, the plan has %d convolutions", cap, n); return -1; }
  std::vector<int> work;
  backward_work(*P, P->trainable.empty() ? nullptr : P->trainable.data(), want_dx != 0, work);
  for (int i = 0; i < n; ++i) flags_out[i] = work[i];
  return n;
}
void plan_destroy(Plan* P) {
  P->run.side.destroy();
  if (P->run.d_wt_tab) (void)hipFree(P->run.d_wt_tab);
  if (P->run.d_wt_tile0) (void)hipFree(P->run.d_wt_tile0);
  delete P;
}
int plan_set_bn_pair(Plan* P, int on) { const int old = P->bn_pair; P->bn_pair = on ? 1 : 0; return old; }
int plan_set_fuse_bnred(Plan* P, int on) { const int old = P->fuse_bnred; P->fuse_bnred = on ? 1 : 0; return old; }

}  // namespace r3m
