/* r3m_hip.h — C ABI of libr3m_hip.so, the MI355X (gfx950) hot path of R3M representation pre-training.
 *
 * The reference (facebookresearch/r3m, mounted at /root/reference) has no FFI of its own: everything below replaces
 * work the reference reaches through PyTorch / torchvision / torch.optim. Each entry point cites the reference call
 * site(s) whose arithmetic it takes over.  Conventions:
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless marked host;
 *   - no allocation, no ownership transfer, no hidden synchronisation: work is enqueued on `stream` and returns;
 *   - outputs and workspaces are pre-allocated by the caller (`*_workspace_bytes` / `*_arena_bytes` queries);
 *   - return 0 on success, non-zero on failure with a thread-local message in r3m_last_error();
 *   - activations are NHWC fp32, conv weights OHWI fp32 (= torch OIHW tensors with channels_last strides);
 *   - re-entrant; a `r3m_resnet_t` handle must not be used from two threads at once.
 */
#ifndef R3M_HIP_H
#define R3M_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* r3m_stream_t;  /* hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) */
typedef struct r3m_resnet* r3m_resnet_t;

int r3m_abi_version(void);
const char* r3m_last_error(void);

/* Measurement aid for bench.py (not part of the replaced reference surface): while enabled, every conv GEMM launch is
 * bracketed by HIP events on its own stream. Classes: 0 gather-GEMM 128x128 tile (conv fwd/dgrad, Linear), 1 gather-GEMM
 * 256x64 tile (64-channel layers), 2 wgrad 128x128, 3 wgrad 64x64. collect() sums elapsed ms / launches / algorithmic
 * FLOPs per class since the last collect (arrays of 4) and resets. */
int r3m_debug_occupancy(int* out4);   /* resident blocks/CU predicted for {gemm128x128, gemm128x128 8-wave, gemm256x64, wgrad128} */
/* Diagnostic: `blocks` workgroups of 256 threads that each hold `lds_bytes` of LDS and idle for `milliseconds` on `stream` — a stand-in
 * for another stream's long-running kernel (an RCCL collective overlapped with backward) when measuring how the compute kernels
 * behave with part of the CUs' LDS / wave slots taken (tools/occupy_ab.py). Returns immediately; does nothing else. */
int r3m_debug_occupy(int blocks, int lds_bytes, double milliseconds, r3m_stream_t stream);
/* Diagnostic: 0 = the encoder's persistent-kernel launches assign tiles statically, 1 (default) = per-XCD tile queues. Returns the old value. */
int r3m_debug_set_dynamic_tiles(int on);
/* Diagnostic (tests): the NEXT convolution launches of the calling thread draw their tiles from per-XCD tile queues, as every launch
   inside r3m_resnet_forward / _backward does (the operator entry points otherwise launch with the static tile split). counters:
   sets x 8 unsigned on the device, ZEROED by the caller on the stream of the launch; one set serves one launch (a stride-2 input
   gradient is up to four launches: pass 4 sets), sets nobody used are dropped after the last launch of the call. NULL takes them back
   (do that when the call they were meant for failed before it launched). Only the fp32 persistent kernel (routes 11 - 13) reads them,
   and only for launches of at least 64 row panels and 64 blocks: smaller ones keep the static split and leave the counters zero.
   Queue launches leave every counter of their set non-zero. */
void r3m_debug_next_launch_tile_queues(unsigned* counters, int sets);
/* Diagnostic, PROBE BUILDS ONLY (-DR3M_PROBES; the shipped library does not contain the kernel and returns -1): 1 = eligible bf16
   forward / dgrad launches run the round-5 persistent big-tile experiment csrc/conv_pw16.hip (pointwise + gather forms), 3 = + its
   3x3 window form; 0 = off. Measured not faster inside the step. Returns the old value. */
int r3m_debug_set_pw16(int mode);
/* Diagnostic (same-process A/B, tests): 1 (default) = the bf16 plans' 3x3 / stride-1 launches run the persistent kernel-row kernels of
   csrc/conv_row16.hip; 0 = the per-tile halo kernels of csrc/conv_bf16.hip (rounds 3-5). The two accumulate the taps in different orders:
   stored elements agree to 1 bf16 ulp, not bit for bit. Returns the old value. */
int r3m_debug_set_conv3x3_bf16(int mode);
/* Diagnostic (same-process A/B, tests): 1 (default) = forwards with training = 2 run the fused inference sequence; 0 = they run the
   training = 0 kernel sequence (conv, then a stand-alone BatchNorm + ReLU pass). Returns the old value. */
int r3m_debug_set_fused_inference(int on);
/* Diagnostic, runs without a GPU: which kernel family the gather-GEMM dispatch (csrc/conv.hip gg_route) picks for every launch of one
   convolution forward (dgrad = 0; flags: 1 = BatchNorm statistics) or input gradient (dgrad = 1; flags: 2 accumulate, 4 masked residual
   join, 64 BatchNorm-backward partials, mask_bits = 1: their ReLU mask comes as bits) — nothing is launched. routes[i]: 1 = 3x3 window
   kernel, 11 / 12 / 13 = persistent kernel (pointwise / gather / strided-output form), 20 = 16-wide-K kernel, 21 = gather kernel,
   22 = generic kernel; bf16 launches: 30 = gather kernel, 31 = per-tile 3x3 halo kernel, 32 = persistent
   kernel-row 3x3 kernel (csrc/conv_row16.hip). Returns the number of launches (a stride-2 dgrad has up to four), -1 on error. */
int r3m_debug_conv_route(int N, int H, int W, int Ci, int Co, int k, int stride, int pad, int dgrad, int flags, int mask_bits, int dtype,
                         int* routes, int cap);
/* Diagnostic, runs without a GPU: 1 when the inference forward of this convolution with epilogue `flags` (128 eval BatchNorm [| 2 add
   onto the residual in the output] [| 16 ReLU]) runs on a kernel built for those flags, so the engine stores the activated block
   output from the convolution itself; 0 when the engine runs that block's unfused sequence instead. r3m_debug_conv_route with the same
   flags (dgrad = 0) reports the route the fused launch takes. */
int r3m_debug_conv_fuses_affine(int N, int H, int W, int Ci, int Co, int k, int stride, int pad, int flags, int dtype);
/* Diagnostic, runs without a GPU: what the weight gradient of one convolution behind the stem (r3m_conv2d_wgrad_dt, the engine's
   backward) runs -- the plan of csrc/wgrad.hip wgrad_plan, the one dispatch of that kernel family; nothing is launched. out[0..8]:
     0  route: fp32 40 = one tap per block, rows linear in m (1x1 / stride 1), 41 = one tap per block, gathered rows, 42 = one kernel
        row (three taps) per block, 43 = kernel row from a shared input window (3x3 / stride 1 / pad 1); bf16 50 = one tap per block,
        51 = one kernel row per block, 52 = all nine taps per block
     1  tile width (128 | 64)     2  rows per K step     3  route 51: 1 = the division-free coordinate walk
     4  split-K factor (the workspace is split * Co * k * k * Ci floats)     5  GEMM rows per split
     6  ci tiles     7  blocks per split (the grid is out[7] * out[4] blocks)     8  dynamic LDS bytes (0: static LDS)
   Returns the number of ints written (9), -1 on error (cap < 9). */
int r3m_debug_wgrad_route(int N, int H, int W, int Ci, int Co, int k, int stride, int pad, int dtype, int* out, int cap);
/* Diagnostic, runs without a GPU: the launch geometry the streaming BatchNorm passes of csrc/bn.hip pick for a [rows][C] tensor of `dtype` (C a
   power of two >= 4) -- computed by the helpers the launchers themselves call, nothing is launched. out[0..13]:
     0-2   forward apply (r3m_bn_act_fwd_dt): elements per lane (4 | 8), items per block (span: 256 | 1024), blocks
     3-7   backward reduce (first pass of r3m_bn_bwd_dt): elements per lane, rows per block, rows per pass (rpp: the rows a block reads at
           once), column blocks (2 for fp32 at C = 2048), blocks = partial rows
     8-10  backward apply (second pass, also the paired one): elements per lane, span, blocks
     11    slices of the fp64 reduce over the backward's partial rows (out[7])
     12    slices of that reduce when `rows` itself is a partial-row count (r3m_bn_train_coeffs with stats_rows = rows,
           r3m_bn_bwd_from_partials_dt with partial_rows = rows)
     13    the cap on the slice count for this C (256 at C = 64 ... 64 at C = 2048)
   Returns the number of ints written (14), -1 on error (cap < 14, bad rows / C / dtype). */
int r3m_debug_bn_geometry(long long rows, int C, int dtype, int* out, int cap);
/* Diagnostic, runs without a GPU: the launch geometry of the fused stem tail of csrc/bn_pool.hip (r3m_bn_relu_maxpool_fwd_dt,
   r3m_bn_maxpool_bwd_dt) for y [N, Hi, Wi, C] of `dtype` -- the struct the launchers themselves launch from, nothing is launched. out[0..17]:
     0-1    pooled extents Ho, Wo
     2-6    forward: 1 = the bf16 row-walking kernel (C a power of two <= 2048), 0 = the one-output-per-thread kernel; segments of 8 output
            rows per frame (0 for the latter); blocks; threads per block; items per block (Wo * C / 8 for the row-walking kernel, whose
            threads loop over them; 256 for the other)
     7-14   backward reduce (first pass): quad rows per block rq; blocks = partial rows; threads; items per quad row (Wo * C / out[17]);
            threads per channel vector; the groups of the second LDS stage (min(out[11], 8)); dynamic LDS bytes; the partial rows the
            workspace of r3m_bn_workspace_bytes(N * Hi * Wi, C) holds (out[8] <= out[14])
     15-16  backward apply (second pass): blocks, threads
     17     elements per lane (4 fp32 | 8 bf16)
   The backward takes C a power of two in 8..1024; for any other C out[7..16] are 0 (r3m_bn_maxpool_bwd_dt refuses it).
   Returns the number of ints written (18), -1 on error (cap < 18, unknown dtype, N / Hi / Wi < 1, C not a positive multiple of 8). */
int r3m_debug_pool_geometry(int N, int Hi, int Wi, int C, int dtype, int* out, int cap);
void r3m_profile_enable(int on);
/* which kernel classes are bracketed while profiling is on: bit k = class k (0 conv fwd/dgrad 128-wide, 1 64-wide, 2 / 3 the weight
   gradients); default all. Each bracket costs the stream two event records. Returns the old mask. */
unsigned r3m_profile_classes(unsigned mask);
/* What the four classes contain (tests/test_gpu_profile.py pins it against tests/profile_model.py). Brackets sit in the dispatchers of the
   gather GEMM, of the weight gradients and of the stem's forward / weight gradient, so:
     - classes 0 / 1: one launch per convolution forward and per stride-1 input gradient, one per parity class of a strided input gradient
       (FLOPs 2 M N taps K with the taps of that class, taps on padding included); the stem forward is class 1; a bf16 3x3 launch on the
       kernel-row route is class 0 whatever its width. ALSO every Linear that runs as a 1x1 convolution: the hidden Linears of the reward
       head (r3m_langrew_forward / _backward / _call_*) and of the DistilBERT forward (r3m_text_forward), with taps = 1 and M, N, K = rows,
       outputs, inputs. A reader of bench.py's per-class lines finds them inside classes 0 / 1.
     - classes 2 / 3: one launch per weight gradient (the stem's is class 3; the reward head's Linears' too); the split-K reduce behind it is
       not bracketed.
     - in NO class: launches of the few-row split-K kernel (r3m_conv2d_fwd_affine_small, r3m_linear_fwd_small; r3m_resnet_forward_prepared
       counts only the convolutions the routing rule leaves or whose block does not run the fused sequence; likewise r3m_langrew_infer and
       r3m_text_forward_small), the stem's input gradient (a backward with dx counts no launch more than one without), and every
       BatchNorm, pooling, loss, optimizer, transpose and conversion kernel.
   A launcher that returns an error counts nothing. The open bracket belongs to the calling thread: launches from several threads (a
   backward on autograd's thread) are all counted. collect() sums per class since the last collect and resets; r3m_profile_enable(0)
   drops what was recorded and not yet collected. */
int r3m_profile_collect(double* ms, long long* launches, double* flops);
/* algorithmic HBM bytes per class of the launches of the last collect(): what each launch reads once plus what it writes once -- the input
   pixels some (output row, tap) pair reads (padding and pixels no tap reaches are no traffic), the weights of its taps, the result, and what
   its epilogue adds (statistics / partial rows, per-channel vectors, residuals, mask bits); a weight gradient: dY, the input pixels in range
   and its split-K slabs */
int r3m_profile_collect_bytes(double* bytes);
int r3m_profile_dump_to(const char* host_path);   /* also write one CSV row per launch at collect(); NULL/"" stops */

/* ---------------- encoder engine -----------------------------------------------------------------------------
 * Replaces torchvision.models.resnet{18,34,50}(pretrained=False) with fc=Identity as built by R3M.__init__
 * (r3m/models/models_r3m.py:44-52,62-63) and run by R3M.forward (models_r3m.py:84-100: x/255 -> Normalize -> convnet);
 * backward replaces autograd through that graph (r3m/trainer.py:157).                                            */
r3m_resnet_t r3m_resnet_create(int size /*18|34|50*/, int frames);
void r3m_resnet_destroy(r3m_resnet_t h);
int r3m_resnet_out_dim(r3m_resnet_t h);                 /* 512 | 512 | 2048 (models_r3m.py:45,48,51) */
long long r3m_resnet_num_params(r3m_resnet_t h);        /* floats in the flat parameter / gradient buffers */
long long r3m_resnet_num_buffers(r3m_resnet_t h);       /* floats in the flat running-statistics buffer */
long long r3m_resnet_arena_bytes(r3m_resnet_t h);       /* activation + scratch arena for `frames` */
int r3m_resnet_num_tensors(r3m_resnet_t h);
/* i-th tensor in torchvision state-dict order. kind: 0 conv weight (shape O,I,kh,kw; stored OHWI), 1 bn weight,
 * 2 bn bias (offsets into params), 3 running_mean, 4 running_var (offsets into buffers). */
int r3m_resnet_tensor_info(r3m_resnet_t h, int i, char* name, int name_cap, int* kind, long long* offset, int* ndim,
                           int* shape4);
/* backward stage s (0: avgpool+layer4, 1: layer3, 2: layer2, 3: layer1+stem) finishes params [offset, offset+count) */
int r3m_resnet_stage_range(r3m_resnet_t h, int stage, long long* offset, long long* count);
/* x: [frames,3,224,224] fp32 NCHW in 0..255 ([frames,3,H,W] for r3m_resnet_create_hw plans; models_r3m.py:96: "Input must be
 * [0, 255]"); h_out: [frames, out_dim].
 * training=1: batch statistics + running-stat update (momentum 0.1, eps 1e-5); 0: running statistics, everything a backward needs
 * kept (fine-tuning with frozen statistics); 2: INFERENCE — running statistics and nothing kept: BatchNorm, the residual join and the
 * ReLU are applied where each convolution stores its result (no raw conv outputs, no stand-alone BatchNorm passes, no mask bits), an
 * identity block's sum overwrites its input. What `load_r3m(...).eval()` under torch.no_grad() runs (/root/reference/r3m/__init__.py:
 * 72-75, r3m/example.py:19-33). fp32: bit-identical to training=0; bf16: one rounding per stored tensor instead of two (closer to
 * float64). r3m_resnet_backward after it returns an error. */
int r3m_resnet_forward(r3m_resnet_t h, const float* x, const float* params, float* buffers, void* arena, float* h_out,
                       int training, r3m_stream_t stream);
/* dh: [frames, out_dim]. Runs stages [stage_begin, stage_end) in order. The stages of one backward share state inside the plan
 * (the running output gradient, buffer roles, BatchNorm partials written by one stage's dgrad epilogues for the next): after
 * each forward they MUST be called in the order 0,1,2,3 (in one call or several); stage 0 may restart a backward over the same
 * forward at any time; any other out-of-order stage, or a backward before the first forward, returns non-zero.
 * accumulate=0 overwrites grads, 1 adds to them. */
/* The same forward fed from RAW clips through crop boxes: the rc / rctraj RandomResizedCrop(224) of the reference's loader
 * (r3m/utils/data_loaders.py:47-50,88-102) resampled INSIDE the stem pre-pass — one gather-bilinear pass from uint8 (or float
 * 0..255) frames [F,3,Hi,Wi] straight into the normalised stem image; the cropped fp32 frames are never materialised.
 * boxes[f / frames_per_box] = {top, left, height, width}; frames_per_box = 5 (rctraj: one box per clip) or 1 (rc).
 * Bit-identical to r3m_crop_resize followed by r3m_resnet_forward. */
int r3m_resnet_forward_crop(r3m_resnet_t h, const void* frames, int frames_are_u8, const int* boxes, int frames_per_box, int Hi,
                            int Wi, const float* params, float* buffers, void* arena, float* h_out, int training,
                            r3m_stream_t stream);
/* Per-plan switch of the backward schedule: 1 = the first pass of BatchNorm backward is computed inside the epilogue of the dgrad
 * that produces its dz (EPI_BNRED; default for fp32 plans), 0 = stand-alone reduce passes (default for bf16 plans, where the
 * fused form measured slower). Both schedules compute the same sums (different summation order). Returns the previous value. */
int r3m_resnet_set_fused_bn_reduce(r3m_resnet_t h, int on);
/* Per-plan switch: 1 (default) = the two BatchNorms that feed a downsample block's add + ReLU (the block's last one and the downsample
 * branch's) run their backward passes as ONE launch each — they see the same masked output gradient, which is then read once instead
 * of twice; 0 = separate passes. Bit-identical gradients either way. Returns the previous value. */
int r3m_resnet_set_bn_pair(r3m_resnet_t h, int on);
int r3m_resnet_backward(r3m_resnet_t h, const float* dh, const float* params, float* grads, void* arena, int stage_begin,
                        int stage_end, int accumulate, r3m_stream_t stream);
/* r3m_resnet_backward with two optional outputs (r3m_resnet_backward(...) == r3m_resnet_backward_ex(..., grads, ..., NULL, 0, stream)):
 *   grads == NULL : no parameter gradient is written and no weight-gradient launch is enqueued (frozen encoder); the BatchNorm
 *                   backward sums that dz still needs go to plan scratch (reserved in the arena at create time)
 *   dx != NULL    : d/d(frames) [frames,3,224,224] fp32 NCHW of the frames given to r3m_resnet_forward, written (dx_accumulate = 0)
 *                   or added to dx by the call that runs stage 3. Not available after r3m_resnet_forward_crop or an
 *                   inference-mode (training = 2) forward: returns non-zero. With frozen tensors (r3m_resnet_set_trainable) the
 *                   call that runs stage 0 plans the whole backward, so it must be given dx too (any call may carry it; only stage 3
 *                   writes it); with grads == NULL stage 0 assumes dx is wanted. A stage-3 call with a dx the plan of stage 0 did
 *                   not provide for (the gradient chain stopped above the stem) returns non-zero.
 * What autograd computes for obs.grad through the reference's R3M.forward (models_r3m.py:84-100): the encoder as a frozen,
 * differentiable reward or perceptual loss. */
int r3m_resnet_backward_ex(r3m_resnet_t h, const float* dh, const float* params, float* grads, void* arena, int stage_begin,
                           int stage_end, int accumulate, float* dx, int dx_accumulate, r3m_stream_t stream);
/* Partial-freeze fine-tuning (requires_grad_(False) on a sub-tree of the reference's autograd graph, models_r3m.py:44-52,99): mask is
 * a HOST array of n = r3m_resnet_num_tensors(h) bytes in r3m_resnet_tensor_info order, non-zero = the tensor wants a gradient (entries
 * of kinds 3 and 4 are ignored); NULL restores "all trainable", the default. The backward then enqueues only what the trainable
 * tensors (and dx) need: frozen weights get no weight-gradient launch and their range of grads is not written, frozen BatchNorm
 * parameter sums go to plan scratch, and everything below the lowest trainable tensor is skipped (a stage without work enqueues
 * nothing and returns 0). An all-zero mask behaves like grads == NULL. Host-only; takes effect at the next backward that begins with
 * stage 0; between the stages of a running backward it returns non-zero. */
int r3m_resnet_set_trainable(r3m_resnet_t h, const unsigned char* mask, int n);
/* Diagnostic, runs without a GPU: the work a backward under the current mask does per convolution (r3m_resnet_conv_info order), from
 * the predicate the backward itself executes. flags_out[i]: 1 = BatchNorm parameter sums (first pass), 2 = BatchNorm apply (dY is
 * formed), 4 = dgrad, 8 = wgrad. want_dx: the input gradient is asked for. Returns the number of convolutions, -1 on error. */
int r3m_debug_backward_plan(r3m_resnet_t h, int want_dx, int* flags_out, int cap);

/* Spatial feature maps: what the reference's users take from convnet.layer1 .. convnet.layer4 of the torchvision module built at
 * models_r3m.py:44-52 (a forward hook on convnet.layerk, nn.Sequential(*list(convnet.children())[:-2]), or calling the layers by hand).
 * Feature map k (1..4) is the output of torchvision's layer`k`: the activated output of that stage's last residual block, after the
 * add and the ReLU. It leaves the library as fp32 NCHW [frames, C, H, W] and its gradient enters as fp32 NCHW, for fp32 and bf16
 * plans alike (bf16 activations widen exactly; the gradient is added in fp32 and rounded once to the plan's storage type).
 *
 * Geometry of feature map `layer` for this plan. Needs no GPU. Non-zero for a layer outside 1..4. */
int r3m_resnet_feature_info(r3m_resnet_t h, int layer, int* C, int* H, int* W);
/* r3m_resnet_forward + fp32 NCHW copies of the requested stage outputs: feats[k-1] != NULL receives feature map k (feats is a HOST
 * array of four device pointers; NULL entries = not wanted; feats == NULL is r3m_resnet_forward, launch for launch). Every training
 * mode; in inference mode (training = 2) the copy is taken before a later block overwrites the map in place. */
int r3m_resnet_forward_features(r3m_resnet_t h, const float* x, const float* params, float* buffers, void* arena, float* h_out,
                                float* const feats[4], int training, r3m_stream_t stream);
/* PREPARED INFERENCE — a frozen encoder called on one image or a handful of frames at a time (/root/reference/r3m/example.py:19-33).
 * r3m_resnet_forward(training = 2) recomputes the eval-mode BatchNorm coefficients of every layer (one launch per convolution) and, on a
 * bf16 plan, re-converts all weights on every call, although both change only when parameters or running statistics do.
 *
 * r3m_resnet_inference_prepare writes the coefficients of every BatchNorm of the plan into the arena's coefficient blocks in ONE launch
 * (the layer table travels in the kernel arguments: no allocation, no host-to-device copy; bit for bit r3m_bn_eval_coeffs per layer)
 * and, for a bf16 plan, the bf16 weight image. It must be called again whenever params (bf16 plans), the BatchNorm parameters or
 * `buffers` change, and after ANY other forward of this plan on this arena (r3m_resnet_forward*, every training mode: they rewrite
 * the coefficient blocks), which r3m_resnet_forward_prepared detects and refuses. NOT detected: another plan that ran on the same
 * arena (plans of different frame counts or sizes lay it out differently) — prepare again after switching plans. */
int r3m_resnet_inference_prepare(r3m_resnet_t h, const float* params, const float* buffers, void* arena, r3m_stream_t stream);
/* Diagnostic (tests), needs no GPU: byte offset inside the arena of the coefficient block of convolution i (r3m_resnet_conv_info
 * order): [6][Co] floats, rows mean, invstd, scale, shift (what r3m_bn_eval_coeffs writes as coef[4][Co]) and two rows a backward
 * uses. -1 for an index out of range. */
long long r3m_debug_resnet_coef_offset(r3m_resnet_t h, int i);
/* Bytes of the caller-owned workspace of r3m_resnet_forward_prepared: the split-K tickets of every launch that the routing rule of
 * r3m_conv2d_fwd_affine_small takes, then one slab area sized for the largest of them. 0 for plans without such launches (bf16 plans,
 * large frame counts). Not part of the arena: r3m_resnet_arena_bytes and every arena offset are what they were. */
long long r3m_resnet_inference_workspace_bytes(r3m_resnet_t h);
/* The fused inference sequence of r3m_resnet_forward_features(training = 2) on a prepared arena: no coefficient launches, no weight
 * conversion; the fp32 weights are read live from params. flags bit 0 set: every convolution runs the kernel it runs in
 * r3m_resnet_forward (results bit-identical to it, embedding and feature maps). Bit 0 clear, fp32 plans: the launches the routing rule
 * takes run the small-M split-K kernel instead (one hipMemsetAsync over the tickets per call; workspace must hold
 * r3m_resnet_inference_workspace_bytes; results deterministic, within the fp32 ceiling of the other kernels but not their bits: K is
 * summed in another order). bf16 plans run exactly today's kernels either way. workspace may be NULL when the plan needs none or bit 0
 * is set. r3m_resnet_backward after it returns the "inference mode" error. */
int r3m_resnet_forward_prepared(r3m_resnet_t h, const float* x, const float* params, void* arena, void* workspace, float* h_out,
                                float* const feats[4], int flags, r3m_stream_t stream);
/* r3m_resnet_backward_ex + the gradients w.r.t. those outputs: dfeats[k-1] != NULL (HOST array of four device pointers, fp32 NCHW) is
 * added to the running output gradient where autograd adds it, immediately before the backward of that stage's last block — what
 * loss.backward() does for a loss that reads convnet.layerk's output. dh == NULL: no gradient reaches the embedding (zeros flow down
 * from the pool). Staged calls carry the same dfeats array; the stage that owns an entry (stage 4 - k) reads it. An entry whose
 * block has no work under the trainable mask (frozen prefix, no dx) is dropped. After an inference-mode forward: non-zero. */
int r3m_resnet_backward_features(r3m_resnet_t h, const float* dh, const float* const dfeats[4], const float* params, float* grads,
                                 void* arena, int stage_begin, int stage_end, int accumulate, float* dx, int dx_accumulate,
                                 r3m_stream_t stream);
/* The two kernels one by one (tests, tools/feature_bench.py). z / g: NHWC [N,H,W,C] fp32 (dtype 0) or bf16 (dtype 1); out / d: fp32
 * NCHW [N,C,H,W]. export: out = z.permute(0,3,1,2).float(), bit for bit. grad_add: g = (g.float() + d.permute(0,2,3,1)).to(dtype),
 * one fp32 add and one rounding per element, no atomics. C must be a multiple of 64, N, H, W >= 1. z / g must be 16-byte aligned;
 * out / d need only float alignment, except for H * W = 1 (both layouts are the same bytes and both sides move 16 bytes at a
 * time), where they must be 16-byte aligned too. Bad arguments return non-zero before any launch. */
int r3m_feature_export_dt(const void* z_nhwc, float* out_nchw, int N, int H, int W, int C, int dtype, r3m_stream_t stream);
int r3m_feature_grad_add_dt(const float* d_nchw, void* g_nhwc, int N, int H, int W, int C, int dtype, r3m_stream_t stream);

/* ---------------- single operators (parity-tested one by one) -------------------------------------------------
 * conv2d fwd / dgrad / wgrad: ATen conv2d + autograd under torchvision ResNet.forward (call site models_r3m.py:99). */
int r3m_conv2d_stats_rows(int N, int Hi, int Wi, int Co, int k, int stride, int pad);
/* stats (optional): [stats_rows][2][Co] per-row-block sum / sum of squares of y (BatchNorm statistics partials) */
int r3m_conv2d_fwd(const float* x, const float* w_ohwi, float* y, float* stats, int N, int Hi, int Wi, int Ci, int Co, int k,
                   int stride, int pad, r3m_stream_t stream);
size_t r3m_conv2d_dgrad_workspace_bytes(int Ci, int Co, int k);
int r3m_conv2d_dgrad(const float* dy, const float* w_ohwi, float* dx, void* workspace, size_t workspace_bytes, int N, int Hi,
                     int Wi, int Ci, int Co, int k, int stride, int pad, r3m_stream_t stream);
size_t r3m_conv2d_wgrad_workspace_bytes(int N, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad);
int r3m_conv2d_wgrad(const float* x, const float* dy, float* dw_ohwi, void* workspace, size_t workspace_bytes, int N, int Hi,
                     int Wi, int Ci, int Co, int k, int stride, int pad, int accumulate, r3m_stream_t stream);
/* the stem as the engine runs it (models_r3m.py:97-99 + torchvision conv1), no patch matrix in HBM:
 *   r3m_stem_prep      x [frames,3,224,224] fp32 NCHW in 0..255 -> xn [frames,224,224,3] = (x/255 - mean)/std (NHWC)
 *   r3m_stem_conv_fwd  xn, w_ohwi [64,7,7,3] -> y [frames,112,112,64] (NHWC) (+ BatchNorm partials [frames*49][2][64])
 *   r3m_stem_conv_wgrad  xn, dy (same layout as y) -> dw_ohwi [64,7,7,3] */
int r3m_stem_prep(const float* x_nchw, float* xn, int frames, r3m_stream_t stream);
int r3m_stem_conv_fwd(const float* xn, const float* w_ohwi, float* y, float* stats, int frames, r3m_stream_t stream);
size_t r3m_stem_conv_wgrad_workspace_bytes(void);
int r3m_stem_conv_wgrad(const float* xn, const float* dy, float* dw_ohwi, void* workspace, size_t workspace_bytes, int frames,
                        int accumulate, r3m_stream_t stream);
/* input gradient of the stem (x/255 -> Normalize -> conv1): dz [frames,112,112,64] NHWC, fp32 (dz_dtype R3M_DT_F32) or bf16
 * (R3M_DT_BF16), w_ohwi [64,7,7,3] fp32 -> dx_nchw [frames,3,224,224] fp32 = d/d(frames in 0..255); accumulate: 0 writes, 1 adds.
 * fp32 accumulation; the bf16 rounding of the normalised frames in bf16 plans is taken as identity (as autocast does). */
int r3m_stem_input_grad(const void* dz, int dz_dtype, const float* w_ohwi, float* dx_nchw, int frames, int accumulate,
                        r3m_stream_t stream);

/* BatchNorm2d(eps, momentum) train/eval + ReLU + residual add (torchvision BasicBlock/Bottleneck).
 * coef: [4][C] = mean, invstd, scale = gamma*invstd, shift = beta - mean*scale. */
size_t r3m_bn_workspace_bytes(long long rows, int C);
/* stats: [stats_rows][2][C] fp32 partial sums / sums of squares of y over any blocking of the rows (a conv epilogue's); they are added up
 * in fp64: mean = sum / count, var = max(sumsq / count - mean^2, 0) (biased), coef from their fp32 values. running_mean / running_var
 * (both or neither; NULL: not updated) move by `momentum` towards mean and var * count / (count - 1).
 * count = 1 (one frame at 32 x 32 reaches it in layer4; torch refuses it in training mode): defined here as the variance of the single
 * value -- 0 up to the rounding of the partials, never negative -- with the unbiased factor taken as 1 instead of 1 / 0, so invstd is
 * at most 1 / sqrt(eps) and every output, the running statistics included, stays finite. */
int r3m_bn_train_coeffs(const float* stats, int stats_rows, long long count, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps, float* coef, void* workspace,
                        size_t workspace_bytes, int C, r3m_stream_t stream);
int r3m_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                       float* coef, int C, r3m_stream_t stream);
/* z = [relu](scale*y + shift [+ r] [+ scale2*y2 + shift2]) ; pass r for the identity branch, or y2+coef2 for a
 * downsample branch (then r must be NULL). maskbits (optional): 1 bit per element = [z > 0], rows*C/8 bytes (float4 index i
 * owns nibble i&7 of 32-bit word i>>3) — what the backward reads instead of z. */
int r3m_bn_act_fwd(const float* y, const float* coef, const float* r, const float* y2, const float* coef2, float* z,
                   long long rows, int C, int relu, unsigned* maskbits, r3m_stream_t stream);
/* g = dz * [mask], mask = zbits (bit mask from r3m_bn_act_fwd) if given, else (zmask > 0) if given, else
 * (scale*y+shift > 0); dgamma = sum g*yhat, dbeta = sum g,
 * dy = scale*(g - mean(g) - yhat*mean(g*yhat)) (batch stats) or scale*g (use_batch_stats=0). */
int r3m_bn_bwd(const float* dz, const float* zmask, const unsigned* zbits, const float* y, const float* coef, float* dgamma,
               float* dbeta, float* dy, void* workspace, size_t workspace_bytes, long long rows, int C, int use_batch_stats, int accumulate,
               r3m_stream_t stream);
/* MaxPool2d(3,2,1) and AdaptiveAvgPool2d(1)+flatten, NHWC */
int r3m_maxpool_fwd(const float* z, float* p, unsigned char* argmax, int N, int Hi, int Wi, int C, r3m_stream_t stream);
int r3m_maxpool_bwd(const float* dp, const unsigned char* argmax, float* dz, int N, int Hi, int Wi, int C, r3m_stream_t stream);
int r3m_avgpool_fwd(const float* x, float* h, int N, int HW, int C, r3m_stream_t stream);
int r3m_avgpool_bwd(const float* dh, float* dx, int N, int HW, int C, r3m_stream_t stream);

/* ---------------- mixed precision: bf16 activations (BASELINE configs[2], [4]) -------------------------------------
 * The `_dt` variants take `dtype`: R3M_DT_F32 (identical to the plain entry points above) or R3M_DT_BF16. With bf16 every
 * ACTIVATION tensor (x, y, z, r, dy, dz, dx, dp ...) is NHWC bfloat16; what stays fp32: master weights, weight / BatchNorm
 * gradients, BatchNorm statistics partials and coefficients, the embedding h / dh, and all
 * accumulation (v_mfma_f32_32x32x16_bf16). This is the counterpart of running the reference's encoder call
 * (r3m/models/models_r3m.py:99, backward at r3m/trainer.py:157) under torch.autocast(bfloat16); the reference itself is
 * fp32 only. Channel counts must be multiples of 64 (every ResNet-18/34/50 layer behind the stem is).
 *   r3m_conv2d_fwd_dt    w: bf16 [Co][k][k][Ci] for R3M_DT_BF16 (make it with r3m_convert_bf16 from the fp32 master)
 *   r3m_conv2d_dgrad_dt  w: the fp32 master [Co][k][k][Ci] (transposed + converted into the workspace)
 *   r3m_conv2d_wgrad_dt  dw: fp32 */
enum { R3M_DT_F32 = 0, R3M_DT_BF16 = 1 };
r3m_resnet_t r3m_resnet_create_dt(int size /*18|34|50*/, int frames, int dtype);
int r3m_resnet_dtype(r3m_resnet_t h);
/* Native resolution: a plan for frames [frames,3,height,width], any height and width in 32..512 (torchvision's ResNet takes any size:
 * every layer's output is floor((n + 2 pad - k) / stride) + 1 per dimension, the global average pool ends in [frames, out_dim]).
 * r3m_resnet_create_hw(size, frames, dtype, 224, 224) is r3m_resnet_create_dt(size, frames, dtype): same plan, same arena, same kernels.
 * Other sizes run the general stem kernels (csrc/stem_gen.hip) and the same layer kernels as 224. r3m_resnet_forward / _backward(_ex)
 * then take x and dx as [frames,3,height,width]; r3m_resnet_forward_crop (224 crops) returns an error on a plan that is not 224 x 224.
 * Returns NULL with r3m_last_error() set for sizes outside 32..512 and when some tensor of the plan would hold 2^31 elements or more
 * (the kernels index with 32-bit integers). Needs no GPU. */
r3m_resnet_t r3m_resnet_create_hw(int size /*18|34|50*/, int frames, int dtype, int height, int width);
int r3m_resnet_input_hw(r3m_resnet_t h, int* height, int* width);
/* Read-only geometry of convolution i (0 = conv1, then torchvision's module order of each block: conv1, conv2[, conv3][, downsample.0]):
 * channels in / out, kernel size, stride, pad, input and output height / width. r3m_resnet_num_convs gives the count. Needs no GPU. */
int r3m_resnet_num_convs(r3m_resnet_t h);
int r3m_resnet_conv_info(r3m_resnet_t h, int i, int* Ci, int* Co, int* k, int* stride, int* pad, int* Hi, int* Wi, int* Ho, int* Wo);
/* Diagnostic (same-process A/B, tests): 1 = forwards of 224 x 224 plans run the general stem kernels too (the frames must come through
 * r3m_resnet_forward; the backward follows what the last forward ran); 0 (default) = the 224-specialised stem. Returns the old value. */
int r3m_debug_set_generic_stem(int on);
/* The general stem kernels one by one (tests, tools/resolution_bench.py). xn: the normalised image [F][H][W*3], fp32 (dtype 0) or bf16
 * (dtype 1), r3m_stem_gen_image_bytes() long; w147: fp32 conv1 weights OHWI [64][7][7][3]; y / dy: [F,Ho,Wo,64] of the dtype;
 * stats (optional): BatchNorm partial rows [ceil(F Ho Wo / 256)][2][64] (sum, sum of squares); ws: r3m_stem_gen_wgrad_ws_bytes();
 * dx: fp32 NCHW [F,3,H,W]. */
size_t r3m_stem_gen_image_bytes(int F, int H, int W, int dtype);
size_t r3m_stem_gen_wgrad_ws_bytes(void);
int r3m_stem_gen_prep(const float* x_nchw, void* xn, int F, int H, int W, int dtype, r3m_stream_t stream);
int r3m_stem_gen_fwd(const void* xn, const float* w147, void* y, float* stats, int F, int H, int W, int dtype, r3m_stream_t stream);
int r3m_stem_gen_wgrad(const void* xn, const void* dy, float* dw147, void* ws, int F, int H, int W, int accumulate, int dtype,
                       r3m_stream_t stream);
int r3m_stem_gen_input_grad(const void* dy, const float* w147, float* dx, int F, int H, int W, int accumulate, int dtype,
                            r3m_stream_t stream);
/* LDS bytes per block of the three general stem kernels at F x H x W (at most 160 KiB over the supported range). Needs no GPU. */
int r3m_stem_gen_lds_bytes(int F, int H, int W, int* fwd, int* wgrad, int* input_grad);
int r3m_convert_bf16(const float* src, void* dst_bf16, long long n /* multiple of 4 */, r3m_stream_t stream);
int r3m_conv2d_fwd_dt(const void* x, const void* w_ohwi, void* y, float* stats, int N, int Hi, int Wi, int Ci, int Co, int k,
                      int stride, int pad, int dtype, r3m_stream_t stream);
int r3m_conv2d_dgrad_dt(const void* dy, const float* w_ohwi, void* dx, void* workspace, size_t workspace_bytes, int N, int Hi,
                        int Wi, int Ci, int Co, int k, int stride, int pad, int dtype, r3m_stream_t stream);
/* dgrad whose epilogue ALSO emits the first pass of the consumer BatchNorm's backward (what the engine runs for every BatchNorm
 * whose dz has one producing dgrad): dx [N,Hi,Wi,Ci] is the gradient entering BatchNorm(+ReLU) with pre-normalisation input bn_y
 * (same shape / dtype as dx) — optionally plus a masked residual gradient (dx = dgrad + residual_grad * [residual_bits], the
 * join at a block input). partials [r3m_conv2d_dgrad_bnred_rows][2][Ci] (fp32): per 64 result rows, sum(g) and
 * sum(g * (y - mean)) with g = dx * [mask]; mask = bn_bits (1 bit per element of the BatchNorm's block output) or, when
 * bn_bits is NULL, recomputed as fma(y, bn_scale, bn_shift) > 0. Equals r3m_bn_bwd's reduce pass on the stored dx
 * (replaces torch's batch_norm_backward reduction under the ResNet graph, call site trainer.py:157). */
int r3m_conv2d_dgrad_bnred_rows(int N, int Hi, int Wi, int stride);
int r3m_conv2d_dgrad_bnred_dt(const void* dy, const float* w_ohwi, void* dx, void* workspace, size_t workspace_bytes, int N, int Hi,
                              int Wi, int Ci, int Co, int k, int stride, int pad, const void* residual_grad,
                              const unsigned* residual_bits, const void* bn_y, const unsigned* bn_bits, const float* bn_scale,
                              const float* bn_shift, const float* bn_mean, float* partials, int dtype, r3m_stream_t stream);
/* The two input-gradient epilogues of a residual block's entry that only the engine launched so far (tests), through the launcher
 * the engine calls, the weight image made in the workspace as r3m_conv2d_dgrad_dt does:
 *   accumulate = 1                 dx += dgrad: the downsample branch (k = 1, pad 0, stride 1 or 2) adding onto the input gradient the
 *                                  block's first convolution stored. A strided 1x1 leaves the pixels without taps untouched.
 *   residual_grad, residual_bits   dx = dgrad + residual_grad * [residual_bits]: the join at the input of an identity block (stride 1)
 *                                  without BatchNorm partials (every identity block of a bf16 plan, the first block of an fp32 plan).
 *                                  residual_grad: [N,Hi,Wi,Ci] of the dtype; residual_bits: 1 bit per element, required (the engine
 *                                  always passes the block output's mask bits).
 * Exactly one of the two. */
int r3m_conv2d_dgrad_join_dt(const void* dy, const float* w_ohwi, void* dx, void* workspace, size_t workspace_bytes, int N, int Hi,
                             int Wi, int Ci, int Co, int k, int stride, int pad, int accumulate, const void* residual_grad,
                             const unsigned* residual_bits, int dtype, r3m_stream_t stream);
/* The small-M inference forward of one convolution (csrc/conv_small.hip): out = [relu](conv(x, w) * scale[co] + shift[co] [+ out]) like
 * r3m_conv2d_fwd_affine_dt, fp32 only, for launches of few GEMM rows (N * Ho * Wo): 16-, 32- or 64-row x 64-column tiles on the exact
 * fp32 MFMA, K (taps x Ci / 32 chunks) cut into S slices, one block per (tile, slice), about 1/2 - 1 x the CU count in all. Each slice
 * block writes an fp32 slab to the workspace, releases once and draws a ticket; the block that draws the last ticket of its tile sums
 * the S slabs in slice order and stores. No block waits for another and nothing is added with floating-point atomics: the same
 * operands give the same bits on every launch. S = 1 uses neither ticket nor slab.
 * Takes k in {1, 3} (pad k / 2), stride in {1, 2}, Ci a multiple of 32, Co a multiple of 64, at most 65536 rows, flags 128, 128|16 or
 * 128|2|16; anything else returns non-zero with a message. split = 0: S by the rule; split > 0 (tests): S forced, at most the tenth
 * value of r3m_debug_conv_small_plan. workspace: r3m_conv2d_small_workspace_bytes for the same split; the entry zeroes the tickets it
 * uses with one hipMemsetAsync on `stream`. */
size_t r3m_conv2d_small_workspace_bytes(int N, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad, int split);
int r3m_conv2d_fwd_affine_small(const float* x, const float* w_ohwi, float* out, const float* scale, const float* shift, int N, int Hi,
                                int Wi, int Ci, int Co, int k, int stride, int pad, int flags, int split, void* workspace,
                                size_t workspace_bytes, r3m_stream_t stream);
/* Diagnostic, runs without a GPU and launches nothing: what that entry runs with split = 0. out[0..9] = {the routing rule of
 * r3m_resnet_forward_prepared takes this launch (a pure function of the geometry), tile rows, tile columns, S, grid (blocks), K chunks
 * per slice, row tiles, column tiles, K chunks in all, largest split accepted}; all zero for a shape the kernel does not take.
 * Returns 10, -1 on error. */
int r3m_debug_conv_small_plan(int N, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad, int flags, int* out, int cap);
/* The inference forward of one convolution, as r3m_resnet_forward(training = 2) launches it (tests): out = [relu](conv(x, w) * scale[co]
 * + shift[co] [+ out]) stored by the convolution kernel itself, rounded once for bf16. flags: 128 (eval BatchNorm: the downsample
 * branch), 128 | 16 (+ ReLU: inner convolutions), 128 | 2 | 16 (+ the residual, which `out` holds on entry: a block's last
 * convolution). x, w as r3m_conv2d_fwd_dt; scale, shift: fp32 [Co]. Returns non-zero with a message where
 * r3m_debug_conv_fuses_affine answers 0: the engine does not make that launch (it runs conv + r3m_bn_act_fwd instead). */
int r3m_conv2d_fwd_affine_dt(const void* x, const void* w_ohwi, void* out, const float* scale, const float* shift, int N, int Hi, int Wi,
                             int Ci, int Co, int k, int stride, int pad, int flags, int dtype, r3m_stream_t stream);
size_t r3m_conv2d_wgrad_workspace_bytes_dt(int N, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad, int dtype);
int r3m_conv2d_wgrad_dt(const void* x, const void* dy, float* dw_ohwi, void* workspace, size_t workspace_bytes, int N, int Hi,
                        int Wi, int Ci, int Co, int k, int stride, int pad, int accumulate, int dtype, r3m_stream_t stream);
int r3m_stem_conv_fwd_dt(const float* xn, const float* w_ohwi, void* y, float* stats, int frames, int dtype, r3m_stream_t stream);
int r3m_stem_conv_wgrad_dt(const float* xn, const void* dy, float* dw_ohwi, void* workspace, size_t workspace_bytes, int frames,
                           int accumulate, int dtype, r3m_stream_t stream);
/* The stem on the bf16 MFMA (bf16 plans): r3m_stem_prep_bf16 writes the normalised frames as a padded, channel-interleaved bf16
 * image xn16[frames][232][704] (r3m_stem_xn16_bytes), from which conv1 forward (y: bf16 [frames,112,112,64], stats as above) and its
 * weight gradient (dy bf16, dw fp32 [64,7,7,3]) stage their operands by plain contiguous copies. Same call sites as r3m_stem_*. */
size_t r3m_stem_xn16_bytes(int frames);
int r3m_stem_prep_bf16(const float* x_nchw, void* xn16, int frames, r3m_stream_t stream);
/* The same pre-pass reading RAW clips through crop boxes (what r3m_resnet_forward_crop runs first): frames [F,3,Hi,Wi] uint8 or
 * float 0..255, boxes[f / frames_per_box] = {top, left, height, width}; dtype R3M_DT_F32 writes xn (layout of r3m_stem_prep),
 * R3M_DT_BF16 writes xn16 (layout of r3m_stem_prep_bf16). Bit-identical to r3m_crop_resize followed by r3m_stem_prep[_bf16]. */
int r3m_stem_prep_crop(const void* frames, int frames_are_u8, const int* boxes, int frames_per_box, int Hi, int Wi, void* xn_out,
                       int F, int dtype, r3m_stream_t stream);
int r3m_stem_conv_fwd_bf16(const void* xn16, const float* w_ohwi, void* y, float* stats, int frames, r3m_stream_t stream);
size_t r3m_stem_conv_wgrad_bf16_workspace_bytes(void);
int r3m_stem_conv_wgrad_bf16(const void* xn16, const void* dy, float* dw_ohwi, void* workspace, size_t workspace_bytes, int frames,
                             int accumulate, r3m_stream_t stream);
/* The BatchNorm entry points check their arguments, carve the workspace and run the host sequences of csrc/bn.hip / bn_pool.hip
 * (bn_train_coeffs, bn_bwd, bn_bwd_pair, bn_bwd_pool), which are the launch sequences of the engine's training step. */
int r3m_bn_act_fwd_dt(const void* y, const float* coef, const void* r, const void* y2, const float* coef2, void* z,
                      long long rows, int C, int relu, unsigned* maskbits, int dtype, r3m_stream_t stream);
int r3m_bn_bwd_dt(const void* dz, const void* zmask, const unsigned* zbits, const void* y, const float* coef, float* dgamma,
                  float* dbeta, void* dy, void* workspace, size_t workspace_bytes, long long rows, int C, int use_batch_stats,
                  int accumulate, int dtype, r3m_stream_t stream);
/* The backward of the TWO BatchNorms that feed a downsample block's add + ReLU, out = relu(bn_a(y_a) + bn_b(y_b)), as the engine runs it
 * with r3m_resnet_set_bn_pair on (tests): both see g = dz * [zbits] (mask bits of the block output, required). The first passes run as
 * one launch where the library has one (bf16, C a multiple of 8), else one after the other; the second passes always run as one launch
 * that reads dz and the bits once. coef_a / coef_b: [6][C] -- rows 0-3 as r3m_bn_*_coeffs write them, rows 4 and 5 RECEIVE c1 = mean(g)
 * and c2 = mean(g yhat) (0 with use_batch_stats = 0), the engine's coefficient block. dy_a / dy_b equal two r3m_bn_bwd_dt calls bit for
 * bit; dgamma / dbeta equal them bit for bit where the first passes ran one after the other, to rounding where the joint one ran.
 * workspace = r3m_bn_pair_workspace_bytes(rows, C). C >= 8. */
size_t r3m_bn_pair_workspace_bytes(long long rows, int C);
int r3m_bn_bwd_pair_dt(const void* dz, const unsigned* zbits, const void* y_a, float* coef_a, const void* y_b, float* coef_b,
                       float* dgamma_a, float* dbeta_a, void* dy_a, float* dgamma_b, float* dbeta_b, void* dy_b, void* workspace,
                       size_t workspace_bytes, long long rows, int C, int use_batch_stats, int accumulate, int dtype, r3m_stream_t stream);
/* BatchNorm backward whose first pass a dgrad epilogue already ran (the fp32 plans' default schedule, tests): partials
 * [partial_rows][2][C] as r3m_conv2d_dgrad_bnred_dt writes them -- sum(g) and sum(g (y - mean)) over any blocking of the rows -- are
 * added up in fp64, the second sum times invstd gives sum(g yhat); then dgamma / dbeta (accumulate: 0 writes, 1 adds) and the second
 * pass dy, as r3m_bn_bwd_dt. The mask comes as zbits or, when NULL, is recomputed from y. workspace = r3m_bn_workspace_bytes(rows, C). */
int r3m_bn_bwd_from_partials_dt(const void* dz, const unsigned* zbits, const void* y, const float* coef, const float* partials,
                                int partial_rows, float* dgamma, float* dbeta, void* dy, void* workspace, size_t workspace_bytes,
                                long long rows, int C, int use_batch_stats, int accumulate, int dtype, r3m_stream_t stream);
/* Stem tail fused (what the engine runs after conv1): z = relu(bn(y)) is pooled on the fly — the activated tensor and its
 * gradient, the two largest tensors of the network, are never written. Same arithmetic as r3m_bn_act_fwd + r3m_maxpool_fwd and
 * r3m_maxpool_bwd + r3m_bn_bwd (mask recomputed from y); workspace = r3m_bn_workspace_bytes(N*Hi*Wi, C). */
int r3m_bn_relu_maxpool_fwd_dt(const void* y, const float* coef, void* p, unsigned char* argmax, int N, int Hi, int Wi, int C,
                               int dtype, r3m_stream_t stream);
int r3m_bn_maxpool_bwd_dt(const void* dp, const unsigned char* argmax, const void* y, const float* coef, float* dgamma, float* dbeta,
                          void* dy, void* workspace, size_t workspace_bytes, int N, int Hi, int Wi, int C, int use_batch_stats,
                          int accumulate, int dtype, r3m_stream_t stream);
int r3m_maxpool_fwd_dt(const void* z, void* p, unsigned char* argmax, int N, int Hi, int Wi, int C, int dtype, r3m_stream_t stream);
int r3m_maxpool_bwd_dt(const void* dp, const unsigned char* argmax, void* dz, int N, int Hi, int Wi, int C, int dtype,
                       r3m_stream_t stream);
int r3m_avgpool_fwd_dt(const void* x, float* h, int N, int HW, int C, int dtype, r3m_stream_t stream);
int r3m_avgpool_bwd_dt(const float* dh, void* dx, int N, int HW, int C, int dtype, r3m_stream_t stream);

/* nn.Linear (+ReLU) of LanguageReward.pred (r3m/models/models_language.py:43-51): y[M,N] = x[M,K] w[N,K]^T + b */
int r3m_linear_fwd(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int relu,
                   r3m_stream_t stream);
/* The same Linear over FEW rows on the split-K kernel of csrc/conv_small.hip: the launch of the 1 x 1 geometry (M, 1, 1, K, N, 1, 1, 0),
 * with that kernel's tiles, slices, slabs and tickets (r3m_conv2d_fwd_affine_small) and a Linear store in place of the affine one.
 * flags: 8 (y = x w^T + bias), 8 | 16 (+ ReLU: the reward head), 8 | 256 (the exact GELU 0.5 v (1 + erf(v / sqrt 2)) of v = acc + bias:
 * the text model's lin1). Takes K a multiple of 32, N a multiple of 64, 1 <= M <= 65536; a convolution flag set (128 ...) or anything
 * else returns non-zero with a message. split and workspace as r3m_conv2d_fwd_affine_small: split = 0 is the rule's S, the workspace is
 * r3m_linear_small_workspace_bytes for the same split (0 for a shape the kernel refuses), and the entry zeroes its tickets with one
 * hipMemsetAsync on `stream`. The same operands give the same bits on every launch. */
size_t r3m_linear_small_workspace_bytes(int M, int K, int N, int split);
int r3m_linear_fwd_small(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int flags, int split,
                         void* workspace, size_t workspace_bytes, r3m_stream_t stream);
/* Diagnostic, runs without a GPU and launches nothing: the ten integers of r3m_debug_conv_small_plan for that Linear (one planner: it
 * IS the plan of the 1 x 1 geometry); out[0] is the routing rule r3m_langrew_infer and r3m_text_forward_small follow. All zero for a
 * shape or a flag set the Linear entry refuses. Returns 10, -1 on error. */
int r3m_debug_linear_small_plan(int M, int K, int N, int flags, int* out, int cap);

/* RandomResizedCrop resample of the rc / rctraj augmentations (r3m/utils/data_loaders.py:47-50,81-102): crop box
 * boxes[n / frames_per_box] = {top, left, height, width} (host-drawn), bilinear resize to Ho x Wo (align_corners=False),
 * on x/255, result * 255. frames: [N,C,Hi,Wi] uint8 or float in 0..255; out: [N,C,Ho,Wo] float. frames_per_box = 5 for
 * rctraj (one box per clip), 1 for rc. Every box must lie inside its frame (not checked). This call and r3m_resize_crop refuse
 * Hi, Wi, C < 1 and N, Ho, Wo < 0 before any launch; N, Ho or Wo of 0 is an empty call. */
int r3m_crop_resize(const void* frames, int frames_are_u8, const int* boxes, float* out, long long N, int C, int Hi, int Wi,
                    int Ho, int Wo, int frames_per_box, r3m_stream_t stream);
/* R3M.forward's branch for inputs that are not 224 x 224 (r3m/models/models_r3m.py:85-90: transforms.Resize(256) +
 * CenterCrop(224) on x/255): bilinear resize of the whole frame to resized_h x resized_w (align_corners=False, no antialias) of
 * which only the Ho x Wo window at (top, left) is computed. frames [N,C,Hi,Wi] uint8 or float 0..255 -> out [N,C,Ho,Wo] float
 * 0..255. The caller derives resized_h/w and the window with torchvision's rounding (r3m_amd/augment.py). */
int r3m_resize_crop(const void* frames, int frames_are_u8, float* out, long long N, int C, int Hi, int Wi, int resized_h,
                    int resized_w, int top, int left, int Ho, int Wo, r3m_stream_t stream);
/* Adjoint of r3m_resize_crop for float frames: dout [N,C,Ho,Wo] -> din [N,C,Hi,Wi] (accumulate: 0 writes, 1 adds). A gather (each
 * input pixel sums the <= 2 x 2 taps per window pixel that sampled it, same source-index arithmetic as the forward): no atomics,
 * the same bits on every run. uint8 frames carry no gradient. */
int r3m_resize_crop_backward(const float* dout, float* din, long long N, int C, int Hi, int Wi, int resized_h, int resized_w, int top,
                             int left, int Ho, int Wo, int accumulate, r3m_stream_t stream);

/* LanguageReward, all 15 evaluations of a step batched (r3m/trainer.py:72-92 calling r3m/models/models_r3m.py:78-81 and
 * r3m/models/models_language.py:43-55). alle [B,5,D]; feats [B,lang_dim] = frozen sentence features (LangEncoder output,
 * NOT permuted); perm/iperm [9][B] int32 = the reference's torch.randperm draws in order (a,b,c) x 3 (trainer.py:86-92) and
 * their inverses; params/grads = flat pred.{0,2,4,6,8}.{weight,bias} in state-dict order (r3m_langrew_num_params floats).
 * forward leaves the activations in `workspace`; backward consumes them, writes parameter gradients (= or +=) and ADDS
 * d/d alle into dalle [B,5,D] (may be NULL). scores/dscore are [15][B] in the reference's call order. */
long long r3m_langrew_num_params(int D, int hidden, int lang_dim);
size_t r3m_langrew_workspace_bytes(int B, int D, int hidden, int lang_dim);
int r3m_langrew_forward(const float* alle, const float* feats, const int* perm, const float* params, float* scores, void* workspace,
                        size_t workspace_bytes, int B, int D, int hidden, int lang_dim, r3m_stream_t stream);
int r3m_langrew_backward(const float* dscore, const int* iperm, const float* params, float* grads, float* dalle, void* workspace,
                         size_t workspace_bytes, int B, int D, int hidden, int lang_dim, int accumulate, r3m_stream_t stream);
/* The same pass with the MLP's tensors stored in `dtype` (R3M_DT_F32: identical to the calls above; R3M_DT_BF16: mixed precision
 * in the manner of torch.autocast(bfloat16) around the reference's get_reward calls (r3m/trainer.py:72-92) — input rows, hidden
 * activations and their gradients bf16, every Linear on the bf16 GEMM kernels with fp32 accumulation; master weights, biases,
 * scores, all parameter gradients and dalle stay fp32 — with one difference: a hidden activation is rounded twice (GEMM result
 * to bf16, then bias + ReLU to bf16) where autocast rounds once). Same workspace size; bf16 needs lang_dim % 64 == 0. */
int r3m_langrew_forward_dt(const float* alle, const float* feats, const int* perm, const float* params, float* scores, void* workspace,
                           size_t workspace_bytes, int B, int D, int hidden, int lang_dim, int dtype, r3m_stream_t stream);
int r3m_langrew_backward_dt(const float* dscore, const int* iperm, const float* params, float* grads, float* dalle, void* workspace,
                            size_t workspace_bytes, int B, int D, int hidden, int lang_dim, int accumulate, int dtype, r3m_stream_t stream);
/* The same pass for any number of cross-clip negatives N = the reference's model.num_negatives (r3m/trainer.py:66,86-92), 0 <= N <=
 * R3M_MAX_NEGATIVES: 6 + 3N evaluations, (6 + 3N) B rows. perm / iperm are [3N][B] in the reference's draw order, row 3k + j the k-th
 * draw of head j (may be NULL when N = 0); scores / dscore are [6 + 3N][B]: rows 0-2 the positives (e0,eg) (e0,es1) (e0,es2), rows 3-5
 * the in-clip negatives (e0,e0) (e0,es0) (e0,es1), row q = 6 + 3k + j the k-th permuted negative of head j. Every call above is the
 * N = 3 call of these. The cap of 16 is this library's (54 score rows), the reference has none; N outside 0..16, a row count
 * (6 + 3N) B of 2^31 or more, or a workspace smaller than r3m_langrew_workspace_bytes_n reports return non-zero before any HIP call
 * (workspace_bytes_n returns 0 for what it refuses, with the message set). */
#define R3M_MAX_NEGATIVES 16
size_t r3m_langrew_workspace_bytes_n(int B, int D, int hidden, int lang_dim, int N);
int r3m_langrew_forward_n(const float* alle, const float* feats, const int* perm, const float* params, float* scores, void* workspace,
                          size_t workspace_bytes, int B, int D, int hidden, int lang_dim, int N, int dtype, r3m_stream_t stream);
int r3m_langrew_backward_n(const float* dscore, const int* iperm, const float* params, float* grads, float* dalle, void* workspace,
                           size_t workspace_bytes, int B, int D, int hidden, int lang_dim, int N, int accumulate, int dtype,
                           r3m_stream_t stream);
/* ONE differentiable evaluation score[R] = G(e0[R,D], eg[R,D], le[R,lang_dim]) — the reference's own calling form
 * (R3M.get_reward r3m/models/models_r3m.py:78-81 -> LanguageReward.forward models_language.py:53-55, called 15x with autograd
 * by r3m/trainer.py:72-92). forward leaves the activations in `workspace` (r3m_langrew_call_workspace_bytes(R, ...));
 * backward consumes them, writes parameter gradients (= or +=, flat layout as above) and WRITES the input gradients
 * de0 / deg [R,D] and dle [R,lang_dim] (each may be NULL). */
size_t r3m_langrew_call_workspace_bytes(int R, int D, int hidden, int lang_dim);
int r3m_langrew_call_forward(const float* e0, const float* eg, const float* le, const float* params, float* score, void* workspace,
                             size_t workspace_bytes, int R, int D, int hidden, int lang_dim, r3m_stream_t stream);
int r3m_langrew_call_backward(const float* dscore, const float* params, float* grads, float* de0, float* deg, float* dle,
                              void* workspace, size_t workspace_bytes, int R, int D, int hidden, int lang_dim, int accumulate,
                              r3m_stream_t stream);
/* The same evaluation WITHOUT a backward, for one frame or a handful per call: score[R] = G(e0, eg[R,D], le), fp32, same parameter
 * layout. R0 is the row count of e0 [R0,D] and le [R0,lang_dim]: R0 == R is one row per frame, R0 == 1 broadcasts ONE first frame and
 * ONE instruction to all R rows (inside the concat kernel); any other R0 is refused. Launches on `stream`: concat, ONE memset over the
 * tickets of all four hidden Linears, the four Linears (flags 8 | 16) and the final GEMV. A hidden Linear runs on the few-row kernel
 * (r3m_linear_fwd_small's) where r3m_debug_linear_small_plan says take, else on the launch r3m_langrew_call_forward runs: a pure
 * function of (R, D, hidden, lang_dim). The workspace keeps only what a forward needs: the input rows, two hidden buffers, the tickets
 * and ONE slab area sized for the largest launch. */
size_t r3m_langrew_infer_workspace_bytes(int R, int D, int hidden, int lang_dim);
int r3m_langrew_infer(const float* e0, const float* eg, const float* le, const float* params, float* score, void* workspace,
                      size_t workspace_bytes, int R, int R0, int D, int hidden, int lang_dim, r3m_stream_t stream);

/* ---------------- sentence features: the DistilBERT forward of LangEncoder (r3m/models/models_language.py:13-35) ----------------
 * What the reference reaches through transformers' DistilBertModel under no_grad, then last_hidden_state.mean(1). Inference only,
 * fp32, no dropout. The model is six HOST ints, dims = {vocab, max_pos, dim, n_layers, n_heads, ffn_dim} (distilbert-base-uncased:
 * {30522, 512, 768, 6, 12, 3072}), and one flat fp32 DEVICE parameter buffer of r3m_text_num_params(dims) floats (66 362 880 for
 * distilbert-base). r3m_text_tensor_info enumerates the buffer under HuggingFace's own state-dict names (index <
 * r3m_text_num_tensors): offset and count in floats, ndim 1 or 2, shape2 = {rows, columns} ({n, 1} for a vector). Linear weights
 * stay [out][in]; a layer's q, k and v weights, then their biases, are adjacent, so QKV is one [3 dim, dim] Linear. Every offset is
 * a multiple of 4 floats: a 16-byte-aligned buffer keeps every tensor 16-byte aligned. The queries run without a GPU; num_params /
 * num_tensors return -1 and workspace_bytes returns 0 for dims or shapes they refuse.
 * Supported: dim % 64 == 0, ffn_dim % 64 == 0, head_dim = dim / n_heads a multiple of 32, 1 <= T <= min(max_pos, 128), B >= 1,
 * B * T * max(3 dim, ffn_dim) < 2^31, and T keys and values of one head within a CU's LDS (4 (T (2 head_dim + 4) + 4 head_dim + 4 T)
 * bytes <= 160 KiB: head_dim 64 up to T = 128, head_dim 192 up to T = 102). Anything else returns non-zero before any HIP call.
 * r3m_text_forward: ids, mask int32 [B,T] (mask != 0: a real token); feats [B,dim]; hidden: the last hidden state [B,T,dim], or
 * NULL. pool 0: mean over ALL T positions, padding included (models_language.py:34); pool 1: mean over the positions with
 * mask != 0, the count clamped to at least 1. 2 + 8 n_layers launches on `stream`, no allocation, no synchronisation.
 * Padded query rows are computed like any other row (they attend to the real keys; pool 0 averages them in). An id outside
 * [0, vocab) is CLAMPED into the table by the embedding kernel, so a bad id never reads outside the parameter buffer; callers that
 * want an error validate ids on the host (r3m_amd.text.HipDistilBert does). */
long long r3m_text_num_params(const int* dims);
int r3m_text_num_tensors(const int* dims);
int r3m_text_tensor_info(const int* dims, int index, char* name, int name_cap, long long* offset, long long* count, int* ndim,
                         int* shape2);
size_t r3m_text_workspace_bytes(const int* dims, int B, int T);
int r3m_text_forward(const int* ids, const int* mask, const float* params, float* feats, float* hidden, void* workspace,
                     size_t workspace_bytes, int B, int T, const int* dims, int pool, r3m_stream_t stream);
/* r3m_text_forward for few rows (B * T): the same sequence, the same arguments and refusals, but a Linear that
 * r3m_debug_linear_small_plan takes at B * T rows runs on the few-row kernel (QKV, the output Linear and lin2 with flags 8, lin1 with
 * 8 | 256, so no bias + GELU launch follows it); a Linear the plan leaves makes exactly r3m_text_forward's launches. One memset over
 * all tickets per call. The workspace (r3m_text_small_workspace_bytes) is r3m_text_forward's plus the tickets and one slab area. */
size_t r3m_text_small_workspace_bytes(const int* dims, int B, int T);
int r3m_text_forward_small(const int* ids, const int* mask, const float* params, float* feats, float* hidden, void* workspace,
                           size_t workspace_bytes, int B, int T, const int* dims, int pool, r3m_stream_t stream);
/* The model's own kernels, one by one (all pointers 16-byte aligned, C a multiple of 4).
 * r3m_text_embed: y[b,t,:] = LayerNorm(word[clamp(ids[b,t], 0, vocab - 1)] + pos[t]); word [vocab][C], pos [>= T][C].
 * r3m_layernorm_fwd: y = LayerNorm(x (+ residual, may be NULL)) over the last dimension of [rows][C], biased variance, two passes (a
 *   row of equal values has variance exactly 0); the model uses eps = 1e-12. y may alias x or residual.
 * r3m_bias_gelu: x = gelu(x + bias[column]) in place on [rows][C], the exact erf form (HuggingFace "gelu").
 * r3m_attention_fwd: qkv [B*T][3 dim] (q | k | v, dim = n_heads * head_dim, head h at columns h * head_dim) -> out [B*T][dim] =
 *   softmax(q k^T / sqrt(head_dim), keys with mask == 0 scored as the most negative finite float) v, per sentence and head. A row
 *   whose keys are all masked comes out as the plain average of v, not NaN. One workgroup per (sentence, head), K and V in LDS.
 * r3m_text_pool: feats [B][C] from hidden [B][T][C], pool as above; B <= 65535. */
int r3m_text_embed(const int* ids, const float* word, const float* pos, const float* gamma, const float* beta, float* y, int B, int T,
                   int C, int vocab, float eps, r3m_stream_t stream);
int r3m_layernorm_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* y, long long rows, int C,
                      float eps, r3m_stream_t stream);
int r3m_bias_gelu(float* x, const float* bias, long long rows, int C, r3m_stream_t stream);
int r3m_attention_fwd(const float* qkv, const int* mask, float* out, int B, int T, int n_heads, int head_dim, r3m_stream_t stream);
int r3m_text_pool(const float* hidden, const int* mask, float* feats, int B, int T, int C, int pool, r3m_stream_t stream);

/* ---------------- objective (r3m/trainer.py:39-152, R3M.sim models_r3m.py:102-107) ----------------------------
 * alle [B,5,D] (e0, eg, es0, es1, es2 per clip); perm/iperm [6][B] int32: the reference's torch.randperm draws in
 * order (es0-perm, es2-perm) x 3 (trainer.py:136-137) and their inverses. Writes d(full_loss)/d(alle) to dalle
 * (may be NULL: metrics only). workspace: r3m_loss_workspace_bytes(B).  */
size_t r3m_loss_workspace_bytes(int B);
int r3m_loss_tcn_lp(const float* alle, const int* perm, const int* iperm, float* dalle, void* workspace, size_t workspace_bytes,
                    int B, int D, int l2dist, float l2weight, float l1weight, float tcnweight, r3m_stream_t stream);
/* scores [15][B] of the 15 get_reward calls in reference order (trainer.py:72-92); mask [B] (trainer.py:107-109);
 * dscore [15][B] = d(full_loss)/d(score). Same workspace as r3m_loss_tcn_lp. */
int r3m_loss_lang_infonce(const float* scores, const float* mask, float* dscore, void* workspace, size_t workspace_bytes, int B,
                          float langweight, r3m_stream_t stream);
/* The objective for any number of cross-clip negatives N = model.num_negatives (trainer.py:66,86-92 and :124,135-139), 0 <= N <=
 * R3M_MAX_NEGATIVES (16: this library's cap, the reference has none). The three calls above are the N = 3 calls of these.
 *   TCN: 3 + 2N similarities per clip; perm / iperm [2N][B] int32 in the reference's draw order, row 2k the es0 permutation and row
 *     2k + 1 the es2 permutation of negative k. The sums over negatives run k = 0..N-1 after the fixed terms. N = 0 with tcnweight > 0
 *     is refused: the reference fails there (torch.stack of an empty list, trainer.py:140). N = 0 with tcnweight == 0 computes the
 *     LP terms (perm / iperm are not read).
 *   language InfoNCE: scores / dscore [6 + 3N][B], rows 0-2 positives, 3-5 in-clip negatives, q = 6 + 3k + j the k-th permuted negative
 *     of head j; head j's negatives are summed in-clip first, then k = 0..N-1; rewacc_j compares the positive with the max of all
 *     1 + N. N = 0 is the in-clip negative alone.
 * The workspace grows with N (r3m_loss_workspace_bytes_n; 0 with the message set for a refused B or N); the per-clip partials lead it,
 * so r3m_loss_finalize takes no N and accepts a workspace sized for any N. All refusals come before any HIP call. */
size_t r3m_loss_workspace_bytes_n(int B, int N);
int r3m_loss_tcn_lp_n(const float* alle, const int* perm, const int* iperm, float* dalle, void* workspace, size_t workspace_bytes,
                      int B, int D, int N, int l2dist, float l2weight, float l1weight, float tcnweight, r3m_stream_t stream);
int r3m_loss_lang_infonce_n(const float* scores, const float* mask, float* dscore, void* workspace, size_t workspace_bytes, int B, int N,
                            float langweight, r3m_stream_t stream);
/* metrics[16]: 0 l2loss 1 l1loss 2 l0loss 3 tcnloss 4 aligned 5 rewloss 6-8 rewacc1-3 9 full_loss (trainer.py:55-57,111-117,147-152).
 * Takes the workspace that r3m_loss_tcn_lp[_n] (and r3m_loss_lang_infonce[_n]) filled, whatever N they ran with. It reads the per-clip
 * partials that lead it, 48 B bytes, and refuses a workspace smaller than that; before the `_n` entry points existed it asked for the
 * whole r3m_loss_workspace_bytes(B), which a workspace sized for fewer than 3 negatives does not have. */
int r3m_loss_finalize(void* workspace, size_t workspace_bytes, int B, int have_lang, float* metrics, float l2weight,
                      float l1weight, float tcnweight, float langweight, r3m_stream_t stream);

/* ---------------- optimizer: torch.optim.Adam(params, lr) defaults (models_r3m.py:76; trainer.py:156-158) -------
 * one pass over the flat buffers; step counts from 1; grad_scale multiplies g on the fly (1/world_size for SUM all-reduce).
 * n is a positive multiple of 4: n == 0 is refused on the host like any other bad n (only the ranged forms may have nothing to do) */
int r3m_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, double lr, double beta1,
                  double beta2, double eps, long long step, float grad_scale, r3m_stream_t stream);
/* torch.optim.SGD on the same flat buffers (momentum / dampening / weight_decay / nesterov as torch defines them; momentum_buf may
 * be NULL when momentum == 0; step counts from 1 and selects the buffer initialisation). The reference trains with Adam only
 * (models_r3m.py:76); BASELINE.json's north_star names "the SGD/Adam step". */
int r3m_sgd_step(float* params, const float* grads, float* momentum_buf, long long n, double lr, double momentum, double dampening,
                 double weight_decay, int nesterov, long long step, float grad_scale, r3m_stream_t stream);
/* The same steps over n_ranges disjoint ranges [off[i], off[i] + count[i]) of the flat buffers, sorted by offset, each with its own
 * step count (torch keeps `step` per parameter: a tensor frozen for some steps gets the bias correction of the steps it took).
 * off / count / step are HOST arrays; offsets and counts are multiples of 4. One launch per 64 ranges (the range table travels in the
 * kernel arguments: nothing is allocated or uploaded); n_ranges == 0 launches nothing. Elements inside a range get bit for bit what
 * r3m_adam_step / r3m_sgd_step on that slice with that step gives them; elements outside are not touched. Misaligned, unsorted or
 * overlapping ranges and step < 1 return non-zero before anything is launched. */
int r3m_adam_step_ranges(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const long long* off,
                         const long long* count, const long long* step, int n_ranges, double lr, double beta1, double beta2, double eps,
                         float grad_scale, r3m_stream_t stream);
int r3m_sgd_step_ranges(float* params, const float* grads, float* momentum_buf, const long long* off, const long long* count,
                        const long long* step, int n_ranges, double lr, double momentum, double dampening, double weight_decay,
                        int nesterov, float grad_scale, r3m_stream_t stream);

/* ---------------- parameter groups, weight decay and gradient clipping on the flat buffers ----------------
 * Sum of squares of the fp32 gradients over n_ranges ranges (HOST arrays, checked as above, no step counts), accumulated in fp64:
 * what torch.nn.utils.clip_grad_norm_ squares and adds, without its ~2 launches per tensor. *sqnorm (DEVICE, one double) is
 * written (accumulate == 0) or added to (accumulate != 0): chain calls over several flat buffers for one global norm. Two launches
 * per 64 ranges (one partial per block into `workspace`, then one block adds the partials in a fixed order); no atomics: the same
 * gradients give the same bits on every run and every rank. n_ranges == 0: accumulate ? nothing : *sqnorm = 0. */
size_t r3m_grad_sqnorm_workspace_bytes(void);
int r3m_grad_sqnorm_ranges(const float* grads, const long long* off, const long long* count, int n_ranges, double* sqnorm,
                           int accumulate, void* workspace, size_t workspace_bytes, r3m_stream_t stream);
/* coef_norm (DEVICE, two floats) = { min(1, max_norm / (norm + 1e-6)), norm } with norm = grad_scale * sqrt(*sqnorm), formed in double
 * and rounded once: clip_grad_norm_'s coefficient (its 1e-6 included; error_if_nonfinite=False: a non-finite norm is not treated
 * specially) and the norm before clipping, of the gradients scaled by grad_scale. */
int r3m_clip_coef(const double* sqnorm, double max_norm, float grad_scale, float* coef_norm, r3m_stream_t stream);
/* The ranged steps with a learning rate and a weight decay per range (HOST double arrays, >= 0) and an optional clip coefficient
 * (DEVICE float, coef_norm above; NULL: no multiplication): parameter groups of torch.optim.Adam(weight_decay=) (decoupled == 0:
 * g += wd * p), torch.optim.AdamW (decoupled == 1: p *= (float)(1 - lr * wd) before the update) and torch.optim.SGD, after
 * clip_grad_norm_. Per element g' = (g * grad_scale) * coef, then the decay, then the arithmetic of r3m_adam_step / r3m_sgd_step.
 * One launch per 64 ranges. A range with weight_decay 0 skips the decay operation: with every weight_decay 0, one lr and a NULL
 * coefficient the result is bit for bit that of r3m_adam_step_ranges / r3m_sgd_step_ranges (r3m_sgd_step_groups also with one
 * non-zero weight_decay). A coefficient of exactly 1.0f gives the bits of NULL whenever g * grad_scale is exact (grad_scale a power of
 * two, as 1 / world_size usually is); otherwise the fused g * grad_scale - m of the plain step may differ from it by one rounding.
 * Bad ranges, step < 1, a negative (or NaN) lr or weight_decay return non-zero before anything is launched. */
int r3m_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const long long* off,
                         const long long* count, const long long* step, const double* lr, const double* weight_decay, int n_ranges,
                         double beta1, double beta2, double eps, int decoupled, float grad_scale, const float* clip_coef,
                         r3m_stream_t stream);
int r3m_sgd_step_groups(float* params, const float* grads, float* momentum_buf, const long long* off, const long long* count,
                        const long long* step, const double* lr, const double* weight_decay, int n_ranges, double momentum,
                        double dampening, int nesterov, float grad_scale, const float* clip_coef, r3m_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
