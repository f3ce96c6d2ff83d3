// r3m_amd — fused Adam step over ONE flat fp32 parameter buffer (all encoder + language-head tensors are views into it),
// replacing the per-tensor python loop of torch.optim.Adam that the reference builds at
// /root/reference/r3m/models/models_r3m.py:76 and steps at /root/reference/r3m/trainer.py:156-158
// (betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad). One HBM pass: read p,g,m,v - write p,m,v.
//
// One step kernel and one launcher per optimizer (adam_step_kernel / launch_adam, sgd_step_kernel / launch_sgd) serve all three forms
// of the C API. The kernel steps up to OPT_MAX_RANGES sorted, disjoint [offset, count) ranges of the buffer, each with its own step
// count, learning rate and weight decay (StepTable), and an optional clip coefficient read from device memory:
//   *_step_groups  the general form: parameter groups (AdamW / L2 decay, lr per group) after torch.nn.utils.clip_grad_norm_
//   *_step_ranges  one lr for all ranges, Adam without decay, no coefficient (partial-freeze fine-tuning: torch.optim.Adam skips
//                  parameters without a gradient and keeps `step` per parameter)
//   *_step         the same with the one range [0, n)
// A block picks the element loop of its range (adam_span_t<COEF, DECAY> / sgd_span_t<COEF>), so a range gets bit for bit the same
// result through every form that describes it. One exception to "one kernel", kept for its speed: a call with a single range and
// nothing for a table to say (no coefficient, Adam: no decay) -- the step of every run that freezes nothing -- goes to
// adam_whole_kernel / sgd_whole_kernel, eight lines around the same element loop. sqnorm_* and clip_coef_kernel at the end of this
// file form the clip coefficient as a deterministic fp64 sum over ranges.
#include "common.h"

namespace r3m {

// ---- the range tables ---------------------------------------------------------------------------------------------
// Up to OPT_MAX_RANGES ranges per launch. The table travels BY VALUE in the kernel arguments (no device table, no allocation, no
// upload). Range r owns blocks [first_block[r], first_block[r + 1]); a block finds its range by scanning first_block, which is uniform
// over the block (scalar loads from the argument segment), then runs the element loop on that range with its own grid stride.
constexpr int OPT_MAX_RANGES = 64;
struct RangeTable {                   // where the ranges lie: all that the gradient norm needs
  int first_block[OPT_MAX_RANGES + 1];
  int n;
  long long off4[OPT_MAX_RANGES];     // offset / 4
  long long n4[OPT_MAX_RANGES];       // count / 4
};
struct StepTable {                    // and how each range steps
  RangeTable r;
  float a[OPT_MAX_RANGES];            // Adam: -lr_r / bias_correction1 ; SGD: 1.f on the range's first step
  float b[OPT_MAX_RANGES];            // Adam: sqrt(bias_correction2) ; SGD: lr_r
  float wd[OPT_MAX_RANGES];           // Adam L2 and SGD: weight_decay_r ; AdamW: (float)(1 - lr_r * weight_decay_r), 1.f = no decay
};
static_assert(sizeof(StepTable) == sizeof(RangeTable) + 3 * 256 && sizeof(StepTable) + 64 <= 4096,
              "the range table travels in the kernel arguments (4 KiB)");

__device__ __forceinline__ int range_of_block(const RangeTable& t) {
  int r = 0;
  while (r + 1 < t.n && (int)blockIdx.x >= t.first_block[r + 1]) ++r;
  return r;
}

static int opt_grid(long long n4) {
  int grid = ceil_div(n4, 256);
  return grid > 256 * 16 ? 256 * 16 : grid;
}

// host checks shared by both optimizers and the gradient norm (no step counts there); nothing is launched when one fails
static int check_ranges(const char* what, const long long* off, const long long* count, const long long* step, int n_ranges,
                        bool with_step = true) {
  R3M_REQUIRE(n_ranges >= 0, "%s: n_ranges=%d", what, n_ranges);
  R3M_REQUIRE(n_ranges == 0 || (off && count && (step || !with_step)), "%s: null range arrays", what);
  long long end = 0;
  for (int i = 0; i < n_ranges; ++i) {
    R3M_REQUIRE(off[i] >= 0 && count[i] >= 0 && off[i] % 4 == 0 && count[i] % 4 == 0,
                "%s: range %d = [%lld, +%lld): offsets and counts must be non-negative multiples of 4", what, i, off[i], count[i]);
    R3M_REQUIRE(off[i] >= end, "%s: range %d starts at %lld, before the end %lld of the range before it (ranges must be sorted and disjoint)",
                what, i, off[i], end);
    R3M_REQUIRE(!with_step || step[i] >= 1, "%s: range %d has step=%lld, must be >= 1", what, i, step[i]);
    end = off[i] + count[i];
  }
  return 0;
}
// the same, and the per-range learning rates and weight decays where the call brings them (a NaN fails `>= 0`)
static int check_step_ranges(const char* what, const StepRanges& r) {
  if (int e = check_ranges(what, r.off, r.count, r.step, r.n)) return e;
  for (int i = 0; i < r.n; ++i) {
    R3M_REQUIRE(!r.lrs || r.lrs[i] >= 0.0, "%s: range %d has lr=%g, must be >= 0", what, i, r.lrs[i]);
    R3M_REQUIRE(!r.wds || r.wds[i] >= 0.0, "%s: range %d has weight_decay=%g, must be >= 0", what, i, r.wds[i]);
  }
  return 0;
}
// the next up-to-OPT_MAX_RANGES non-empty ranges from *i on -> t, which comes zeroed (offsets, counts, block shares; src[r]: where
// table entry r came from); returns the grid
static int fill_ranges(RangeTable& t, const long long* off, const long long* count, int n_ranges, int* i, int* src) {
  int blocks = 0;
  for (; *i < n_ranges && t.n < OPT_MAX_RANGES; ++*i) {
    if (count[*i] == 0) continue;
    const int r = t.n++;
    src[r] = *i;
    t.off4[r] = off[*i] / 4;
    t.n4[r] = count[*i] / 4;
    t.first_block[r] = blocks;
    blocks += opt_grid(t.n4[r]);
  }
  for (int r = t.n; r <= OPT_MAX_RANGES; ++r) t.first_block[r] = blocks;
  return blocks;
}

// ---- Adam ---------------------------------------------------------------------------------------------------------
// f32x4 groups i, i + stride, ... < n4 of the buffers.
// COEF: the gradient is also multiplied by `coef` (gradient clipping). DECAY 1: gr += wd * p (torch.optim.Adam(weight_decay=)),
// DECAY 2: p *= wd, wd = (float)(1 - lr * weight_decay) (AdamW), before the update. <false, 0> is the plain step.
template <bool COEF, int DECAY>
__device__ __forceinline__ void adam_span_t(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            long long i, long long stride, long long n4, float beta2, float one_minus_beta1,
                                            float one_minus_beta2, float neg_step_size, float bc2_sqrt, float eps, float grad_scale,
                                            float coef, float wd) {
  for (; i < n4; i += stride) {
    f32x4 pp = *reinterpret_cast<f32x4*>(p + i * 4);
    f32x4 gg = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mm = *reinterpret_cast<f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float gr = gg[e] * grad_scale;
      if (COEF) gr = gr * coef;
      if (DECAY == 1) gr = gr + wd * pp[e];
      if (DECAY == 2) pp[e] = pp[e] * wd;
      // exp_avg.lerp_(grad, 1-beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
      mm[e] = mm[e] + (gr - mm[e]) * one_minus_beta1;
      vv[e] = vv[e] * beta2 + (one_minus_beta2 * gr) * gr;
      // denom = sqrt(v)/sqrt(bias_correction2) + eps ; p.addcdiv_(m, denom, value=-lr/bias_correction1)
      const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
      pp[e] = pp[e] + (neg_step_size * mm[e]) / denom;
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = pp;
    *reinterpret_cast<f32x4*>(m + i * 4) = mm;
    *reinterpret_cast<f32x4*>(v + i * 4) = vv;
  }
}

template <bool COEF>
__device__ __forceinline__ void adam_step_block(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, const StepTable& t, float beta2, float one_minus_beta1,
                                                float one_minus_beta2, float eps, float grad_scale, float coef, int decoupled) {
  const int r = range_of_block(t.r);
  const long long o = t.r.off4[r] * 4;
  const int blocks = t.r.first_block[r + 1] - t.r.first_block[r];
  const long long i = (long long)(blockIdx.x - t.r.first_block[r]) * 256 + threadIdx.x, stride = (long long)blocks * 256;
  const float wd = t.wd[r];
  if (decoupled ? wd == 1.f : wd == 0.f)
    adam_span_t<COEF, 0>(p + o, g + o, m + o, v + o, i, stride, t.r.n4[r], beta2, one_minus_beta1, one_minus_beta2, t.a[r], t.b[r], eps,
                         grad_scale, coef, 0.f);
  else if (decoupled)
    adam_span_t<COEF, 2>(p + o, g + o, m + o, v + o, i, stride, t.r.n4[r], beta2, one_minus_beta1, one_minus_beta2, t.a[r], t.b[r], eps,
                         grad_scale, coef, wd);
  else
    adam_span_t<COEF, 1>(p + o, g + o, m + o, v + o, i, stride, t.r.n4[r], beta2, one_minus_beta1, one_minus_beta2, t.a[r], t.b[r], eps,
                         grad_scale, coef, wd);
}

__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, const StepTable t, float beta2, float one_minus_beta1,
                                                         float one_minus_beta2, float eps, float grad_scale,
                                                         const float* __restrict__ coef, int decoupled) {
  if (coef)       // the same address for every lane: one scalar load
    adam_step_block<true>(p, g, m, v, t, beta2, one_minus_beta1, one_minus_beta2, eps, grad_scale, *coef, decoupled);
  else
    adam_step_block<false>(p, g, m, v, t, beta2, one_minus_beta1, one_minus_beta2, eps, grad_scale, 0.f, decoupled);
}

// One range without decay or coefficient, the step of every run that freezes nothing: the table has nothing to say, and the plain
// grid-stride launch spares each block the look-up (2 % on ResNet-50's buffer: profiles/optim_groups.txt). The same element loop.
__global__ __launch_bounds__(256) void adam_whole_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long long n4, float beta2, float one_minus_beta1,
                                                          float one_minus_beta2, float neg_step_size, float bc2_sqrt, float eps,
                                                          float grad_scale) {
  adam_span_t<false, 0>(p, g, m, v, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256, n4, beta2, one_minus_beta1,
                        one_minus_beta2, neg_step_size, bc2_sqrt, eps, grad_scale, 0.f, 0.f);
}

// bias corrections of one step count, formed in double (torch.optim.Adam's python scalars)
static void adam_bias_corrections(double lr, double beta1, double beta2, long long step, float* neg_step, float* bc2s) {
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  *neg_step = (float)(-(lr / bc1));
  *bc2s = (float)sqrt(bc2);
}

int launch_adam(const char* what, float* p, const float* g, float* m, float* v, const StepRanges& r, double beta1, double beta2, double eps,
                int decoupled, float grad_scale, const float* clip_coef, hipStream_t s) {
  if (int e = check_step_ranges(what, r)) return e;
  if (r.n == 1 && r.count[0] > 0 && !clip_coef && (r.wds ? r.wds[0] : r.wd) == 0.0) {
    const long long o = r.off[0], n4 = r.count[0] / 4;
    float neg_step, bc2s;
    adam_bias_corrections(r.lrs ? r.lrs[0] : r.lr, beta1, beta2, r.step[0], &neg_step, &bc2s);
    hipLaunchKernelGGL(adam_whole_kernel, dim3(opt_grid(n4)), dim3(256), 0, s, p + o, g + o, m + o, v + o, n4, (float)beta2,
                       (float)(1.0 - beta1), (float)(1.0 - beta2), neg_step, bc2s, (float)eps, grad_scale);
    return check_launch(what);
  }
  for (int i = 0; i < r.n;) {
    StepTable t = {};
    int src[OPT_MAX_RANGES];
    const int grid = fill_ranges(t.r, r.off, r.count, r.n, &i, src);
    if (!grid) break;
    for (int k = 0; k < t.r.n; ++k) {
      const double lr = r.lrs ? r.lrs[src[k]] : r.lr, wd = r.wds ? r.wds[src[k]] : r.wd;
      adam_bias_corrections(lr, beta1, beta2, r.step[src[k]], &t.a[k], &t.b[k]);
      // AdamW: param.mul_(1 - lr * weight_decay), the factor a python (double) scalar
      t.wd[k] = decoupled ? (wd == 0.0 ? 1.f : (float)(1.0 - lr * wd)) : (float)wd;
    }
    hipLaunchKernelGGL(adam_step_kernel, dim3(grid), dim3(256), 0, s, p, g, m, v, t, (float)beta2, (float)(1.0 - beta1),
                       (float)(1.0 - beta2), (float)eps, grad_scale, clip_coef, decoupled ? 1 : 0);
    if (int e = check_launch(what)) return e;
  }
  return 0;
}

// ---- SGD ----------------------------------------------------------------------------------------------------------
// Fused SGD over a flat buffer, torch.optim.SGD semantics (momentum, dampening, weight decay, Nesterov):
//   g' = g*grad_scale + wd*p ; buf = (first step) g' : momentum*buf + (1-dampening)*g' ; d = nesterov ? g' + momentum*buf : buf ; p -= lr*d
// The reference trains with Adam only (models_r3m.py:76); BASELINE.json's north_star names "the SGD/Adam step", so the plain
// optimizer is provided on the same flat-buffer layout (one HBM pass: read p, g, buf - write p, buf).
// COEF: the gradient is also multiplied by `coef` (gradient clipping); <false> is the plain step.
template <bool COEF>
__device__ __forceinline__ void sgd_span_t(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long i,
                                           long long stride, long long n4, float lr, float momentum, float one_minus_damp, float wd,
                                           int nesterov, int first, float grad_scale, float coef) {
  for (; i < n4; i += stride) {
    f32x4 pp = *reinterpret_cast<f32x4*>(p + i * 4);
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 bb = {0.f, 0.f, 0.f, 0.f};
    if (buf && !first) bb = *reinterpret_cast<f32x4*>(buf + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float gr = gg[e] * grad_scale;
      if (COEF) gr = gr * coef;
      if (wd != 0.f) gr = gr + wd * pp[e];
      float d = gr;
      if (buf) {
        bb[e] = first ? gr : bb[e] * momentum + one_minus_damp * gr;
        d = nesterov ? gr + momentum * bb[e] : bb[e];
      }
      pp[e] = pp[e] - lr * d;
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = pp;
    if (buf) *reinterpret_cast<f32x4*>(buf + i * 4) = bb;
  }
}

__global__ __launch_bounds__(256) void sgd_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                        const StepTable t, float momentum, float one_minus_damp, int nesterov,
                                                        float grad_scale, const float* __restrict__ coef) {
  const int r = range_of_block(t.r);
  const long long o = t.r.off4[r] * 4;
  const int blocks = t.r.first_block[r + 1] - t.r.first_block[r];
  const long long i = (long long)(blockIdx.x - t.r.first_block[r]) * 256 + threadIdx.x, stride = (long long)blocks * 256;
  float* b = buf ? buf + o : nullptr;
  if (coef)
    sgd_span_t<true>(p + o, g + o, b, i, stride, t.r.n4[r], t.b[r], momentum, one_minus_damp, t.wd[r], nesterov, t.a[r] != 0.f, grad_scale,
                     *coef);
  else
    sgd_span_t<false>(p + o, g + o, b, i, stride, t.r.n4[r], t.b[r], momentum, one_minus_damp, t.wd[r], nesterov, t.a[r] != 0.f, grad_scale,
                      0.f);
}

// one range without coefficient: as adam_whole_kernel
__global__ __launch_bounds__(256) void sgd_whole_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                         long long n4, float lr, float momentum, float one_minus_damp, float wd,
                                                         int nesterov, int first, float grad_scale) {
  sgd_span_t<false>(p, g, buf, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256, n4, lr, momentum, one_minus_damp, wd,
                    nesterov, first, grad_scale, 0.f);
}

int launch_sgd(const char* what, float* p, const float* g, float* momentum_buf, const StepRanges& r, double momentum, double dampening,
               int nesterov, float grad_scale, const float* clip_coef, hipStream_t s) {
  if (int e = check_step_ranges(what, r)) return e;
  R3M_REQUIRE(momentum == 0.0 || momentum_buf, "sgd: momentum needs a momentum buffer");
  R3M_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0), "sgd: nesterov needs momentum > 0 and dampening = 0");
  float* buf = momentum != 0.0 ? momentum_buf : nullptr;
  if (r.n == 1 && r.count[0] > 0 && !clip_coef) {
    const long long o = r.off[0], n4 = r.count[0] / 4;
    hipLaunchKernelGGL(sgd_whole_kernel, dim3(opt_grid(n4)), dim3(256), 0, s, p + o, g + o, buf ? buf + o : nullptr, n4,
                       (float)(r.lrs ? r.lrs[0] : r.lr), (float)momentum, (float)(1.0 - dampening), (float)(r.wds ? r.wds[0] : r.wd), nesterov,
                       r.step[0] == 1 ? 1 : 0, grad_scale);
    return check_launch(what);
  }
  for (int i = 0; i < r.n;) {
    StepTable t = {};
    int src[OPT_MAX_RANGES];
    const int grid = fill_ranges(t.r, r.off, r.count, r.n, &i, src);
    if (!grid) break;
    for (int k = 0; k < t.r.n; ++k) {
      t.a[k] = r.step[src[k]] == 1 ? 1.f : 0.f;
      t.b[k] = (float)(r.lrs ? r.lrs[src[k]] : r.lr);
      t.wd[k] = (float)(r.wds ? r.wds[src[k]] : r.wd);
    }
    hipLaunchKernelGGL(sgd_step_kernel, dim3(grid), dim3(256), 0, s, p, g, buf, t, (float)momentum,
                       (float)(1.0 - dampening), nesterov, grad_scale, clip_coef);
    if (int e = check_launch(what)) return e;
  }
  return 0;
}

// ---- squared gradient norm over ranges (torch.nn.utils.clip_grad_norm_'s norm, without its ~2 launches per tensor) --------------
// Deterministic fp64: blocks map to ranges as in the steps; a lane squares and adds its elements in double, in index order; the 64
// lanes of a wave combine by a fixed shuffle tree, the 4 waves of the block in wave order; one partial per block. A second,
// single-block kernel adds the partials (lane l: l, l + 256, ... in index order, then the same block combine) and writes the total
// to *out or adds it to *out: a plain load, add and store by lane 0. No atomics: the same input gives the same bits every time.
constexpr int SQNORM_MAX_BLOCKS = OPT_MAX_RANGES * 256 * 16;      // opt_grid's cap per range

__device__ __forceinline__ double block_sum_256(double x, double* wave_sums) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];      // every lane; lane 0 stores
}

__global__ __launch_bounds__(256) void sqnorm_ranges_kernel(const float* __restrict__ g, const RangeTable t, double* __restrict__ partial) {
  __shared__ double wave_sums[4];
  const int r = range_of_block(t);
  const float* gr = g + t.off4[r] * 4;
  const int blocks = t.first_block[r + 1] - t.first_block[r];
  const long long stride = (long long)blocks * 256, n4 = t.n4[r];
  double acc = 0.0;
  for (long long i = (long long)(blockIdx.x - t.first_block[r]) * 256 + threadIdx.x; i < n4; i += stride) {
    const f32x4 gg = *reinterpret_cast<const f32x4*>(gr + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double x = (double)gg[e];
      acc = acc + x * x;
    }
  }
  const double sum = block_sum_256(acc, wave_sums);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void sqnorm_finish_kernel(const double* __restrict__ partial, int n, double* __restrict__ out,
                                                             int accumulate) {
  __shared__ double wave_sums[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc = acc + partial[i];
  const double sum = block_sum_256(acc, wave_sums);
  if (threadIdx.x == 0) *out = accumulate ? *out + sum : sum;
}

size_t grad_sqnorm_workspace_bytes() { return (size_t)SQNORM_MAX_BLOCKS * sizeof(double); }

int launch_grad_sqnorm_ranges(const float* g, const long long* off, const long long* count, int n_ranges, double* sqnorm, int accumulate,
                              double* ws, hipStream_t s) {
  if (int e = check_ranges("grad_sqnorm_ranges", off, count, nullptr, n_ranges, false)) return e;
  bool launched = false;
  for (int i = 0; i < n_ranges;) {
    RangeTable t = {};
    int src[OPT_MAX_RANGES];
    const int grid = fill_ranges(t, off, count, n_ranges, &i, src);
    if (!grid) break;
    hipLaunchKernelGGL(sqnorm_ranges_kernel, dim3(grid), dim3(256), 0, s, g, t, ws);
    if (int e = check_launch("grad_sqnorm_ranges")) return e;
    hipLaunchKernelGGL(sqnorm_finish_kernel, dim3(1), dim3(256), 0, s, ws, grid, sqnorm, (accumulate || launched) ? 1 : 0);
    if (int e = check_launch("grad_sqnorm_finish")) return e;
    launched = true;
  }
  if (!launched && !accumulate) {      // nothing to add up: the norm of no gradient is 0
    hipLaunchKernelGGL(sqnorm_finish_kernel, dim3(1), dim3(256), 0, s, ws, 0, sqnorm, 0);
    return check_launch("grad_sqnorm_finish");
  }
  return 0;
}

// torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): clip_coef = clamp(max_norm / (total_norm + 1e-6), max=1.0). In double, each
// result rounded once to float; a non-finite norm takes the same course as in torch (inf -> 0, nan -> nan).
__global__ void clip_coef_kernel(const double* __restrict__ sqnorm, double max_norm, float grad_scale, float* __restrict__ coef_norm) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double norm = (double)grad_scale * sqrt(*sqnorm);
  double c = max_norm / (norm + 1e-6);
  if (c > 1.0) c = 1.0;
  coef_norm[0] = (float)c;
  coef_norm[1] = (float)norm;
}

int launch_clip_coef(const double* sqnorm, double max_norm, float grad_scale, float* coef_norm, hipStream_t s) {
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, s, sqnorm, max_norm, grad_scale, coef_norm);
  return check_launch("clip_coef");
}

}  // namespace r3m
