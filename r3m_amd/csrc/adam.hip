// r3m_amd — fused Adam step over ONE flat fp32 parameter buffer (all encoder + language-head tensors are views into it),
// replacing the per-tensor python loop of torch.optim.Adam that the reference builds at
// /root/reference/r3m/models/models_r3m.py:76 and steps at /root/reference/r3m/trainer.py:156-158
// (betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad). One HBM pass: read p,g,m,v - write p,m,v.
//
// The *_ranges forms step only some [offset, count) ranges of the buffer, each with its own step count (partial-freeze
// fine-tuning: torch.optim.Adam skips parameters without a gradient and keeps `step` per parameter). Both forms run the same
// element loop (adam_span / sgd_span), so a range gets bit for bit what the whole-buffer kernel gives the same elements.
#include "common.h"
#include <cstring>

namespace r3m {

// f32x4 groups i, i + stride, ... < n4 of the buffers
__device__ __forceinline__ void adam_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                          long long i, long long stride, long long n4, float beta2, float one_minus_beta1,
                                          float one_minus_beta2, float neg_step_size, float bc2_sqrt, float eps, float grad_scale) {
  for (; i < n4; i += stride) {
    f32x4 pp = *reinterpret_cast<f32x4*>(p + i * 4);
    f32x4 gg = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mm = *reinterpret_cast<f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = gg[e] * grad_scale;
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

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long long n4, float beta1, float beta2,
                                                    float one_minus_beta1, float one_minus_beta2, float neg_step_size,
                                                    float bc2_sqrt, float eps, float grad_scale) {
  adam_span(p, g, m, v, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256, n4, beta2, one_minus_beta1, one_minus_beta2,
            neg_step_size, bc2_sqrt, eps, grad_scale);
  (void)beta1;
}

// bias corrections of one step count, formed in double (torch.optim.Adam's python scalars)
static void adam_bias_corrections(double lr, double beta1, double beta2, long long step, float* neg_step, float* bc2s) {
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  *neg_step = (float)(-(lr / bc1));
  *bc2s = (float)sqrt(bc2);
}
static int opt_grid(long long n4) {
  int grid = ceil_div(n4, 256);
  return grid > 256 * 16 ? 256 * 16 : grid;
}

int launch_adam(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2, double eps,
                long long step, float grad_scale, hipStream_t s) {
  R3M_REQUIRE(n % 4 == 0, "adam: n=%lld must be a multiple of 4", n);
  R3M_REQUIRE(step >= 1, "adam: step=%lld must be >= 1", step);
  float neg_step, bc2s;
  adam_bias_corrections(lr, beta1, beta2, step, &neg_step, &bc2s);
  const long long n4 = n / 4;
  hipLaunchKernelGGL(adam_kernel, dim3(opt_grid(n4)), dim3(256), 0, s, p, g, m, v, n4, (float)beta1, (float)beta2, (float)(1.0 - beta1),
                     (float)(1.0 - beta2), neg_step, bc2s, (float)eps, grad_scale);
  return check_launch("adam");
}

// ---- ranged steps ---------------------------------------------------------------------------------------------
// Up to OPT_MAX_RANGES ranges per launch. The table travels BY VALUE in the kernel arguments (no device table, no allocation, no
// upload). Range r owns blocks [first_block[r], first_block[r + 1]); a block finds its range by scanning first_block, which is uniform
// over the block (scalar loads from the argument segment), then runs the whole-buffer loop on that range with its own grid stride.
constexpr int OPT_MAX_RANGES = 64;
struct RangeTable {
  int first_block[OPT_MAX_RANGES + 1];
  int n;
  long long off4[OPT_MAX_RANGES];     // offset / 4
  long long n4[OPT_MAX_RANGES];       // count / 4
  float a[OPT_MAX_RANGES];            // Adam: -lr / bias_correction1 ; SGD: 1.f on the range's first step
  float b[OPT_MAX_RANGES];            // Adam: sqrt(bias_correction2)
};

__device__ __forceinline__ int range_of_block(const RangeTable& t) {
  int r = 0;
  while (r + 1 < t.n && (int)blockIdx.x >= t.first_block[r + 1]) ++r;
  return r;
}

__global__ __launch_bounds__(256) void adam_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const RangeTable t, float beta2, float one_minus_beta1,
                                                           float one_minus_beta2, float eps, float grad_scale) {
  const int r = range_of_block(t);
  const long long o = t.off4[r] * 4;
  const int blocks = t.first_block[r + 1] - t.first_block[r];
  adam_span(p + o, g + o, m + o, v + o, (long long)(blockIdx.x - t.first_block[r]) * 256 + threadIdx.x, (long long)blocks * 256, t.n4[r], beta2,
            one_minus_beta1, one_minus_beta2, t.a[r], t.b[r], eps, grad_scale);
}

// host checks shared by both optimizers; nothing is launched when one fails
static int check_ranges(const char* what, const long long* off, const long long* count, const long long* step, int n_ranges) {
  R3M_REQUIRE(n_ranges >= 0, "%s: n_ranges=%d", what, n_ranges);
  R3M_REQUIRE(n_ranges == 0 || (off && count && step), "%s: null range arrays", what);
  long long end = 0;
  for (int i = 0; i < n_ranges; ++i) {
    R3M_REQUIRE(off[i] >= 0 && count[i] >= 0 && off[i] % 4 == 0 && count[i] % 4 == 0,
                "%s: range %d = [%lld, +%lld): offsets and counts must be non-negative multiples of 4", what, i, off[i], count[i]);
    R3M_REQUIRE(off[i] >= end, "%s: range %d starts at %lld, before the end %lld of the range before it (ranges must be sorted and disjoint)",
                what, i, off[i], end);
    R3M_REQUIRE(step[i] >= 1, "%s: range %d has step=%lld, must be >= 1", what, i, step[i]);
    end = off[i] + count[i];
  }
  return 0;
}
// the next up-to-OPT_MAX_RANGES non-empty ranges from *i on -> t (offsets, counts, block shares); returns the grid
static int fill_ranges(RangeTable& t, const long long* off, const long long* count, int n_ranges, int* i, int* src) {
  memset(&t, 0, sizeof t);
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

int launch_adam_ranges(float* p, const float* g, float* m, float* v, const long long* off, const long long* count, const long long* step,
                       int n_ranges, double lr, double beta1, double beta2, double eps, float grad_scale, hipStream_t s) {
  if (int e = check_ranges("adam_ranges", off, count, step, n_ranges)) return e;
  for (int i = 0; i < n_ranges;) {
    RangeTable t;
    int src[OPT_MAX_RANGES];
    const int grid = fill_ranges(t, off, count, n_ranges, &i, src);
    if (!grid) break;
    for (int r = 0; r < t.n; ++r) adam_bias_corrections(lr, beta1, beta2, step[src[r]], &t.a[r], &t.b[r]);
    hipLaunchKernelGGL(adam_ranges_kernel, dim3(grid), dim3(256), 0, s, p, g, m, v, t, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                       (float)eps, grad_scale);
    if (int e = check_launch("adam_ranges")) return e;
  }
  return 0;
}

// Fused SGD over a flat buffer, torch.optim.SGD semantics (momentum, dampening, weight decay, Nesterov):
//   g' = g*grad_scale + wd*p ; buf = (first step) g' : momentum*buf + (1-dampening)*g' ; d = nesterov ? g' + momentum*buf : buf ; p -= lr*d
// The reference trains with Adam only (models_r3m.py:76); BASELINE.json's north_star names "the SGD/Adam step", so the plain
// optimizer is provided on the same flat-buffer layout (one HBM pass: read p, g, buf - write p, buf).
__device__ __forceinline__ void sgd_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long i,
                                         long long stride, long long n4, float lr, float momentum, float one_minus_damp, float wd,
                                         int nesterov, int first, float grad_scale) {
  for (; i < n4; i += stride) {
    f32x4 pp = *reinterpret_cast<f32x4*>(p + i * 4);
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 bb = {0.f, 0.f, 0.f, 0.f};
    if (buf && !first) bb = *reinterpret_cast<f32x4*>(buf + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float gr = gg[e] * grad_scale;
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

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long n4,
                                                   float lr, float momentum, float one_minus_damp, float wd, int nesterov, int first,
                                                   float grad_scale) {
  sgd_span(p, g, buf, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256, n4, lr, momentum, one_minus_damp, wd, nesterov,
           first, grad_scale);
}

__global__ __launch_bounds__(256) void sgd_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                          const RangeTable t, float lr, float momentum, float one_minus_damp, float wd,
                                                          int nesterov, float grad_scale) {
  const int r = range_of_block(t);
  const long long o = t.off4[r] * 4;
  const int blocks = t.first_block[r + 1] - t.first_block[r];
  sgd_span(p + o, g + o, buf ? buf + o : nullptr, (long long)(blockIdx.x - t.first_block[r]) * 256 + threadIdx.x, (long long)blocks * 256,
           t.n4[r], lr, momentum, one_minus_damp, wd, nesterov, t.a[r] != 0.f, grad_scale);
}

static int check_sgd(double momentum, double dampening, int nesterov, const float* momentum_buf) {
  R3M_REQUIRE(momentum == 0.0 || momentum_buf, "sgd: momentum needs a momentum buffer");
  R3M_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0), "sgd: nesterov needs momentum > 0 and dampening = 0");
  return 0;
}

int launch_sgd(float* p, const float* g, float* momentum_buf, long long n, double lr, double momentum, double dampening,
               double weight_decay, int nesterov, long long step, float grad_scale, hipStream_t s) {
  R3M_REQUIRE(n % 4 == 0, "sgd: n=%lld must be a multiple of 4", n);
  R3M_REQUIRE(step >= 1, "sgd: step=%lld must be >= 1", step);
  if (int e = check_sgd(momentum, dampening, nesterov, momentum_buf)) return e;
  const long long n4 = n / 4;
  hipLaunchKernelGGL(sgd_kernel, dim3(opt_grid(n4)), dim3(256), 0, s, p, g, momentum != 0.0 ? momentum_buf : nullptr, n4, (float)lr,
                     (float)momentum, (float)(1.0 - dampening), (float)weight_decay, nesterov, step == 1 ? 1 : 0, grad_scale);
  return check_launch("sgd");
}

int launch_sgd_ranges(float* p, const float* g, float* momentum_buf, const long long* off, const long long* count, const long long* step,
                      int n_ranges, double lr, double momentum, double dampening, double weight_decay, int nesterov, float grad_scale,
                      hipStream_t s) {
  if (int e = check_ranges("sgd_ranges", off, count, step, n_ranges)) return e;
  if (int e = check_sgd(momentum, dampening, nesterov, momentum_buf)) return e;
  for (int i = 0; i < n_ranges;) {
    RangeTable t;
    int src[OPT_MAX_RANGES];
    const int grid = fill_ranges(t, off, count, n_ranges, &i, src);
    if (!grid) break;
    for (int r = 0; r < t.n; ++r) t.a[r] = step[src[r]] == 1 ? 1.f : 0.f;
    hipLaunchKernelGGL(sgd_ranges_kernel, dim3(grid), dim3(256), 0, s, p, g, momentum != 0.0 ? momentum_buf : nullptr, t, (float)lr,
                       (float)momentum, (float)(1.0 - dampening), (float)weight_decay, nesterov, grad_scale);
    if (int e = check_launch("sgd_ranges")) return e;
  }
  return 0;
}

}  // namespace r3m
