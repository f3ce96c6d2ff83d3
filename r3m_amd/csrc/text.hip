// r3m_amd — DistilBERT forward for LangEncoder's sentence features (reference: r3m/models/models_language.py:13-35, which runs
// HuggingFace's DistilBertModel under no_grad and pools last_hidden_state.mean(1)). Inference only, fp32.
//
// The model is six ints {vocab, max_pos, dim, n_layers, n_heads, ffn_dim} and ONE flat fp32 parameter buffer:
//   embeddings.word_embeddings.weight [vocab][dim]   embeddings.position_embeddings.weight [max_pos][dim]   embeddings.LayerNorm.{weight,bias}
//   per layer l (transformer.layer.l.):  attention.{q,k,v}_lin.weight  attention.{q,k,v}_lin.bias   <- adjacent: QKV is one [3 dim, dim] Linear
//                                        attention.out_lin.{weight,bias}  sa_layer_norm.{weight,bias}
//                                        ffn.lin1.{weight,bias}  ffn.lin2.{weight,bias}  output_layer_norm.{weight,bias}
// Linear weights stay [out][in] (the OHWI layout of a 1x1 convolution). With dim % 64 == 0 every tensor's float count is a multiple
// of 4, so every offset is 16-byte aligned without padding and the buffer holds exactly the model's parameter count.
//
// Launches per call: embed, then per layer  QKV Linear -> attention -> out Linear -> LayerNorm(+residual) -> lin1 -> bias + GELU ->
// lin2 -> LayerNorm(+residual),  then pool: 2 + 8 n_layers. The Linears are the project's gather-GEMM (conv_forward_launch, as
// lang.hip); its epilogues have neither GELU nor a residual, so those live in the kernels below.
#include "engine.h"
#include "../../include/r3m_hip.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace r3m {

static ConvGeom text_linear_geom(int R, int K, int H) { return {R, 1, 1, K, H, 1, 1, 0}; }

constexpr int TEXT_MAX_T = 128;           // the attention kernel keeps at most two scores per lane
constexpr int TEXT_LDS_MAX = 160 * 1024;  // LDS of one CU (gfx950)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// ---- LayerNorm: one wave per row, two passes over the row (mean, then the centred sum of squares: a row of equal values has
// variance exactly 0), a third to store. a (+ b) is re-read from L1 / L2 instead of held: C is not bounded. ----
__device__ __forceinline__ void layernorm_row(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float* __restrict__ y, int C, float eps, int lane) {
  float s = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    f32x4 v = ldg4(a + c);
    if (b) v += ldg4(b + c);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    f32x4 v = ldg4(a + c);
    if (b) v += ldg4(b + c);
    v -= mean;
    q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
  for (int c = lane * 4; c < C; c += 256) {
    f32x4 v = ldg4(a + c);
    if (b) v += ldg4(b + c);
    *reinterpret_cast<f32x4*>(y + c) = (v - mean) * rstd * ldg4(gamma + c) + ldg4(beta + c);
  }
}

__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ y, int rows, int C, float eps) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const long long o = (long long)r * C;
  layernorm_row(x + o, res ? res + o : nullptr, gamma, beta, y + o, C, eps, threadIdx.x & 63);
}

// y[b, t, :] = LayerNorm(word[clamp(ids[b, t])] + pos[t])
__global__ __launch_bounds__(256) void text_embed_kernel(const int* __restrict__ ids, const float* __restrict__ word,
                                                          const float* __restrict__ pos, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ y, int rows, int T, int C,
                                                          int vocab, float eps) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  int id = ids[r];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  layernorm_row(word + (long long)id * C, pos + (long long)(r % T) * C, gamma, beta, y + (long long)r * C, C, eps, threadIdx.x & 63);
}

// x = gelu(x + bias[col]), the exact form 0.5 x (1 + erf(x / sqrt 2))
__global__ __launch_bounds__(256) void bias_gelu_kernel(float* __restrict__ x, const float* __restrict__ bias, long long n4, int C4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4 v = ldg4(x + i * 4) + ldg4(bias + (int)(i % C4) * 4);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = gelu_erf(v[e]);
  *reinterpret_cast<f32x4*>(x + i * 4) = o;
}

// ---- attention: one workgroup per (sentence, head); the head's K and V slices in LDS, one wave per query row ----
// qkv [B*T][3 dim] (q | k | v, head h at columns h * hd), out [B*T][dim]. K rows are padded by one 16-byte slot: a lane reads its
// own key's row with 16-byte reads, and row strides of hd + 4 floats put the 16 lanes of a read group on 16 different slots.
struct AttnLds { int k, v, q, p, floats; };
static inline AttnLds attn_lds(int T, int hd) {
  AttnLds l;
  const int Tp = (T + 3) / 4 * 4;
  l.k = 0;
  l.v = l.k + T * (hd + 4);
  l.q = l.v + T * hd;
  l.p = l.q + 4 * hd;
  l.floats = l.p + 4 * Tp;
  return l;
}

__global__ __launch_bounds__(256) void attention_kernel(const float* __restrict__ qkv, const int* __restrict__ mask,
                                                         float* __restrict__ out, int T, int n_heads, int hd, float scale, AttnLds L) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.x / n_heads, h = blockIdx.x - b * n_heads;
  const int dim = n_heads * hd, hd4 = hd / 4, ks = hd + 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* base = qkv + (long long)b * T * 3 * dim + h * hd;
  float* Ks = lds + L.k;
  float* Vs = lds + L.v;
  float* qs = lds + L.q + wave * hd;
  float* ps = lds + L.p + wave * ((T + 3) / 4 * 4);
  for (int i = threadIdx.x; i < T * hd4; i += 256) {
    const int j = i / hd4, c = (i - j * hd4) * 4;
    const float* row = base + (long long)j * 3 * dim + c;
    *reinterpret_cast<f32x4*>(Ks + j * ks + c) = ldg4(row + dim);
    *reinterpret_cast<f32x4*>(Vs + j * hd + c) = ldg4(row + 2 * dim);
  }
  // this lane's keys: lane and lane + 64 (T <= 128)
  const int j0 = lane, j1 = lane + 64;
  const bool m0 = j0 < T && mask[b * T + j0] != 0, m1 = j1 < T && mask[b * T + j1] != 0;
  const float* k0 = Ks + (j0 < T ? j0 : T - 1) * ks;
  const float* k1 = Ks + (j1 < T ? j1 : T - 1) * ks;
  for (int it = 0; it * 4 < T; ++it) {          // every wave makes the same number of trips: the barriers are uniform
    const int i = it * 4 + wave;                // query row (padded rows included: computed like any other)
    const bool live = i < T;
    __syncthreads();                            // K / V staged (first trip); the previous trip's q and p are no longer read
    if (live)
      for (int c = lane * 4; c < hd; c += 256) *reinterpret_cast<f32x4*>(qs + c) = ldg4(base + (long long)i * 3 * dim + c);
    __syncthreads();
    if (live) {
      float s0 = 0.f, s1 = 0.f;
      for (int c = 0; c < hd; c += 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(qs + c);
        const f32x4 a = *reinterpret_cast<const f32x4*>(k0 + c);
        s0 = fmaf(q[0], a[0], s0); s0 = fmaf(q[1], a[1], s0); s0 = fmaf(q[2], a[2], s0); s0 = fmaf(q[3], a[3], s0);
        if (T > 64) {
          const f32x4 d = *reinterpret_cast<const f32x4*>(k1 + c);
          s1 = fmaf(q[0], d[0], s1); s1 = fmaf(q[1], d[1], s1); s1 = fmaf(q[2], d[2], s1); s1 = fmaf(q[3], d[3], s1);
        }
      }
      // masked keys score the most negative finite float: a row without a real key becomes the uniform average of V, never NaN
      s0 = m0 ? s0 * scale : -FLT_MAX;
      s1 = m1 ? s1 * scale : -FLT_MAX;
      const float mx = wave_max(fmaxf(j0 < T ? s0 : -FLT_MAX, j1 < T ? s1 : -FLT_MAX));
      const float e0 = j0 < T ? expf(s0 - mx) : 0.f, e1 = j1 < T ? expf(s1 - mx) : 0.f;
      const float inv = 1.0f / wave_sum(e0 + e1);
      if (j0 < T) ps[j0] = e0 * inv;
      if (j1 < T) ps[j1] = e1 * inv;
    }
    __syncthreads();
    if (live)
      for (int d = lane; d < hd; d += 64) {
        float acc = 0.f;
        for (int j = 0; j < T; ++j) acc = fmaf(ps[j], Vs[j * hd + d], acc);
        out[((long long)b * T + i) * dim + h * hd + d] = acc;
      }
  }
}

// feats[b, c] = sum_t w_t hidden[b, t, c] / n:  pool 0: w = 1, n = T (padding included, models_language.py:34); pool 1: w = mask != 0, n = max(sum w, 1)
__global__ __launch_bounds__(256) void text_pool_kernel(const float* __restrict__ hidden, const int* __restrict__ mask,
                                                         float* __restrict__ feats, int T, int C, int pool) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  int n = 0;
  for (int t = 0; t < T; ++t) {
    const bool w = pool == 0 || mask[b * T + t] != 0;
    if (w) { s += hidden[((long long)b * T + t) * C + c]; ++n; }
  }
  feats[(long long)b * C + c] = s / (float)(n < 1 ? 1 : n);
}

// ---- launchers: every requirement is checked before the first HIP call ----
static int launch_layernorm(const float* x, const float* res, const float* gamma, const float* beta, float* y, long long rows, int C,
                            float eps, hipStream_t s) {
  R3M_REQUIRE(rows > 0 && rows < (1LL << 31) && C > 0 && C % 4 == 0, "layernorm_fwd: rows=%lld, C=%d (C must be a positive multiple of 4)", rows, C);
  hipLaunchKernelGGL(layernorm_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, s, x, res, gamma, beta, y, (int)rows, C, eps);
  return check_launch("layernorm_fwd");
}

static int launch_text_embed(const int* ids, const float* word, const float* pos, const float* gamma, const float* beta, float* y, int B,
                             int T, int C, int vocab, float eps, hipStream_t s) {
  R3M_REQUIRE(B > 0 && T > 0 && (long long)B * T < (1LL << 31) && C > 0 && C % 4 == 0 && vocab > 0,
              "text_embed: B=%d, T=%d, C=%d (a positive multiple of 4), vocab=%d", B, T, C, vocab);
  hipLaunchKernelGGL(text_embed_kernel, dim3(ceil_div((long long)B * T, 4)), dim3(256), 0, s, ids, word, pos, gamma, beta, y, B * T, T, C,
                     vocab, eps);
  return check_launch("text_embed");
}

int launch_bias_gelu(float* x, const float* bias, long long rows, int C, hipStream_t s) {
  R3M_REQUIRE(rows > 0 && C > 0 && C % 4 == 0 && rows * C / 4 < (1LL << 31) * 256, "bias_gelu: rows=%lld, C=%d (C must be a positive multiple of 4)",
              rows, C);
  const long long n4 = rows * C / 4;
  hipLaunchKernelGGL(bias_gelu_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, s, x, bias, n4, C / 4);
  return check_launch("bias_gelu");
}

static int attention_check(int B, int T, int n_heads, int hd, const char* what) {
  R3M_REQUIRE(B > 0 && n_heads > 0 && (long long)B * n_heads < (1LL << 31), "%s: B=%d sentences, n_heads=%d", what, B, n_heads);
  R3M_REQUIRE(T >= 1 && T <= TEXT_MAX_T, "%s: T=%d tokens (supported: 1 to %d)", what, T, TEXT_MAX_T);
  R3M_REQUIRE(hd > 0 && hd % 32 == 0, "%s: head_dim=%d must be a positive multiple of 32", what, hd);
  R3M_REQUIRE((long long)B * T * 3 * n_heads * hd < (1LL << 31), "%s: B * T * 3 dim = %lld must stay below 2^31", what,
              (long long)B * T * 3 * n_heads * hd);
  const long long bytes = 4LL * ((long long)T * (2 * hd + 4) + 4 * hd + 4 * ((T + 3) / 4 * 4));
  R3M_REQUIRE(bytes <= TEXT_LDS_MAX, "%s: T=%d keys of head_dim=%d need %lld bytes of LDS, a CU has %d", what, T, hd, bytes, TEXT_LDS_MAX);
  return 0;
}

static int launch_attention(const float* qkv, const int* mask, float* out, int B, int T, int n_heads, int hd, hipStream_t s) {
  TRY(attention_check(B, T, n_heads, hd, "attention_fwd"));
  const AttnLds L = attn_lds(T, hd);
  const int bytes = L.floats * 4;
  static DynLdsOptIn optin;
  if (bytes > 64 * 1024) TRY(ensure_dyn_lds(optin, reinterpret_cast<const void*>(attention_kernel), bytes, "attention_fwd"));
  hipLaunchKernelGGL(attention_kernel, dim3(B * n_heads), dim3(256), bytes, s, qkv, mask, out, T, n_heads, hd, 1.0f / sqrtf((float)hd), L);
  return check_launch("attention_fwd");
}

static int launch_text_pool(const float* hidden, const int* mask, float* feats, int B, int T, int C, int pool, hipStream_t s) {
  R3M_REQUIRE(B > 0 && B < 65536 && T > 0 && C > 0 && (long long)B * T < (1LL << 31), "text_pool: B=%d (1 to 65535), T=%d, C=%d", B, T, C);
  R3M_REQUIRE(pool == 0 || pool == 1, "text_pool: pool=%d (0: mean over all positions, 1: mean over mask != 0)", pool);
  hipLaunchKernelGGL(text_pool_kernel, dim3(ceil_div(C, 256), B), dim3(256), 0, s, hidden, mask, feats, T, C, pool);
  return check_launch("text_pool");
}

// ---- the model ----
struct TextDims { int vocab, max_pos, dim, n_layers, n_heads, ffn; };
enum { TEXT_HEAD_TENSORS = 4, TEXT_LAYER_TENSORS = 16 };
struct TextLayer { long long wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b, end; };

static int text_dims(const int* d6, TextDims* d, const char* what) {
  R3M_REQUIRE(d6, "%s: null dims", what);
  *d = {d6[0], d6[1], d6[2], d6[3], d6[4], d6[5]};
  R3M_REQUIRE(d->vocab > 0 && d->max_pos > 0 && d->n_layers > 0 && d->n_heads > 0 && d->dim > 0 && d->ffn > 0,
              "%s: dims {vocab=%d, max_pos=%d, dim=%d, n_layers=%d, n_heads=%d, ffn_dim=%d} must be positive", what, d->vocab, d->max_pos,
              d->dim, d->n_layers, d->n_heads, d->ffn);
  R3M_REQUIRE(d->dim % 64 == 0, "%s: dim=%d must be a multiple of 64", what, d->dim);
  R3M_REQUIRE(d->ffn % 64 == 0, "%s: ffn_dim=%d must be a multiple of 64", what, d->ffn);
  R3M_REQUIRE(d->dim % d->n_heads == 0 && (d->dim / d->n_heads) % 32 == 0, "%s: head_dim = dim / n_heads = %d / %d must be a multiple of 32",
              what, d->dim, d->n_heads);
  return 0;
}

static long long text_head_floats(const TextDims& d) { return ((long long)d.vocab + d.max_pos + 2) * d.dim; }
static TextLayer text_layer(const TextDims& d, int l) {
  const long long D = d.dim, F = d.ffn;
  const long long per = 4 * D * D + 4 * D + 2 * D + 2 * D * F + F + D + 2 * D;
  TextLayer t;
  long long o = text_head_floats(d) + per * l;
  t.wqkv = o; o += 3 * D * D;
  t.bqkv = o; o += 3 * D;
  t.wo = o; o += D * D;
  t.bo = o; o += D;
  t.ln1g = o; o += D;
  t.ln1b = o; o += D;
  t.w1 = o; o += F * D;
  t.b1 = o; o += F;
  t.w2 = o; o += D * F;
  t.b2 = o; o += D;
  t.ln2g = o; o += D;
  t.ln2b = o; o += D;
  t.end = o;
  return t;
}

static int text_tensor(const TextDims& d, int i, char* name, int cap, long long* offset, long long* count, int* ndim, int* shape2) {
  const long long D = d.dim, F = d.ffn;
  long long off, r, c = 0;     // c == 0: a vector of r floats
  char buf[96];
  if (i < TEXT_HEAD_TENSORS) {
    static const char* const names[] = {"embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
                                        "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"};
    snprintf(buf, sizeof buf, "%s", names[i]);
    const long long V = d.vocab, P = d.max_pos;
    switch (i) {
      case 0: off = 0; r = V; c = D; break;
      case 1: off = V * D; r = P; c = D; break;
      case 2: off = (V + P) * D; r = D; break;
      default: off = (V + P + 1) * D; r = D; break;
    }
  } else {
    const int l = (i - TEXT_HEAD_TENSORS) / TEXT_LAYER_TENSORS, k = (i - TEXT_HEAD_TENSORS) % TEXT_LAYER_TENSORS;
    const TextLayer t = text_layer(d, l);
    static const char* const names[] = {"attention.q_lin.weight", "attention.k_lin.weight", "attention.v_lin.weight", "attention.q_lin.bias",
                                        "attention.k_lin.bias", "attention.v_lin.bias", "attention.out_lin.weight", "attention.out_lin.bias",
                                        "sa_layer_norm.weight", "sa_layer_norm.bias", "ffn.lin1.weight", "ffn.lin1.bias", "ffn.lin2.weight",
                                        "ffn.lin2.bias", "output_layer_norm.weight", "output_layer_norm.bias"};
    snprintf(buf, sizeof buf, "transformer.layer.%d.%s", l, names[k]);
    switch (k) {
      case 0: case 1: case 2: off = t.wqkv + k * D * D; r = D; c = D; break;
      case 3: case 4: case 5: off = t.bqkv + (k - 3) * D; r = D; break;
      case 6: off = t.wo; r = D; c = D; break;
      case 7: off = t.bo; r = D; break;
      case 8: off = t.ln1g; r = D; break;
      case 9: off = t.ln1b; r = D; break;
      case 10: off = t.w1; r = F; c = D; break;
      case 11: off = t.b1; r = F; break;
      case 12: off = t.w2; r = D; c = F; break;
      case 13: off = t.b2; r = D; break;
      case 14: off = t.ln2g; r = D; break;
      default: off = t.ln2b; r = D; break;
    }
  }
  if (name && cap > 0) snprintf(name, (size_t)cap, "%s", buf);
  if (offset) *offset = off;
  if (count) *count = c ? r * c : r;
  if (ndim) *ndim = c ? 2 : 1;
  if (shape2) { shape2[0] = (int)r; shape2[1] = (int)(c ? c : 1); }
  return 0;
}

// workspace (floats, every slot a multiple of 16 floats): x, sa, tmp, ctx [B T][dim]; big [B T][max(3 dim, ffn)] = qkv, then the FFN's hidden rows
struct TextWs { long long x, sa, tmp, ctx, big, total; };
static TextWs text_ws(const TextDims& d, long long rows) {
  TextWs w;
  long long o = 0;
  auto take = [&](long long n) { const long long r = o; o = (o + n + 15) / 16 * 16; return r; };
  w.x = take(rows * d.dim);
  w.sa = take(rows * d.dim);
  w.tmp = take(rows * d.dim);
  w.ctx = take(rows * d.dim);
  w.big = take(rows * (3 * d.dim > d.ffn ? 3 * d.dim : d.ffn));
  w.total = o;
  return w;
}

static int text_check_shape(const TextDims& d, int B, int T, const char* what) {
  R3M_REQUIRE(B >= 1, "%s: B=%d sentences", what, B);
  R3M_REQUIRE(T >= 1 && T <= TEXT_MAX_T, "%s: T=%d tokens (supported: 1 to %d)", what, T, TEXT_MAX_T);
  R3M_REQUIRE(T <= d.max_pos, "%s: T=%d tokens, the model has max_pos=%d positions", what, T, d.max_pos);
  const long long widest = 3LL * d.dim > d.ffn ? 3LL * d.dim : d.ffn;
  R3M_REQUIRE((long long)B * T * widest < (1LL << 31), "%s: B * T * max(3 dim, ffn_dim) = %lld must stay below 2^31", what,
              (long long)B * T * widest);
  R3M_REQUIRE(B < 65536, "%s: B=%d sentences (at most 65535)", what, B);
  return attention_check(B, T, d.n_heads, d.dim / d.n_heads, what);
}

// The four Linears of a layer as a SmallLaunchSet (engine.h has the workspace layout), repeated once per layer: the shapes are the same
// in every layer, so is the routing, a pure function of (R, dims). few_rows (r3m_text_forward_small): the rule decides, and the
// set's workspace lies behind the base workspace, from small_off on. Otherwise every entry is the ordinary launch and the set needs no bytes.
enum { TL_QKV = 0, TL_OUT = 1, TL_LIN1 = 2, TL_LIN2 = 3 };
struct TextSmall {
  SmallLaunchSet set;
  size_t small_off, total;   // bytes from the workspace's start
};
static TextSmall text_small(const TextDims& d, long long rows, bool few_rows) {
  TextSmall w;
  const int R = (int)rows, D = d.dim, F = d.ffn;
  const SmallRoute route = few_rows ? SMALL_BY_RULE : SMALL_NEVER;
  w.set.reps = d.n_layers;
  w.set.add(text_linear_geom(R, D, 3 * D), EPI_BIAS, 0, route);              // TL_QKV
  w.set.add(text_linear_geom(R, D, D), EPI_BIAS, 0, route);                  // TL_OUT
  w.set.add(text_linear_geom(R, D, F), EPI_BIAS | EPI_GELU, 0, route);       // TL_LIN1: bias + GELU in the store
  w.set.add(text_linear_geom(R, F, D), EPI_BIAS, 0, route);                  // TL_LIN2
  w.small_off = ((size_t)text_ws(d, rows).total * 4 + 255) / 256 * 256;
  w.total = w.small_off + (w.set.bytes() + 255) / 256 * 256;
  return w;
}

// few_rows == false: the launches of r3m_text_forward, exactly
static int text_forward(const int* ids, const int* mask, const float* P, float* feats, float* hidden, float* ws, int B, int T,
                        const TextDims& d, int pool, bool few_rows, hipStream_t s) {
  const int D = d.dim, R = B * T, hd = D / d.n_heads;
  const float eps = 1e-12f;
  const TextWs w = text_ws(d, R);
  float* x = ws + w.x;
  float* sa = ws + w.sa;
  float* tmp = ws + w.tmp;
  float* ctx = ws + w.ctx;
  float* big = ws + w.big;
  const long long V = d.vocab, MP = d.max_pos;
  const TextSmall sw = text_small(d, R, few_rows);
  char* sws = reinterpret_cast<char*>(ws) + sw.small_off;
  R3M_REQUIRE(!sw.set.reset(sws, s), "text_forward_small: cannot reset the tickets");
  TRY(launch_text_embed(ids, P, P + V * D, P + (V + MP) * D, P + (V + MP + 1) * D, x, B, T, D, d.vocab, eps, s));
  for (int l = 0; l < d.n_layers; ++l) {
    const TextLayer t = text_layer(d, l);
    TRY(sw.set.linear(TL_QKV, l, sws, x, P + t.wqkv, P + t.bqkv, big, s));
    TRY(launch_attention(big, mask, ctx, B, T, d.n_heads, hd, s));
    TRY(sw.set.linear(TL_OUT, l, sws, ctx, P + t.wo, P + t.bo, tmp, s));
    TRY(launch_layernorm(tmp, x, P + t.ln1g, P + t.ln1b, sa, R, D, eps, s));
    TRY(sw.set.linear(TL_LIN1, l, sws, sa, P + t.w1, P + t.b1, big, s));
    TRY(sw.set.linear(TL_LIN2, l, sws, big, P + t.w2, P + t.b2, tmp, s));
    float* y = (l == d.n_layers - 1 && hidden) ? hidden : x;     // the last hidden state goes straight to the caller's buffer
    TRY(launch_layernorm(tmp, sa, P + t.ln2g, P + t.ln2b, y, R, D, eps, s));
    x = y;
  }
  return launch_text_pool(x, mask, feats, B, T, D, pool, s);
}

}  // namespace r3m

using namespace r3m;
static inline hipStream_t S(r3m_stream_t s) { return static_cast<hipStream_t>(s); }

extern "C" {

long long r3m_text_num_params(const int* dims) {
  TextDims d;
  if (text_dims(dims, &d, "text_num_params")) return -1;
  return text_layer(d, d.n_layers - 1).end;
}
int r3m_text_num_tensors(const int* dims) {
  TextDims d;
  if (text_dims(dims, &d, "text_num_tensors")) return -1;
  return TEXT_HEAD_TENSORS + TEXT_LAYER_TENSORS * d.n_layers;
}
int r3m_text_tensor_info(const int* dims, int index, char* name, int name_cap, long long* offset, long long* count, int* ndim, int* shape2) {
  TextDims d;
  TRY(text_dims(dims, &d, "text_tensor_info"));
  R3M_REQUIRE(index >= 0 && index < TEXT_HEAD_TENSORS + TEXT_LAYER_TENSORS * d.n_layers, "text_tensor_info: index %d of %d tensors", index,
              TEXT_HEAD_TENSORS + TEXT_LAYER_TENSORS * d.n_layers);
  return text_tensor(d, index, name, name_cap, offset, count, ndim, shape2);
}
size_t r3m_text_workspace_bytes(const int* dims, int B, int T) {
  TextDims d;
  if (text_dims(dims, &d, "text_workspace_bytes") || text_check_shape(d, B, T, "text_workspace_bytes")) return 0;
  return (size_t)text_ws(d, (long long)B * T).total * 4;
}
static int text_forward_entry(const char* what, bool few_rows, const int* ids, const int* mask, const float* params, float* feats,
                              float* hidden, void* ws, size_t ws_bytes, int B, int T, const int* dims, int pool, r3m_stream_t stream) {
  R3M_REQUIRE(ids && mask && params && feats && ws, "%s: null argument", what);
  TextDims d;
  TRY(text_dims(dims, &d, what));
  TRY(text_check_shape(d, B, T, what));
  R3M_REQUIRE(pool == 0 || pool == 1, "%s: pool=%d (0: mean over all positions, 1: mean over mask != 0)", what, pool);
  const size_t need = few_rows ? text_small(d, (long long)B * T, true).total : (size_t)text_ws(d, (long long)B * T).total * 4;
  R3M_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, need %zu)", what, ws_bytes, need);
  R3M_REQUIRE((reinterpret_cast<uintptr_t>(params) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(feats) & 15) == 0 && (reinterpret_cast<uintptr_t>(hidden) & 15) == 0,
              "%s: params, feats, hidden and workspace must be 16-byte aligned", what);
  return text_forward(ids, mask, params, feats, hidden, static_cast<float*>(ws), B, T, d, pool, few_rows, S(stream));
}
int r3m_text_forward(const int* ids, const int* mask, const float* params, float* feats, float* hidden, void* ws, size_t ws_bytes, int B,
                     int T, const int* dims, int pool, r3m_stream_t stream) {
  return text_forward_entry("text_forward", false, ids, mask, params, feats, hidden, ws, ws_bytes, B, T, dims, pool, stream);
}
size_t r3m_text_small_workspace_bytes(const int* dims, int B, int T) {
  TextDims d;
  if (text_dims(dims, &d, "text_small_workspace_bytes") || text_check_shape(d, B, T, "text_small_workspace_bytes")) return 0;
  return text_small(d, (long long)B * T, true).total;
}
int r3m_text_forward_small(const int* ids, const int* mask, const float* params, float* feats, float* hidden, void* ws, size_t ws_bytes,
                           int B, int T, const int* dims, int pool, r3m_stream_t stream) {
  return text_forward_entry("text_forward_small", true, ids, mask, params, feats, hidden, ws, ws_bytes, B, T, dims, pool, stream);
}

int r3m_text_embed(const int* ids, const float* word, const float* pos, const float* gamma, const float* beta, float* y, int B, int T, int C,
                   int vocab, float eps, r3m_stream_t stream) {
  R3M_REQUIRE(ids && word && pos && gamma && beta && y, "text_embed: null argument");
  return launch_text_embed(ids, word, pos, gamma, beta, y, B, T, C, vocab, eps, S(stream));
}
int r3m_layernorm_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* y, long long rows, int C, float eps,
                      r3m_stream_t stream) {
  R3M_REQUIRE(x && gamma && beta && y, "layernorm_fwd: null argument");
  return launch_layernorm(x, residual, gamma, beta, y, rows, C, eps, S(stream));
}
int r3m_bias_gelu(float* x, const float* bias, long long rows, int C, r3m_stream_t stream) {
  R3M_REQUIRE(x && bias, "bias_gelu: null argument");
  return launch_bias_gelu(x, bias, rows, C, S(stream));
}
int r3m_attention_fwd(const float* qkv, const int* mask, float* out, int B, int T, int n_heads, int head_dim, r3m_stream_t stream) {
  R3M_REQUIRE(qkv && mask && out, "attention_fwd: null argument");
  return launch_attention(qkv, mask, out, B, T, n_heads, head_dim, S(stream));
}
int r3m_text_pool(const float* hidden, const int* mask, float* feats, int B, int T, int C, int pool, r3m_stream_t stream) {
  R3M_REQUIRE(hidden && mask && feats, "text_pool: null argument");
  return launch_text_pool(hidden, mask, feats, B, T, C, pool, S(stream));
}

}  // extern "C"
