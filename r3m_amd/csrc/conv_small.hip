// r3m_amd — forward convolution for SMALL row counts (one image or a handful of frames per call): a split-K gather-GEMM on the exact-fp32
// MFMA (v_mfma_f32_16x16x4_f32) with 16-, 32- or 64-row tiles and an in-launch, deterministic, wait-free reduction.
//
// Operands as the other forward kernels: NHWC fp32 input, OHWI fp32 weights (both K-contiguous), k in {1, 3}, stride in {1, 2}; the
// three inference stores EPI_AFFINE [| EPI_RELU] [| EPI_ACCUM | EPI_RELU]. Why another kernel: the 128 x 128 / 256 x 64 tiles of conv.hip /
// conv_pw.hip were sized for thousands of row tiles. At one frame a layer4 launch is 49 rows: a handful of blocks on a 256-CU part,
// each walking the whole K with most of its rows empty. Here
//   * a block is 4 waves over BM x 64 outputs, BM = 16 * MT (MT = 1, 2, 4): wave w owns columns 16 w .. 16 w + 15 and all BM rows;
//   * K (taps x Ci / 32 chunks of 32) is cut into S slices, one block per (row tile, column tile, slice), S chosen so that the grid is
//     about 1/2 - 1 x the CU count (small_conv_plan below; a slice boundary may fall inside a tap);
//   * nothing goes through LDS: a weight element is used by one wave only and the few input rows are L2-resident, so each lane loads
//     its fragments straight to registers (16 B per load, two loads per operand and chunk) one chunk ahead of the MFMAs. Lane l holds
//     k = 16 h + 4 (l >> 4) + j of chunk half h in element j for BOTH operands, so step (h, j) of the MFMA chain multiplies like k;
//   * S > 1: every block writes its accumulators as one fp32 slab (16 B per lane and row group, fragment order), the block performs ONE
//     agent-scope release and draws a ticket from its tile's counter; the block that draws S - 1 performs ONE agent-scope acquire, sums
//     the S slabs IN SLICE ORDER (its own included, read back like the others), applies scale / shift, the residual and the ReLU and
//     stores. No block waits for another one: no spinning, no grid barrier, no floating-point atomics — the same operands give the same
//     bits on every launch whichever block arrives last. S = 1 stores from the accumulators and touches neither counter nor slab.
// Tickets and slabs live in the caller's workspace, laid out by ONE type for every caller: SmallLaunchSet (declared in engine.h with
// the layout rule, defined below) lists a call's launches, gives each its own ticket block, zeroes all of them with one
// hipMemsetAsync ahead of the first launch and shares one slab area between them. The encoder's prepared forward (engine.hip), the
// reward head (lang.hip), the text model (text.hip) and the single-launch C entries at the end of this file all go through it.
//
// A Linear over few rows is the same launch: the 1 x 1 geometry (M, 1, 1, K, N, 1, 1, 0) makes the main loop y[M, N] = x[M, K] w[N, K]^T.
// Only the store differs, so the store is a template parameter (SmallStore): the convolution instantiations keep the affine store
// above, the Linear ones store acc + bias[col] with an optional ReLU (EPI_BIAS [| EPI_RELU]: the reward head) or through the exact GELU
// (EPI_BIAS | EPI_GELU: the text model's lin1). Main loop, slabs, tickets and the slice-order sum are one body for all of them.
#include "engine.h"
#include "../../include/r3m_hip.h"
#include <algorithm>
#include <cstring>

namespace r3m {

struct SmallConvParams {
  const float* x;
  const float* w;
  float* out;
  const float* scale;    // affine store only
  const float* shift;    // the affine store's shift; the bias of the Linear stores
  float* slabs;          // [tiles][S][MT][256] f32x4 (S > 1)
  unsigned* ctr;         // [tiles] tickets, zero before the launch (S > 1)
  int Hi, Wi, Ci, Co, Ho, Wo, M;
  int k, stride, pad, flags;
  int tiles_n;           // Co / 64
  int S, cps, nch, cpt;  // slices, chunks per slice, chunks in all (taps * Ci / 32), chunks per tap (Ci / 32)
};

template <int MT>
struct SmallFrag {
  f32x4 a[MT][2];
  f32x4 b[2];
};

enum SmallStore : int { ST_AFFINE = 0, ST_BIAS = 1, ST_BIAS_GELU = 2 };

template <int MT, int ST>
__global__ __launch_bounds__(256) void conv_small_kernel(const SmallConvParams p) {
  __shared__ int s_ticket;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int slice = blockIdx.x % p.S, tile = blockIdx.x / p.S;
  const int tn = tile % p.tiles_n, tm = tile / p.tiles_n;
  const int col = tn * 64 + wave * 16 + r;               // < Co: Co is a multiple of 64
  const int T = p.k * p.k;

  // the MT input rows this lane feeds (A operand): their pixel origin, or "no row"
  int iy0[MT], ix0[MT];
  long long img[MT];
  bool rowok[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int row = (tm * MT + m) * 16 + r;
    rowok[m] = row < p.M;
    const int rr = rowok[m] ? row : 0;
    const int n = rr / (p.Ho * p.Wo), rem = rr - n * (p.Ho * p.Wo);
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    iy0[m] = oy * p.stride - p.pad;
    ix0[m] = ox * p.stride - p.pad;
    img[m] = (long long)n * p.Hi * p.Wi;
  }
  const float* wcol = p.w + (long long)col * T * p.Ci + q * 4;

  const int c0 = slice * p.cps, c1 = min(c0 + p.cps, p.nch);
  int tap = c0 / p.cpt, kc = c0 - tap * p.cpt;            // chunk c = (tap, kc): advanced by next()
  auto load = [&](SmallFrag<MT>& f) {
    const int kh = tap / p.k, kw = tap - kh * p.k;
    const int koff = kc * 32 + q * 4;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int iy = iy0[m] + kh, ix = ix0[m] + kw;
      const bool ok = rowok[m] && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
      // a padding tap or a row past M loads from the tensor's first pixel and is zeroed afterwards: no branch around the loads
      const float* src = p.x + (ok ? (img[m] + (long long)iy * p.Wi + ix) * p.Ci : 0LL) + koff;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 16);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      f.a[m][0] = ok ? v0 : z;
      f.a[m][1] = ok ? v1 : z;
    }
    const float* wsrc = wcol + (long long)tap * p.Ci + kc * 32;
    f.b[0] = *reinterpret_cast<const f32x4*>(wsrc);
    f.b[1] = *reinterpret_cast<const f32x4*>(wsrc + 16);
  };
  auto next = [&]() { if (++kc == p.cpt) { kc = 0; ++tap; } };

  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c0 < c1) {
    SmallFrag<MT> cur, nxt;
    load(cur);
    for (int c = c0; c < c1; ++c) {
      next();
      const bool more = c + 1 < c1;                        // block-uniform
      if (more) load(nxt);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[m][h][j], cur.b[h][j], acc[m], 0, 0, 0);
      if (more) cur = nxt;
    }
  }

  if (p.S > 1) {
    f32x4* slab = reinterpret_cast<f32x4*>(p.slabs);
    const long long base = ((long long)tile * p.S) * (MT * 256) + tid;
#pragma unroll
    for (int m = 0; m < MT; ++m) slab[base + ((long long)slice * MT + m) * 256] = acc[m];
    // publish: every wave drains its stores, the block meets, ONE lane releases at agent scope, waits once more, then draws the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      s_ticket = (int)__hip_atomic_fetch_add(p.ctr + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s_ticket != p.S - 1) return;                       // not the last slice of this tile to arrive: done, nobody waits
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = 0; s < p.S; ++s)                          // slice order, whoever arrived last
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m] += slab[base + ((long long)s * MT + m) * 256];
  }

  // store: lane holds column `col` of rows 4 q + i of each 16-row group
  if constexpr (ST == ST_AFFINE) {
    const float sc = p.scale[col], sh = p.shift[col];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (tm * MT + m) * 16 + q * 4 + i;
        if (row >= p.M) continue;
        float* o = p.out + (long long)row * p.Co + col;
        float v = fmaf(acc[m][i], sc, sh);
        if (p.flags & EPI_ACCUM) v += *o;
        if (p.flags & EPI_RELU) v = fmaxf(v, 0.f);
        *o = v;
      }
  } else {
    const float b = p.shift[col];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (tm * MT + m) * 16 + q * 4 + i;
        if (row >= p.M) continue;
        float v = acc[m][i] + b;
        if constexpr (ST == ST_BIAS_GELU) v = gelu_erf(v);
        else if (p.flags & EPI_RELU) v = fmaxf(v, 0.f);
        p.out[(long long)row * p.Co + col] = v;
      }
  }
}

// ---- host: the plan (pure), the sizes, the launcher ----
bool small_linear_flags(int flags) { return flags == EPI_BIAS || flags == (EPI_BIAS | EPI_RELU) || flags == (EPI_BIAS | EPI_GELU); }

const char* small_conv_refuses(const ConvGeom& c, int flags) {
  if (c.N < 1 || c.Hi < 1 || c.Wi < 1) return "empty input";
  if (c.k != 1 && c.k != 3) return "k must be 1 or 3";
  if (c.stride != 1 && c.stride != 2) return "stride must be 1 or 2";
  if (c.pad != (c.k == 3 ? 1 : 0)) return "pad must be 1 (k = 3) or 0 (k = 1)";
  if (c.Ci < 32 || (c.Ci & 31)) return "Ci must be a multiple of 32";
  if (c.Co < 64 || (c.Co & 63)) return "Co must be a multiple of 64";
  if (c.Ho() < 1 || c.Wo() < 1) return "empty output";
  if ((long long)c.N * c.Ho() * c.Wo() > SMALL_CONV_ROWS_MAX) return "more rows than the kernel is built for";
  if (flags != EPI_AFFINE && flags != (EPI_AFFINE | EPI_RELU) && flags != (EPI_AFFINE | EPI_ACCUM | EPI_RELU) && !small_linear_flags(flags))
    return "epilogue flags must be 128, 128|16 or 128|2|16 (convolution) or 8, 8|16 or 8|256 (Linear)";
  return nullptr;
}

int small_conv_max_split(const ConvGeom& c) { return std::min(SMALL_CONV_SPLIT_MAX, c.k * c.k * (c.Ci / 32)); }

SmallConvPlan small_conv_plan(const ConvGeom& c, int flags, int split) {
  SmallConvPlan r;
  memset(&r, 0, sizeof r);
  if (small_conv_refuses(c, flags)) return r;
  const int M = c.M();
  r.bm = M <= 16 ? 16 : M <= 32 ? 32 : 64;
  r.bn = 64;
  r.tiles_m = ceil_div(M, r.bm);
  r.tiles_n = c.Co / 64;
  r.nch = c.k * c.k * (c.Ci / 32);
  const int tiles = r.tiles_m * r.tiles_n;
  int S = split;
  if (S <= 0) {
    // decomposition first: blocks = tiles * S about 1/2 - 1 x the 256 CUs, a slice no shorter than 4 chunks (128 k)
    S = std::max(1, std::min(std::min(256 / tiles, r.nch / 4), SMALL_CONV_SPLIT_MAX));
    r.cps = ceil_div(r.nch, S);
    S = ceil_div(r.nch, r.cps);                       // no empty slice
  } else {
    r.cps = ceil_div(r.nch, S);                       // forced (tests): trailing slices may be empty, they contribute zero slabs
  }
  r.S = S;
  r.grid = tiles * S;
  // the routing rule, from the per-launch A/B in profiles/small_batch_latency.txt: while the tiles fit the CUs in one round this
  // kernel's time is one block's latency over a K slice, and the kernels of conv.hip / conv_pw.hip pay for the whole K in a few
  // 128-row tiles (ratios 1.1 - 10); from about 400 blocks on they win (0.45 - 0.93)
  r.take = tiles <= SMALL_CONV_TAKE_TILES && r.nch >= SMALL_CONV_TAKE_CHUNKS ? 1 : 0;
  return r;
}

template <int ST>
static void launch_small_tile(const SmallConvParams& p, const SmallConvPlan& r, hipStream_t s) {
  switch (r.bm) {
    case 16: hipLaunchKernelGGL((conv_small_kernel<1, ST>), dim3(r.grid), dim3(256), 0, s, p); break;
    case 32: hipLaunchKernelGGL((conv_small_kernel<2, ST>), dim3(r.grid), dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL((conv_small_kernel<4, ST>), dim3(r.grid), dim3(256), 0, s, p); break;
  }
}

int launch_conv_small(const float* x, const float* w, float* out, const float* scale, const float* shift, const ConvGeom& c, int flags,
                      int split, unsigned* ctr, float* slabs, hipStream_t s) {
  const char* what = small_linear_flags(flags) ? "linear_fwd_small" : "conv2d_fwd_affine_small";
  if (const char* why = small_conv_refuses(c, flags)) {
    set_last_error("%s: %s (N=%d %dx%d Ci=%d Co=%d k=%d stride=%d pad=%d flags=%d)", what, why, c.N, c.Hi, c.Wi, c.Ci, c.Co, c.k, c.stride,
                   c.pad, flags);
    return 1;
  }
  R3M_REQUIRE(split >= 0 && split <= small_conv_max_split(c), "%s: split=%d outside 0..%d", what, split, small_conv_max_split(c));
  const SmallConvPlan r = small_conv_plan(c, flags, split);
  R3M_REQUIRE(r.S == 1 || (ctr && slabs), "%s: %d slices need a workspace", what, r.S);
  SmallConvParams p;
  p.x = x; p.w = w; p.out = out; p.scale = scale; p.shift = shift; p.slabs = slabs; p.ctr = ctr;
  p.Hi = c.Hi; p.Wi = c.Wi; p.Ci = c.Ci; p.Co = c.Co; p.Ho = c.Ho(); p.Wo = c.Wo(); p.M = c.M();
  p.k = c.k; p.stride = c.stride; p.pad = c.pad; p.flags = flags;
  p.tiles_n = r.tiles_n; p.S = r.S; p.cps = r.cps; p.nch = r.nch; p.cpt = c.Ci / 32;
  if (!small_linear_flags(flags)) launch_small_tile<ST_AFFINE>(p, r, s);
  else if (flags & EPI_GELU) launch_small_tile<ST_BIAS_GELU>(p, r, s);
  else launch_small_tile<ST_BIAS>(p, r, s);
  return check_launch("conv_small");
}

// ---- the workspace of one call (engine.h states the layout) ----
int SmallLaunchSet::add(const ConvGeom& g, int flags, int split, SmallRoute route) {
  if (n == CAP) return -1;
  Entry& t = e[n];
  t = Entry{g, flags, split, false, 0, 0, ctr_bytes};
  if (route != SMALL_NEVER) {
    const SmallConvPlan r = small_conv_plan(g, flags, split);
    t.run = route == SMALL_FORCED ? r.grid != 0 : r.take != 0;
    if (t.run) {
      t.S = r.S;
      t.ctr = ((size_t)r.tiles_m * r.tiles_n * 4 + 255) / 256 * 256;          // one ticket per tile, padded to 256 bytes
      ctr_bytes += t.ctr;
      slab_bytes = std::max(slab_bytes, (size_t)r.S * r.tiles_m * r.bm * g.Co * 4);   // S slabs of tiles_m * bm rows x Co
    }
  }
  return n++;
}

int SmallLaunchSet::reset(void* base, hipStream_t s) const {
  return ticket_bytes() && hipMemsetAsync(base, 0, ticket_bytes(), s) != hipSuccess;
}

int SmallLaunchSet::launch(int i, int rep, void* base, const float* x, const float* w, float* out, const float* scale, const float* shift,
                           hipStream_t s, int flags) const {
  const Entry& t = e[i];
  char* b = static_cast<char*>(base);
  return launch_conv_small(x, w, out, scale, shift, t.g, flags < 0 ? t.flags : flags, t.split,
                           b ? reinterpret_cast<unsigned*>(b + rep * ctr_bytes + t.ctr_off) : nullptr,
                           b ? reinterpret_cast<float*>(b + ticket_bytes()) : nullptr, s);
}

int SmallLaunchSet::linear(int i, int rep, void* base, const float* x, const float* w, const float* bias, float* y, hipStream_t s) const {
  const Entry& t = e[i];
  if (t.run) return launch(i, rep, base, x, w, y, nullptr, bias, s);
  if (!(t.flags & EPI_GELU)) return conv_forward_launch(x, w, y, nullptr, bias, t.g, t.flags, DT_F32, s);
  TRY(conv_forward_launch(x, w, y, nullptr, nullptr, t.g, 0, DT_F32, s));
  return launch_bias_gelu(y, bias, t.g.N, t.g.Co, s);
}

// What the single-launch C entries share: a one-entry set on the caller's workspace — size, check the workspace, reset, launch.
// A shape, flag set or split the kernel does not take goes to the launcher, which says why. sizer: the entry's *_workspace_bytes,
// for the messages; ws_optional: a launch of one slice runs without a workspace.
static int small_entry(const char* what, const char* sizer, bool ws_optional, const float* x, const float* w, float* out,
                       const float* scale, const float* shift, const ConvGeom& g, int flags, int split, void* ws, size_t ws_bytes,
                       hipStream_t s) {
  SmallLaunchSet set;
  set.add(g, flags, split, SMALL_FORCED);
  if (!set.runs(0) || split < 0 || split > small_conv_max_split(g)) return launch_conv_small(x, w, out, scale, shift, g, flags, split, nullptr, nullptr, s);
  const int S = set.e[0].S;
  if (ws_optional) R3M_REQUIRE(S == 1 || ws, "%s: %d slices need a workspace (%s)", what, S, sizer);
  R3M_REQUIRE(ws ? ws_bytes >= set.bytes() : ws_optional, "%s: the workspace has %zu bytes, this launch needs %zu (%s)", what,
              ws ? ws_bytes : (size_t)0, set.bytes(), sizer);
  R3M_REQUIRE(S == 1 || !set.reset(ws, s), "%s: cannot reset the tickets", what);   // one slice touches no ticket
  return set.launch(0, 0, ws, x, w, out, scale, shift, s);
}
static size_t small_entry_bytes(const ConvGeom& g, int flags, int split) {
  SmallLaunchSet set;
  set.add(g, flags, split, SMALL_FORCED);
  return set.bytes();
}

static const char* linear_small_refuses(int M, int K, int N, int flags) {
  if (!small_linear_flags(flags)) return "flags must be 8 (bias), 8|16 (+ ReLU) or 8|256 (+ GELU); the convolution stores belong to r3m_conv2d_fwd_affine_small";
  if (M < 1) return "M must be at least 1";
  if (K < 32 || (K & 31)) return "K must be a multiple of 32";
  if (N < 64 || (N & 63)) return "N must be a multiple of 64";
  return small_conv_refuses({M, 1, 1, K, N, 1, 1, 0}, flags);
}

}  // namespace r3m

using namespace r3m;
static inline hipStream_t S(r3m_stream_t s) { return static_cast<hipStream_t>(s); }

extern "C" {

size_t r3m_conv2d_small_workspace_bytes(int N, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad, int split) {
  return small_entry_bytes({N, Hi, Wi, Ci, Co, k, stride, pad}, EPI_AFFINE | EPI_RELU, split);
}
int r3m_conv2d_fwd_affine_small(const float* x, const float* w, float* out, const float* scale, const float* shift, int N, int Hi, int Wi,
                                int Ci, int Co, int k, int stride, int pad, int flags, int split, void* workspace, size_t workspace_bytes,
                                r3m_stream_t stream) {
  R3M_REQUIRE(x && w && out && scale && shift, "conv2d_fwd_affine_small: null argument");
  R3M_REQUIRE(!small_linear_flags(flags), "conv2d_fwd_affine_small: epilogue flags %d are a Linear store (r3m_linear_fwd_small); this entry "
              "takes 128, 128|16 or 128|2|16", flags);
  return small_entry("conv2d_fwd_affine_small", "r3m_conv2d_small_workspace_bytes", false, x, w, out, scale, shift,
                     {N, Hi, Wi, Ci, Co, k, stride, pad}, flags, split, workspace, workspace_bytes, S(stream));
}
int r3m_debug_conv_small_plan(int N, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad, int flags, int* out, int cap) {
  if (!out || cap < 10) { set_last_error("debug_conv_small_plan: the output buffer needs 10 ints"); return -1; }
  const ConvGeom g{N, Hi, Wi, Ci, Co, k, stride, pad};
  const SmallConvPlan r = small_conv_plan(g, flags, 0);
  const int v[10] = {r.take, r.bm, r.bn, r.S, r.grid, r.cps, r.tiles_m, r.tiles_n, r.nch, r.grid ? small_conv_max_split(g) : 0};
  for (int i = 0; i < 10; ++i) out[i] = v[i];
  return 10;
}

// a Linear over few rows: the 1 x 1 geometry, Linear stores
size_t r3m_linear_small_workspace_bytes(int M, int K, int N, int split) {
  if (linear_small_refuses(M, K, N, EPI_BIAS)) return 0;
  return small_entry_bytes({M, 1, 1, K, N, 1, 1, 0}, EPI_BIAS, split);
}
int r3m_linear_fwd_small(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int flags, int split,
                         void* workspace, size_t workspace_bytes, r3m_stream_t stream) {
  R3M_REQUIRE(x && w && bias && y, "linear_fwd_small: null argument");
  if (const char* why = linear_small_refuses(M, K, N, flags)) {
    set_last_error("linear_fwd_small: %s (M=%d K=%d N=%d flags=%d)", why, M, K, N, flags);
    return 1;
  }
  return small_entry("linear_fwd_small", "r3m_linear_small_workspace_bytes", true, x, w, y, nullptr, bias, {M, 1, 1, K, N, 1, 1, 0}, flags,
                     split, workspace, workspace_bytes, S(stream));
}
int r3m_debug_linear_small_plan(int M, int K, int N, int flags, int* out, int cap) {
  if (!out || cap < 10) { set_last_error("debug_linear_small_plan: the output buffer needs 10 ints"); return -1; }
  for (int i = 0; i < 10; ++i) out[i] = 0;
  if (const char* why = linear_small_refuses(M, K, N, flags)) {
    set_last_error("debug_linear_small_plan: %s (M=%d K=%d N=%d flags=%d)", why, M, K, N, flags);
    return 10;
  }
  return r3m_debug_conv_small_plan(M, 1, 1, K, N, 1, 1, 0, flags, out, cap);
}

}  // extern "C"
