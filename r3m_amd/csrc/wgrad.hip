// r3m_amd — fp32 weight gradient of the convolutions behind the stem, gfx950 (MI355X), on the f32-input MFMA.
//
//   dW[co, tap, ci] = sum_m dY[m, co] * in[pix(m) + off(tap), ci]      (split-K over m, XCD-aware block order)
//
// Replaces the weight-gradient half of ATen's conv2d backward that the reference reaches through torchvision's ResNet
// (r3m/trainer.py, full_loss.backward()).
//
//   wgrad_glds_kernel    the shipped kernel, direct-to-LDS staging through buffer addressing; 128 x 128 tiles when Co and Ci are
//                        multiples of 128, else 64 x 64. Per-tap blocks (1x1, strided, 7x7) or kernel-row blocks (NT = 3: 3-wide
//                        kernels that wgrad_win.hip's shared-window form does not take)
//   wgrad_kernel         register-staged predecessor, probe builds only (R3M_WG_GLDS=0)
//   wgrad_reduce_kernel  fixed-order sum of the split-K partial slabs (also the stem's and the bf16 plans')
//   wgrad_pick_split / launch_wgrad / launch_wgrad_reduce: the split-K factor, the launcher (one body for both tile widths), the reduce
#include "common.h"
#include "conv_dev.h"

namespace r3m {

#ifdef R3M_PROBES   // register-staged predecessor of wgrad_glds_kernel: kept for A/B in probe builds (R3M_WG_GLDS=0), not shipped
// =====================================================================================================
// wgrad: dW[co, tap, ci] = sum_m dY[m, co] * X[pix(m) + off(tap), ci].  GEMM M' = Co tile, N' = Ci tile,
// K' = rows m (split over blockIdx.y). Both operands arrive row(m)-major with channels contiguous, which is exactly
// the [k][i] LDS image the 32x32x2 MFMA wants for conflict-free ds_read_b32 fragment reads.
// Staging is branch-free (clamped addresses + select-to-zero at the LDS write); the (n, oy, ox) decode of the rows a thread
// stages is advanced incrementally (+32 rows per K step) instead of dividing.
// =====================================================================================================
template <int BMt, int BNt>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradParams p) {
  constexpr int BK = 32;
  constexpr int TM = BMt / 64, TN = BNt / 64;
  constexpr int AJ = BMt / 32, BJ = BNt / 32;
  constexpr int A_F4 = BMt / 4, B_F4 = BNt / 4;        // float4 per staged row
  constexpr int A_RPP = 256 / A_F4, B_RPP = 256 / B_F4;  // rows per pass
  __shared__ __attribute__((aligned(16))) float smem[BK * (BMt + BNt)];
  float* sA = smem;
  float* sB = smem + BK * BMt;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int T = p.KH * p.KW;
  const int lid = p.xcd ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int bx = lid % p.gx, by = lid / p.gx;   // by = split index: consecutive logical blocks read the same rows
  const int tap = bx % T;  // the taps of one (co, ci) tile are neighbours: they re-read the same dY rows
  const int tile = bx / T;
  const int tn_ = tile % p.tilesN, tm_ = tile / p.tilesN;
  const int co0 = tm_ * BMt, ci0 = tn_ * BNt;
  const int kh = tap / p.KW, kw = tap - kh * p.KW;
  const int ms = by * p.rows_per_split;
  const int me = min(p.M, ms + p.rows_per_split);

  const int a_c = (tid % A_F4) * 4, a_r = tid / A_F4;
  const int b_c = (tid % B_F4) * 4, b_r = tid / B_F4;
  const bool a_cv = (co0 + a_c) < p.Co;
  const bool b_cv = (ci0 + b_c) < p.Ci;
  const int a_col = a_cv ? co0 + a_c : 0;
  const int b_col = b_cv ? ci0 + b_c : 0;
  const int hw = p.Ho * p.Wo;

  const int q32 = 32 / p.Wo, r32 = 32 - q32 * p.Wo;
  const bool fast_adv = (q32 + 1) <= p.Ho;        // one conditional subtract per axis is enough
  const long long img = (long long)p.Hi * p.Wi * p.Ci;
  long long xb[BJ];
  int xoy[BJ], xox[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int m = ms + b_r + j * B_RPP;
    if (p.simple_rows) {
      xb[j] = 0; xoy[j] = 0; xox[j] = 0;
    } else {
      const int n = m / hw;
      const int rem = m - n * hw;
      xoy[j] = rem / p.Wo;
      xox[j] = rem - xoy[j] * p.Wo;
      xb[j] = (long long)n * img;
    }
  }

  f32x4 ra[AJ], rb[BJ];
  unsigned a_ok = 0, b_ok = 0;
  auto load_tile = [&](int mk) {
    unsigned oka = 0, okb = 0;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int m = mk + a_r + j * A_RPP;
      const bool ok = (m < me) && a_cv;
      oka |= (ok ? 1u : 0u) << j;
      const int mc = min(m, me - 1);
      ra[j] = ldg4(p.dY + (long long)mc * p.Co + a_col);
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      const int m = mk + b_r + j * B_RPP;
      const bool mok = (m < me) && b_cv;
      long long off;
      bool in = true;
      if (p.simple_rows) {
        off = (long long)min(m, me - 1) * p.Ci;
      } else {
        const int iy = xoy[j] * p.stride + kh - p.pad, ix = xox[j] * p.stride + kw - p.pad;
        in = ((unsigned)iy < (unsigned)p.Hi) && ((unsigned)ix < (unsigned)p.Wi);
        const int iyc = min(max(iy, 0), p.Hi - 1), ixc = min(max(ix, 0), p.Wi - 1);
        off = xb[j] + ((long long)iyc * p.Wi + ixc) * p.Ci;
        off = (m < me) ? off : 0;       // rows past the split: any valid address, masked below
      }
      okb |= ((mok && in) ? 1u : 0u) << j;
      rb[j] = ldg4(p.X + off + b_col);
    }
    a_ok = oka; b_ok = okb;
    if (!p.simple_rows) {               // advance the decode to the next K step (+32 rows)
      if (fast_adv) {
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
          int ox = xox[j] + r32, oy = xoy[j] + q32;
          const bool cx = ox >= p.Wo;
          ox = cx ? ox - p.Wo : ox;
          oy = cx ? oy + 1 : oy;
          const bool cy = oy >= p.Ho;
          oy = cy ? oy - p.Ho : oy;
          xb[j] = cy ? xb[j] + img : xb[j];
          xox[j] = ox; xoy[j] = oy;
        }
      } else {
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
          const int m = mk + 32 + b_r + j * B_RPP;
          const int n = m / hw;
          const int rem = m - n * hw;
          xoy[j] = rem / p.Wo;
          xox[j] = rem - xoy[j] * p.Wo;
          xb[j] = (long long)n * img;
        }
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int lrow = lane & 31, lh = lane >> 5;
  const float* fragA = sA + lh * BMt + wm * TM * 32 + lrow;
  const float* fragB = sB + lh * BNt + wn * TN * 32 + lrow;

  if (ms < me) load_tile(ms);
  for (int mk = ms; mk < me; mk += BK) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < AJ; ++j)
      *reinterpret_cast<f32x4*>(sA + (a_r + j * A_RPP) * BMt + a_c) = ((a_ok >> j) & 1u) ? ra[j] : zero4;
#pragma unroll
    for (int j = 0; j < BJ; ++j)
      *reinterpret_cast<f32x4*>(sB + (b_r + j * B_RPP) * BNt + b_c) = ((b_ok >> j) & 1u) ? rb[j] : zero4;
    __syncthreads();
    if (mk + BK < me) load_tile(mk + BK);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      float a[TM], b[TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) a[t] = fragA[kk * 2 * BMt + t * 32];
#pragma unroll
      for (int t = 0; t < TN; ++t) b[t] = fragB[kk * 2 * BNt + t * 32];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
    }
    __syncthreads();
  }

  float* out = p.out + (long long)by * p.Co * T * p.Ci;
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (co >= p.Co) continue;
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const int ci = ci0 + (wn * TN + tn) * 32 + lrow;
        if (ci < p.Ci) out[((long long)co * T + tap) * p.Ci + ci] = acc[tm][tn][r];
      }
    }
}

#endif  // R3M_PROBES

// =====================================================================================================
// wgrad, direct-to-LDS staging through BUFFER addressing (round 3). Same GEMM as the register-staged probe kernel; the
// [k][channel] LDS image is lane-linear (a row of 64 or 128 floats = 256/512 B, one DMA instruction covers 4 or 2 consecutive
// k rows), so no swizzle is needed and the b32 fragment reads stay conflict-free. Two stages, one barrier per K step.
//
// Why buffer addressing: on gfx950 the f32-input MFMA shares the SIMD's fp32 lanes with the VALU, so every vector
// instruction in the K loop costs matrix time. `global_load_lds` needs a 64-bit per-lane address, i.e. per DMA
// piece a 64-bit add, the (oy, ox) walk, four compares and a pointer select in VALU — ~25 vector instructions per X piece of a
// 3x3 convolution, ~125 per 64 MFMAs. `buffer_load_dwordx4 ... lds` takes a wave-uniform 128-bit descriptor (base, bytes) in
// SGPRs plus a 32-bit per-lane offset, and lanes whose offset is >= the descriptor's byte count land ZEROS in LDS
// (tools/micro/bufload.hip). So:
//   * dY, and X of 1x1/stride-1 convolutions (rows are linear in m): the per-lane offset is a CONSTANT; a K step advances the
//     descriptor base by 32 rows and shrinks its byte count with four scalar instructions — rows past the end of the split
//     fall off the descriptor and read zeros. No vector instruction per piece at all.
//   * X of 3x3 / strided convolutions: a DMA instruction covers only 2 (128-wide tile) or 4 (64-wide) consecutive rows m, and
//     which rows is wave-uniform — the (frame, oy, ox) walk, the tap shift and the padding test of every staged row run on the
//     SCALAR unit (in the shadow of the MFMAs); a padding row gets an out-of-range offset. Per lane: pick its row's scalar
//     offset and add the channel offset = 3 (or 6) vector instructions per piece.
// =====================================================================================================
// NT = 3 ("kernel rows", round 3): one block owns the THREE taps (kh, 0..2) of one row of a 3-wide kernel for its (co, ci) tile,
// with three accumulator sets: the dY rows of a K step are staged and read from LDS ONCE for the three taps, the scalar cursor
// walk is shared (the taps differ by one pixel in x) — 2/3 of the DMA instructions and fragment reads per MFMA of the per-tap
// form. K steps of 16 rows keep the two stages at 64 KB (128-wide tile: 2 blocks per CU as before).
template <int BMt, int BNt, int BK = 32, int NT = 1, int IL = -1, int SR = -1>   // IL: DMA pieces spread between the MFMAs (1), in one burst (0), or p.interleave (-1); SR: 1x1 "simple rows" known at compile time (1 / 0) or p.simple_rows (-1)
__global__ __launch_bounds__(256, (NT == 3 && BMt == 128) ? 2 : 1) void wgrad_glds_kernel(const WgradParams p) {
  static_assert(BK == 32 || BK == 16, "K step of 32 or 16 rows");
  static_assert(NT == 1 || NT == 3, "one tap, or the three taps of a kernel row");
  // 128x128: waves 1 x 4, each 128 (co, interleaved: MFMA tile tm owns channels 4*i + tm) x 32 (ci) -> the A fragment of all
  // four tiles is ONE ds_read_b128 per K pair; 64x64: waves 2 x 2, each 32 x 32.
  constexpr bool WIDE = (BMt == 128);
  constexpr int TM = WIDE ? 4 : BMt / 64, TN = WIDE ? 1 : BNt / 64;
  constexpr int WR = BK / 4;                            // k rows staged per wave per stage
  constexpr int A_RPI = 256 / BMt, B_RPI = 256 / BNt;   // k rows covered by one 1 KiB DMA instruction
  constexpr int AJ = WR / A_RPI, BJ = WR / B_RPI;       // DMA pieces per wave per stage (a B piece = NT instructions)
  static_assert(AJ >= 1 && BJ >= 1, "a wave stages whole DMA instructions");
  constexpr int B_TILE = BK * BNt;                      // floats of one tap's X tile
  constexpr int STAGE = BK * BMt + NT * B_TILE;
  __shared__ __attribute__((aligned(128))) float smem[2 * STAGE];

  const bool simple_rows = NT == 1 && (SR < 0 ? p.simple_rows != 0 : SR != 0);   // a kernel-row block (NT = 3) never has 1x1 "simple" rows
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = WIDE ? 0 : (wave_s >> 1), wn = WIDE ? wave_s : (wave_s & 1);
  const int T = p.KH * p.KW;
  const int TG = T / NT;                                // tap groups per tile (NT = 3: kernel rows)
  const int lid = p.xcd ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int bx = lid % p.gx, by = lid / p.gx;   // by = split index: consecutive logical blocks read the same rows
  const int tap0 = (bx % TG) * NT;
  const int tile = bx / TG;
  const int tn_ = tile % p.tilesN, tm_ = tile / p.tilesN;
  const int co0 = tm_ * BMt, ci0 = tn_ * BNt;
  const int kh = tap0 / p.KW, kw0 = tap0 - kh * p.KW;
  const int ms = by * p.rows_per_split;
  const int me = min(p.M, ms + p.rows_per_split);
  const int hw = p.Ho * p.Wo;

  // lane -> (k row within the instruction, first channel); the per-lane offsets below never change in the K loop
  const int a_k = lane / (BMt / 4), a_c = (lane % (BMt / 4)) * 4;
  const int b_k = lane / (BNt / 4), b_c = (lane % (BNt / 4)) * 4;
  const unsigned a_chan = (co0 + a_c) < p.Co ? (unsigned)a_c * 4u : BUF_OOB;
  const unsigned b_chan = (ci0 + b_c) < p.Ci ? (unsigned)b_c * 4u : BUF_OOB;

  // A operand (dY): descriptor = [row ms + BK*step, end of the split) x channels from co0
  const float* a_base = p.dY + (long long)ms * p.Co + co0;
  int a_left = (int)(((long long)(me - ms) * p.Co - co0) * 4);      // bytes (host: a split spans < 2 GB)
  const int a_stepb = BK * p.Co * 4;
  unsigned a_voff[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) a_voff[j] = (unsigned)((wave_s * WR + j * A_RPI + a_k) * p.Co) * 4u + a_chan;

  // B operand (X)
  const long long img = (long long)p.Hi * p.Wi * p.Ci;
  const float* b_base;
  int b_left;
  const int b_stepb = BK * p.Ci * 4;
  unsigned b_voff[BJ];             // simple rows: constant per-lane offsets
  // non-simple rows: ONE scalar cursor (frame offset, oy, ox) that walks the WR consecutive rows this wave stages per K step,
  // then jumps the BK - WR rows to its rows of the next step; `c_left` = rows from the cursor to the end of the split
  int c_ox = 0, c_oy = 0, c_left = 0;
  unsigned c_f = 0;                // byte offset of the cursor row's frame from b_base
  constexpr int JUMP = BK - WR;
  const int qj = JUMP / p.Wo, rj = JUMP - qj * p.Wo;
  const unsigned imgb = (unsigned)(img * 4);
  const int pixb = p.Ci * 4;       // bytes between the X rows of neighbouring taps (one pixel)
  const int kh_p = kh - p.pad, kw_p = kw0 - p.pad;
  if (simple_rows) {
    b_base = p.X + (long long)ms * p.Ci + ci0;
    b_left = (int)(((long long)(me - ms) * p.Ci - ci0) * 4);
#pragma unroll
    for (int j = 0; j < BJ; ++j) b_voff[j] = (unsigned)((wave_s * WR + j * B_RPI + b_k) * p.Ci) * 4u + b_chan;
  } else {
    const int n0 = ms / hw;        // first frame of the split: 32-bit offsets are relative to it
    b_base = p.X + (long long)n0 * img + ci0;
    const long long rest = ((long long)(p.N - n0) * img - ci0) * 4;
    b_left = rest < (long long)BUF_OOB ? (int)rest : (int)BUF_OOB;
#pragma unroll
    for (int j = 0; j < BJ; ++j) b_voff[j] = 0;
    const int m = ms + wave_s * WR;
    const int n = m / hw;
    const int rem = m - n * hw;
    c_oy = rem / p.Wo;
    c_ox = rem - c_oy * p.Wo;
    c_f = (unsigned)(n - n0) * imgb;
    c_left = me - m;
  }
  bool b_is[B_RPI];                // lane masks: "my row is sub-row r of the instruction"
#pragma unroll
  for (int r = 0; r < B_RPI; ++r) b_is[r] = (b_k == r);

  // one DMA piece (pc < AJ: dY rows, else X rows of all NT taps) into `stage`
  auto issue_piece = [&](int stage, auto pc_c) __attribute__((always_inline)) {
    constexpr int pc = decltype(pc_c)::value;
    if (R3M_PROBE(p) & 1) return;                       // timing probes (probe builds only; wrong results)
    if ((R3M_PROBE(p) & 2) && pc >= AJ) return;
    if ((R3M_PROBE(p) & 4) && pc < AJ) return;
    if constexpr (pc < AJ) {
      constexpr int j = pc;
      float* la = smem + stage * STAGE + wave_s * WR * BMt;
      buf_dma16(a_base, a_left, la + j * A_RPI * BMt, a_voff[j]);
    } else {
      constexpr int j = pc - AJ;
      float* lb = smem + stage * STAGE + BK * BMt + wave_s * WR * BNt + j * B_RPI * BNt;
      if (simple_rows) {
        buf_dma16(b_base, b_left, lb, b_voff[j]);
      } else {
        unsigned so[NT][B_RPI];
#pragma unroll
        for (int r = 0; r < B_RPI; ++r) {     // scalar unit: tap shift, padding tests, row offset, cursor to the next row
          const int iy = c_oy * p.stride + kh_p, ix0 = c_ox * p.stride + kw_p;
          const bool rowok = ((unsigned)iy < (unsigned)p.Hi) && (c_left > 0);
          const unsigned off0 = c_f + (unsigned)((iy * p.Wi + ix0) * p.Ci) * 4u;
#pragma unroll
          for (int t = 0; t < NT; ++t)
            so[t][r] = (rowok && (unsigned)(ix0 + t) < (unsigned)p.Wi) ? off0 + (unsigned)(t * pixb) : BUF_OOB;
          c_left -= 1;
          c_ox += 1;
          if (c_ox == p.Wo) {
            c_ox = 0;
            c_oy += 1;
            if (c_oy == p.Ho) { c_oy = 0; c_f += imgb; }
          }
        }
        if constexpr (j == BJ - 1) {          // the wave's rows of this K step are issued: jump to its rows of the next one
          c_left -= JUMP;
          c_ox += rj;
          if (c_ox >= p.Wo) { c_ox -= p.Wo; c_oy += 1; }
          c_oy += qj;
          while (c_oy >= p.Ho) { c_oy -= p.Ho; c_f += imgb; }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          unsigned voff = so[t][0];
#pragma unroll
          for (int r = 1; r < B_RPI; ++r) voff = b_is[r] ? so[t][r] : voff;
          buf_dma16(b_base, b_left, lb + t * B_TILE, voff + b_chan);
        }
      }
    }
  };
  // after the last piece of a K step: both descriptors move on by BK rows (scalar)
  auto advance = [&]() __attribute__((always_inline)) {
    a_base += BK * p.Co;
    a_left = a_left > a_stepb ? a_left - a_stepb : 0;
    if (simple_rows) {
      b_base += BK * p.Ci;
      b_left = b_left > b_stepb ? b_left - b_stepb : 0;
    }
  };
  auto issue = [&](int stage) __attribute__((always_inline)) {
    static_for<AJ + BJ>([&](auto pc_c) __attribute__((always_inline)) { issue_piece(stage, pc_c); });
    advance();
  };

  f32x16 acc[NT][TM][TN];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][a][b][r] = 0.f;

  const int lrow = lane & 31, lh = lane >> 5;
  const float* fragA = smem + lh * BMt + (WIDE ? 4 * lrow : wm * TM * 32 + lrow);
  const float* fragB = smem + BK * BMt + lh * BNt + wn * TN * 32 + lrow;
  // MFMAs of one stage; when dma_stage >= 0 the next K step's DMA pieces are spread between them so that their issue cost
  // hides behind this wave's own MFMAs
  auto mfma_stage = [&](const float* fa, const float* fb, int dma_stage) __attribute__((always_inline)) {
    constexpr int NP = AJ + BJ;
    constexpr int EVERY = (BK / 2) / NP;     // K pairs between two pieces
    static_assert(EVERY >= 1, "at most one DMA piece per K pair");
    static_for<BK / 2>([&](auto kk_c) __attribute__((always_inline)) {
      constexpr int kk = decltype(kk_c)::value;
      float a[TM];
      if constexpr (WIDE) {
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(fa + kk * 2 * BMt);
#pragma unroll
        for (int t = 0; t < TM; ++t) a[t] = a4[t];
      } else {
#pragma unroll
        for (int t = 0; t < TM; ++t) a[t] = fa[kk * 2 * BMt + t * 32];
      }
#pragma unroll
      for (int tp = 0; tp < NT; ++tp) {
        float b[TN];
#pragma unroll
        for (int t = 0; t < TN; ++t) b[t] = fb[tp * B_TILE + kk * 2 * BNt + t * 32];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tp][tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b[tn], acc[tp][tm][tn], 0, 0, 0);
      }
      if constexpr ((kk % EVERY) == EVERY - 1 && kk / EVERY < NP) {
        if (dma_stage >= 0) {
          __builtin_amdgcn_sched_barrier(0);
          issue_piece(dma_stage, std::integral_constant<int, kk / EVERY>{});
          if constexpr (kk / EVERY == NP - 1) advance();
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    });
  };

  const int nk = (me - ms + BK - 1) / BK;
  if (nk > 0) issue(0);
  int kt = 0;
  const bool il = IL < 0 ? (p.interleave != 0) : (IL != 0);
  for (; kt + 1 < nk; kt += 2) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (il) {
      mfma_stage(fragA, fragB, 1);
    } else {
      issue(1);
      mfma_stage(fragA, fragB, -1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (il) {
      mfma_stage(fragA + STAGE, fragB + STAGE, (kt + 2 < nk) ? 0 : -1);
    } else {
      if (kt + 2 < nk) issue(0);
      mfma_stage(fragA + STAGE, fragB + STAGE, -1);
    }
  }
  if (kt < nk) {   // odd tail
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    mfma_stage(fragA, fragB, -1);
  }

  float* out = p.out + (long long)by * p.Co * T * p.Ci;
#pragma unroll
  for (int tp = 0; tp < NT; ++tp)
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rho = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int co = WIDE ? co0 + 4 * rho + tm : co0 + (wm * TM + tm) * 32 + rho;
        if (co >= p.Co) continue;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          const int ci = ci0 + (wn * TN + tn) * 32 + lrow;
          if (ci < p.Ci) out[((long long)co * T + tap0 + tp) * p.Ci + ci] = acc[tp][tm][tn][r];
        }
      }
}

// debug_occupancy (conv.hip), fourth output: resident blocks per CU the runtime predicts for the 128 x 128 per-tap kernel
int wgrad_debug_occupancy(int* out) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, wgrad_glds_kernel<128, 128>, 256, 0) != hipSuccess) return 1;
  *out = n;
  return 0;
}

#ifdef R3M_PROBES
static bool wg_use_glds() {
  const int v = R3M_ENV_INT("R3M_WG_GLDS", 1) != 0;
  return v == 1;
}
#endif

static inline bool wg_wide(int Co, int Ci) { return (Co % 128 == 0) && (Ci % 128 == 0); }
// 3-wide kernels run one block per kernel row (wgrad_glds_kernel NT = 3). R3M_WG_ROWS=0 (probe builds): per-tap blocks.
static bool wg_rows(int KW) {
  const int v = R3M_ENV_INT("R3M_WG_ROWS", 1);
  return v && KW == 3;
}

// Split-K factor: enough blocks for two full waves of resident blocks (128x128: 2 blocks/CU x 256 CUs; 64x64: 5/CU), as few
// splits as that allows (every split writes and re-reads a full dW slab), never fewer than 8 K steps per block.
int wgrad_pick_split(int M, int Co, int Ci, int T) {
  const bool wide = wg_wide(Co, Ci);
  const int bt = wide ? 128 : 64;
  long long tiles = (long long)ceil_div(Co, bt) * ceil_div(Ci, bt) * T;
  if (T == 9 && wg_rows(3)) tiles /= 3;     // kernel-row blocks cover three taps each
  const int tgt = R3M_ENV_INT("R3M_WG_BLOCKS", 0);                       // probe builds: block target override
  const long long target = tgt > 0 ? tgt : (wide ? 1024 : 2560);
  long long split = target / tiles;   // floor: never spill a few blocks into an extra wave
  const long long max_split = (M + 255) / 256;
  if (split > max_split) split = max_split;
  if (split < 1) split = 1;
  long long rps = ((M + split - 1) / split + 31) / 32 * 32;
  return ceil_div(M, rps);
}

// The launch for one tile width: BT = 128 (wg_wide) or 64. p.gx = blocks per split.
template <int BT>
static int launch_wgrad_tiles(WgradParams& p, int splitK, hipStream_t s) {
  constexpr int IL = BT == 128 ? 1 : 0;   // kernel-row and 3x3 / strided per-tap blocks: DMA pieces between the MFMAs on the 128-wide tile only
  const int T = p.KH * p.KW;
  const double flops = 2.0 * (double)p.M * (double)p.Co * (double)T * p.Ci;
  p.tilesN = ceil_div(p.Ci, BT);
  const int tiles = ceil_div(p.Co, BT) * p.tilesN * T;
  prof_begin(BT == 128 ? KC_WGRAD_WIDE : KC_WGRAD_NARROW, flops, p.M, p.Co, p.Ci, T, s);
  p.gx = tiles;
#ifdef R3M_PROBES
  if (!wg_use_glds()) hipLaunchKernelGGL((wgrad_kernel<BT, BT>), dim3(tiles * splitK), dim3(256), 0, s, p);
  else
#endif
  if (wg_rows(p.KW) && R3M_ENV_INT("R3M_WG_WIN", 1) && wgrad_rowwin_eligible(p)) {   // 3x3 "same" convolutions: shared input window (wgrad_win.hip)
    if (int e = launch_wgrad_rowwin(p, splitK, s)) return e;
  } else if (wg_rows(p.KW)) {   // 3-wide kernels: one block per kernel row (three taps), K steps of 16 rows
    p.gx = ceil_div(p.Co, BT) * p.tilesN * p.KH;
    hipLaunchKernelGGL((wgrad_glds_kernel<BT, BT, 16, 3, IL>), dim3(p.gx * splitK), dim3(256), 0, s, p);
  } else {
#ifdef R3M_PROBES
    hipLaunchKernelGGL((wgrad_glds_kernel<BT, BT>), dim3(tiles * splitK), dim3(256), 0, s, p);
#else
    // shipped builds: the two switches of the per-tap kernel are fixed per launch kind -> two compile-time variants
    if (p.simple_rows) hipLaunchKernelGGL((wgrad_glds_kernel<BT, BT, 32, 1, 0, 1>), dim3(tiles * splitK), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((wgrad_glds_kernel<BT, BT, 32, 1, IL, 0>), dim3(tiles * splitK), dim3(256), 0, s, p);
#endif
  }
  return 0;
}

int launch_wgrad(const WgradParams& p0, int splitK, hipStream_t s) {
  WgradParams p = p0;
  R3M_REQUIRE(p.Ci % 4 == 0 && p.Co % 4 == 0, "wgrad: channel counts must be multiples of 4 (Co=%d Ci=%d)", p.Co, p.Ci);
  R3M_REQUIRE(splitK >= 1, "wgrad: splitK=%d", splitK);
  p.rows_per_split = ((p.M + splitK - 1) / splitK + 31) / 32 * 32;
  R3M_REQUIRE(ceil_div(p.M, p.rows_per_split) == splitK, "wgrad: splitK=%d does not tile M=%d", splitK, p.M);
  {   // buffer addressing: a block's operands are reached through 32-bit offsets from the first row / frame of its split
    const long long lim = 0x7FFFF000LL;
    const long long a_span = (long long)p.rows_per_split * p.Co * 4;
    const long long frames = (long long)p.rows_per_split / ((long long)p.Ho * p.Wo) + 2;
    const long long b_span = p.simple_rows ? (long long)p.rows_per_split * p.Ci * 4 : frames * p.Hi * p.Wi * p.Ci * 4;
    R3M_REQUIRE(a_span < lim && b_span < lim, "wgrad: one split spans %lld / %lld bytes (limit 2 GiB): raise splitK (%d)", a_span, b_span, splitK);
  }
  {
    // DMA pieces spread between the MFMAs (one per 2 K pairs) or issued in one burst before them. Round 3, buffer addressing,
    // same box (profiles/r03_wgrad_buffer_ab.txt): spreading wins where a piece carries scalar work — the (oy, ox) walk of 3x3 /
    // strided X rows on a 128-wide tile (115.8 -> 118-123 TFLOP/s) — and loses where it does not (1x1: 134 -> 130) and on the
    // 64-wide tile (107.5 -> 100). Probe builds: R3M_WG_INTERLEAVE = 0 / 1 forces it.
    const int il = R3M_ENV_INT("R3M_WG_INTERLEAVE", -1);
    p.interleave = il >= 0 ? il : (!p.simple_rows && wg_wide(p.Co, p.Ci));
    const int xc = R3M_ENV_INT("R3M_WG_XCD", 1);
    p.xcd = xc;
    p.debug = R3M_ENV_INT("R3M_WG_DEBUG", 0);       // probe builds only (R3M_ENV_INT is the default in shipped builds)
  }
  if (int e = wg_wide(p.Co, p.Ci) ? launch_wgrad_tiles<128>(p, splitK, s) : launch_wgrad_tiles<64>(p, splitK, s)) return e;
  const int T = p.KH * p.KW;
  prof_bytes(4.0 * ((double)p.M * p.Co + (double)p.N * p.Hi * p.Wi * p.Ci + (double)splitK * p.Co * T * p.Ci));
  prof_end(s);
  return check_launch("wgrad");
}

// dW[i] (+)= sum_s partial[s][i]   — fixed summation order: deterministic gradients
// dW[i] (+)= sum over split-K slices of partial[s][i], fixed order (deterministic). A block is TX float4 columns x TY slice
// groups (TX * TY = 256): group g adds slices g, g+TY, ...; the groups are combined through LDS in group order. Small weight
// tensors (e.g. 64x64x9: 9216 float4, 284 slices) get TY = 16 so that the launch has hundreds of blocks and short load chains
// instead of 36 blocks walking 284 slices one after the other (that was up to 1 ms per launch).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dW,
                                                            long long n4, long long n, int splitK, int accumulate, int tx_log2) {
  __shared__ f32x4 red[256];
  const int TX = 1 << tx_log2, TY = 256 >> tx_log2;
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log2;
  const long long i = (long long)blockIdx.x * TX + tx;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (i < n4)
    for (int sidx = ty; sidx < splitK; sidx += TY) v += ldg4(partial + sidx * n + i * 4);
  if (TY == 1) {
    if (i < n4) {
      if (accumulate) v += *reinterpret_cast<const f32x4*>(dW + i * 4);
      *reinterpret_cast<f32x4*>(dW + i * 4) = v;
    }
    return;
  }
  red[threadIdx.x] = v;
  __syncthreads();
  if (ty == 0 && i < n4) {
    for (int g = 1; g < TY; ++g) v += red[(g << tx_log2) + tx];
    if (accumulate) v += *reinterpret_cast<const f32x4*>(dW + i * 4);
    *reinterpret_cast<f32x4*>(dW + i * 4) = v;
  }
}
int launch_wgrad_reduce(const float* partial, float* dW, long long n, int splitK, int accumulate, hipStream_t s) {
  R3M_REQUIRE(n % 4 == 0, "wgrad_reduce: n=%lld must be a multiple of 4", n);
  const long long n4 = n / 4;
  int tx_log2 = 8;                                     // TX = 256, TY = 1
  while (tx_log2 > 4 && ceil_div(n4, 1 << tx_log2) < 1024 && (256 >> tx_log2) * 2 <= splitK) --tx_log2;   // more slice groups for small tensors
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(ceil_div(n4, 1 << tx_log2)), dim3(256), 0, s, partial, dW, n4, n, splitK, accumulate, tx_log2);
  return check_launch("wgrad_reduce");
}

}  // namespace r3m
