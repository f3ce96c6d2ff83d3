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
//   wgrad_reduce_kernel  fixed-order sum of the split-K partial slabs (also the stem's and the bf16 plans')
//   wgrad_plan / launch_wgrad / launch_wgrad_reduce: the dispatch of the WHOLE family, fp32 and bf16 (route, tile, split-K factor
//                        decided once, then one switch over the route), and the reduce. Shared device code: wgrad_dev.h
#include "wgrad_dev.h"

namespace r3m {

// =====================================================================================================
// wgrad, direct-to-LDS staging through BUFFER addressing (round 3; the A/B against its register-staged predecessor is on record
// in profiles/r03_wgrad_buffer_ab.txt). The [k][channel] LDS image is lane-linear (a row of 64 or 128 floats = 256/512 B, one DMA instruction covers 4 or 2 consecutive
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
template <int BMt, int BNt, int BK, int NT, int IL, int SR = 0>   // IL: DMA pieces spread between the MFMAs (1) or in one burst (0); SR: 1x1 "simple rows" (1 / 0)
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

  constexpr bool simple_rows = NT == 1 && SR != 0;      // a kernel-row block (NT = 3) never has 1x1 "simple" rows
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = WIDE ? 0 : (wave_s >> 1), wn = WIDE ? wave_s : (wave_s & 1);
  const int T = p.KH * p.KW;
  const WgBlock blk = wg_block<BMt, BNt, false>(p, T / NT);   // tap groups per tile (NT = 3: kernel rows)
  const int tap0 = blk.grp * NT;
  const int co0 = blk.co0, ci0 = blk.ci0, ms = blk.ms, me = blk.me;
  const int kh = tap0 / p.KW, kw0 = tap0 - kh * p.KW;
  const int hw = p.Ho * p.Wo;

  // lane -> (k row within the instruction, first channel); the per-lane offsets below never change in the K loop
  const int a_k = lane / (BMt / 4), a_c = (lane % (BMt / 4)) * 4;
  const int b_k = lane / (BNt / 4), b_c = (lane % (BNt / 4)) * 4;
  const unsigned a_chan = (co0 + a_c) < p.Co ? (unsigned)a_c * 4u : BUF_OOB;
  const unsigned b_chan = (ci0 + b_c) < p.Ci ? (unsigned)b_c * 4u : BUF_OOB;

  // A operand (dY): descriptor = [row ms + BK*step, end of the split) x channels from co0
  WgRows a = wg_rows<4>(p.dY, ms, me, p.Co, co0, BK);
  unsigned a_voff[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) a_voff[j] = (unsigned)((wave_s * WR + j * A_RPI + a_k) * p.Co) * 4u + a_chan;

  // B operand (X)
  const long long img = (long long)p.Hi * p.Wi * p.Ci;
  WgRows b = wg_rows<4>(p.X, ms, me, p.Ci, ci0, BK);      // simple rows; else the frames from the split's first one
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
#pragma unroll
    for (int j = 0; j < BJ; ++j) b_voff[j] = (unsigned)((wave_s * WR + j * B_RPI + b_k) * p.Ci) * 4u + b_chan;
  } else {
    const int n0 = ms / hw;        // first frame of the split: 32-bit offsets are relative to it
    b.base = reinterpret_cast<const char*>(p.X + (long long)n0 * img + ci0);
    const long long rest = ((long long)(p.N - n0) * img - ci0) * 4;
    b.left = rest < (long long)BUF_OOB ? (int)rest : (int)BUF_OOB;
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
      buf_dma16(a.base, a.left, la + j * A_RPI * BMt, a_voff[j]);
    } else {
      constexpr int j = pc - AJ;
      float* lb = smem + stage * STAGE + BK * BMt + wave_s * WR * BNt + j * B_RPI * BNt;
      if (simple_rows) {
        buf_dma16(b.base, b.left, lb, b_voff[j]);
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
          buf_dma16(b.base, b.left, lb + t * B_TILE, voff + b_chan);
        }
      }
    }
  };
  // after the last piece of a K step: both descriptors move on by BK rows (scalar)
  auto advance = [&]() __attribute__((always_inline)) {
    a.advance();
    if (simple_rows) b.advance();
  };
  auto issue = [&](int stage) __attribute__((always_inline)) {
    static_for<AJ + BJ>([&](auto pc_c) __attribute__((always_inline)) { issue_piece(stage, pc_c); });
    advance();
  };

  f32x16 acc[NT][TM][TN];
  wg_clear(acc);

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
  constexpr bool il = IL != 0;
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

  wg_store<WIDE, true>(p, blk, T, tap0, wm, wn, lrow, lh, acc);
}

// debug_occupancy (conv.hip), fourth output: resident blocks per CU the runtime predicts for the 128 x 128 per-tap kernel
int wgrad_debug_occupancy(int* out) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, wgrad_glds_kernel<128, 128, 32, 1, 1, 0>, 256, 0) != hipSuccess) return 1;
  *out = n;
  return 0;
}

// =====================================================================================================
// The family's dispatch (fp32 and bf16): wgrad_plan decides, launch_wgrad launches what the plan says.
// =====================================================================================================
// Pure: geometry + dtype (+ in probe builds the switches, which are read here and nowhere else; shipped builds compile their
// defaults in). Launches nothing, checks nothing.
WgradPlan wgrad_plan(const WgradParams& p) {
  const bool sw_rows = R3M_ENV_INT("R3M_WG_ROWS", 1) != 0;        // 0: 3-wide fp32 kernels run per-tap blocks
  const bool sw_win = R3M_ENV_INT("R3M_WG_WIN", 1) != 0;          // 0: 3x3 "same" fp32 layers run the kernel-row form
  const bool sw_rows16 = R3M_ENV_INT("R3M_WG16_ROWS", 1) != 0;    // 0: bf16 3-wide kernels on the 128-wide tile run per-tap blocks
  const bool sw_taps16 = R3M_ENV_INT("R3M_WG16_HALO", 1) != 0;    // 0: no bf16 launch runs the all-taps kernel
  WgradPlan r;
  r.xcd = R3M_ENV_INT("R3M_WG_XCD", 1);
  r.debug = R3M_ENV_INT("R3M_WG_DEBUG", 0);
  r.fast = 0;
  r.lds_bytes = 0;
  const int T = p.KH * p.KW;
  const bool wide = wg_wide(p.Co, p.Ci);
  // Split-K: enough blocks for `target`, as few splits as that allows (every split writes and re-reads a full dW slab), never
  // fewer than 256 rows per split. `blocks` = blocks per split as the policy counts them — NOT always r.gx, see the two notes.
  long long blocks, target;
  if (p.dtype == DT_F32) {
    const bool rows = sw_rows && p.KW == 3;        // 3-wide kernels: one block per kernel row (three taps)
    r.route = !rows ? (p.simple_rows ? WG_TAPS_SIMPLE : WG_TAPS_GATHER) : (sw_win && wgrad_rowwin_eligible(p)) ? WG_WINDOW : WG_ROWS;
    r.tile = wide ? 128 : 64;
    r.bk = r.route == WG_ROWS ? 16 : 32;           // kernel rows: K steps of 16 rows keep the two stages at 64 KB
    r.tilesN = ceil_div(p.Ci, r.tile);
    const int tiles = ceil_div(p.Co, r.tile) * r.tilesN;
    r.gx = tiles * (rows ? p.KH : T);
    if (r.route == WG_WINDOW) r.lds_bytes = wgrad_rowwin_lds_bytes(r.tile);
    // two full waves of resident blocks (128 x 128: 2 blocks / CU x 256 CUs; 64 x 64: 5 / CU)
    blocks = (long long)tiles * T;
    if (T == 9 && sw_rows) blocks /= 3;            // note 1: three taps per block is taken from T == 9, not from the route (KW == 3)
    target = wide ? 1024 : 2560;
  } else {
    const bool taps9 = sw_taps16 && wgrad_halo_eligible(p);
    const bool rows = !taps9 && sw_rows16 && wide && p.KW == 3;
    r.route = taps9 ? WG16_ALL_TAPS : rows ? WG16_ROWS : WG16_TAPS;
    r.tile = (wide && !taps9) ? 128 : 64;
    // K steps of 32 rows for the 128 x 128 tile (32 KB of stages instead of 64: -16 % measured over ResNet-50), 64 rows for the
    // 64 x 64 tile (32 rows measured +5 % there) and the all-taps kernel
    r.bk = r.tile == 128 ? 32 : 64;
    r.fast = rows && (32 / p.Wo + 1) <= p.Ho;      // one K step advances a row by less than one frame (see wgrad_bf16_kernel)
    r.tilesN = p.Ci / r.tile;
    r.gx = (p.Co / r.tile) * r.tilesN * (taps9 ? 1 : rows ? p.KH : T);
    if (taps9) r.lds_bytes = wgrad_halo_lds_bytes(p.Wi);
    // fill the chip ~4 (wide) / ~10 (narrow) times; kernel rows: exactly one round of the 2 blocks a CU holds (same box: 802 ->
    // 835, 717 -> 750 TFLOP/s against 1024); all nine taps: 512 splits of the 64-channel layers fill the chip
    const int tiles = wide ? (p.Co / 128) * (p.Ci / 128) * T : ceil_div(p.Co, 64) * ceil_div(p.Ci, 64) * T;
    blocks = tiles > 0 ? tiles : 1;
    target = wide ? 1024 : (T == 9 && sw_taps16) ? 512 * 9 : 2560;   // note 2: the all-taps target goes to EVERY narrow T == 9 launch, eligible or not
    if (sw_rows16 && wide && T == 9) {             // (and wide 3x3 layers count kernel-row blocks even where the all-taps kernel runs them)
      blocks = tiles / 3;
      target = 512;
    }
  }
  long long split = target / blocks;               // floor: never spill a few blocks into an extra wave
  const long long max_split = ceil_div(p.M, 256);
  if (split > max_split) split = max_split;
  if (split < 1) split = 1;
  if (p.dtype == DT_F32) {                         // rows per split a multiple of 32, and no empty split
    const long long rps = ((p.M + split - 1) / split + 31) / 32 * 32;
    r.split = ceil_div(p.M, rps);
    r.rows_per_split = ((p.M + r.split - 1) / r.split + 31) / 32 * 32;
  } else {                                         // a multiple of 64; trailing splits may be empty (they write zeros)
    r.split = (int)split;
    r.rows_per_split = ceil_div(ceil_div(p.M, r.split), 64) * 64;
  }
  return r;
}

// fp32 per-tap and kernel-row blocks. DMA pieces spread between the MFMAs (one per 2 K pairs) or issued in one burst before them:
// round 3, buffer addressing, same box (profiles/r03_wgrad_buffer_ab.txt): spreading wins where a piece carries scalar work — the
// (oy, ox) walk of 3x3 / strided X rows on a 128-wide tile (115.8 -> 118-123 TFLOP/s) — and loses where it does not (1x1: 134 ->
// 130) and on the 64-wide tile (107.5 -> 100).
template <int BK, int NT, int SR>
static void launch_wgrad_glds(const WgradParams& p, const WgradPlan& r, hipStream_t s) {
  const dim3 grid(r.gx * r.split);
  if (r.tile == 128) hipLaunchKernelGGL((wgrad_glds_kernel<128, 128, BK, NT, SR ? 0 : 1, SR>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((wgrad_glds_kernel<64, 64, BK, NT, 0, SR>), grid, dim3(256), 0, s, p);
}

int launch_wgrad(const WgradParams& p0, const WgradPlan& r, hipStream_t s) {
  WgradParams p = p0;
  const int T = p.KH * p.KW, esz = p.dtype == DT_F32 ? 4 : 2;
  if (p.dtype == DT_F32) R3M_REQUIRE(p.Ci % 4 == 0 && p.Co % 4 == 0, "wgrad: channel counts must be multiples of 4 (Co=%d Ci=%d)", p.Co, p.Ci);
  else R3M_REQUIRE(p.Co % 64 == 0 && p.Ci % 64 == 0, "wgrad(bf16): Co=%d, Ci=%d must be multiples of 64", p.Co, p.Ci);
  R3M_REQUIRE(r.split >= 1 && (long long)r.split * r.rows_per_split >= p.M, "wgrad: %d splits of %d rows do not cover M=%d", r.split, r.rows_per_split, p.M);
  p.rows_per_split = r.rows_per_split; p.tilesN = r.tilesN; p.gx = r.gx; p.xcd = r.xcd; p.debug = r.debug;
  {   // buffer addressing: a block's operands are reached through 32-bit offsets from the first row / frame of its split
    const long long lim = 0x7FFFF000LL;
    const long long a_span = (long long)p.rows_per_split * p.Co * esz;
    const long long frames = (long long)p.rows_per_split / ((long long)p.Ho * p.Wo) + 2;
    const long long b_span = p.simple_rows ? (long long)p.rows_per_split * p.Ci * esz : frames * p.Hi * p.Wi * p.Ci * esz;
    R3M_REQUIRE(a_span < lim && b_span < lim, "wgrad: one split spans %lld / %lld bytes (limit 2 GiB): raise splitK (%d)", a_span, b_span, r.split);
  }
  prof_begin(wg_wide(p.Co, p.Ci) ? KC_WGRAD_WIDE : KC_WGRAD_NARROW, 2.0 * (double)p.M * (double)p.Co * (double)T * p.Ci, p.M, p.Co, p.Ci, T, s);
  const char* what = "wgrad";
  switch (r.route) {
    case WG_TAPS_SIMPLE: launch_wgrad_glds<32, 1, 1>(p, r, s); break;
    case WG_TAPS_GATHER: launch_wgrad_glds<32, 1, 0>(p, r, s); break;
    case WG_ROWS:        launch_wgrad_glds<16, 3, 0>(p, r, s); break;
    case WG_WINDOW:      if (int e = launch_wgrad_rowwin(p, r, s)) return e; break;
    case WG16_TAPS:      what = "wgrad_bf16"; if (int e = launch_wgrad_bf16(p, r, s)) return e; break;
    case WG16_ROWS:      what = "wgrad_bf16 (kernel rows)"; if (int e = launch_wgrad_bf16(p, r, s)) return e; break;
    case WG16_ALL_TAPS:  what = "wgrad3x3_halo_bf16"; if (int e = launch_wgrad_bf16(p, r, s)) return e; break;
    default: R3M_REQUIRE(false, "wgrad: route %d", r.route);
  }
  if (prof_open()) {   // dY, the input pixels some (output pixel, tap) pair reads (a 1x1 / stride-2 layer: a quarter), the split-K slabs
    const auto read = [&](int n_in, int n_out, int k) {
      int n = 0;
      for (int i = 0; i < n_in; ++i) {
        bool hit = false;
        for (int kk = 0; kk < k && !hit; ++kk) {
          const int o = i + p.pad - kk;
          hit = o >= 0 && o % p.stride == 0 && o / p.stride < n_out;
        }
        n += hit;
      }
      return n;
    };
    const double x = (double)p.N * read(p.Hi, p.Ho, p.KH) * read(p.Wi, p.Wo, p.KW) * p.Ci;
    prof_bytes((double)esz * ((double)p.M * p.Co + x) + 4.0 * (double)r.split * p.Co * T * p.Ci);
  }
  prof_end(s);
  return check_launch(what);
}

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
