// r3m_amd — bf16-activation weight gradients for gfx950 (the wgrad side of the bf16 path; forward / dgrad: conv_bf16.hip): bf16 dY and
// X in HBM/LDS, fp32 accumulation on v_mfma_f32_32x32x16_bf16, fp32 split-K partials (reduced by wgrad.hip's launch_wgrad_reduce).
//
//   wgrad_bf16_kernel : the contraction runs over rows m while both operands are channel-contiguous, i.e. K-strided in
//       LDS. gfx950's transpose read (ds_read_b64_tr_b16) turns a [4 k][16 channel] LDS block into 4 consecutive k per
//       lane, so the operands still arrive by plain row DMA and no packing VALU is spent. 64-byte channel groups are
//       XOR-swizzled by the k row so the 4 rows one read touches sit in 4 different bank quarters.
//       One tap per block, or (NT = 3) the three taps of a kernel row.
//   wgrad3x3_halo_bf16_kernel : 3x3 / stride 1 / pad 1 at image widths that are multiples of 8: all nine taps per block from one
//       staged X window.
// Which of the three a launch runs, its tile, K step, split and grid: wgrad_plan (wgrad.hip), the one dispatch of the weight-gradient
// family. launch_wgrad_bf16 only launches the instantiation the plan names. Shared device code: wgrad_dev.h.
#include "wgrad_dev.h"

namespace r3m {

typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __attribute__((aligned(256))) unsigned char g_zero_bytes[512];

__device__ __forceinline__ const char* sel_ptr(const char* s, const char* z, bool ok) {
  // bitwise select keeps the loader straight-line (a ?: is turned back into an exec-masked branch)
  const unsigned long long msk = ok ? ~0ull : 0ull;
  return reinterpret_cast<const char*>((reinterpret_cast<unsigned long long>(s) & msk) |
                                       (reinterpret_cast<unsigned long long>(z) & ~msk));
}

__device__ __forceinline__ void dma16(const char* src, unsigned char* lds) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}

// =====================================================================================================
// wgrad on bf16 operands: dW[co, tap, ci] (fp32 split-K partials) = sum_m dY[m, co] * X[pix(m) + off(tap), ci].
// Block tile BMt (co) x BNt (ci), K step 64 rows, 4 waves as 2 x 2. LDS image per operand: [64 k][BMt] bf16, a k row is
// BMt*2 bytes, one DMA instruction covers 1 KiB = 4 (128 wide) or 8 (64 wide) k rows. 64-byte channel groups are
// XOR-swizzled with the k row (on the DMA's global source side and again on the fragment read).
// Fragment of MFMA step s, half r: ds_read_b64_tr_b16 — in each 16-lane group lane c returns element (c & 3) of what
// lane 4j + (c >> 2) addressed, for j = 0..3. With lane q = 4j + i addressing k row kb + j, channels cb + 4i..4i+3, lane c
// receives channel cb + c at k = kb..kb+3: four consecutive k of one channel — half an MFMA operand.
// =====================================================================================================
// NT = 3 (round 3, "kernel-row" blocks of a 3-wide kernel): one block owns the THREE taps (kh, 0..2) of one kernel row for its
// (co, ci) tile — three accumulator sets (192 registers on the 128 x 128 tile). The dY tile of a K step is staged ONCE and its
// fragments are read ONCE for the three taps, the (oy, ox) walk of the staged X rows is shared (the taps differ by one pixel
// in x), and each tap still stages its own exactly-masked X rows (no register masks, any width / stride). Per tap this is 2/3 of
// the L2 -> LDS bytes (the bf16 128 x 128 tile needs ~39 TB/s of that path at the matrix peak; the chip delivers ~17), 2/3 of
// the DMA instructions and 2/3 of the LDS fragment reads of the per-tap form.
// FAST = 1: wgrad_plan has checked (plan.fast) that one K step advances a row by less than one frame ((BK / Wo + 1) <= Ho — every layer of
// the networks here), so the division form of the coordinate walk is not even compiled in (registers, code size).
template <int BMt, int BNt, int BK = 64, int NT = 1, int FAST = 0>   // BK = rows per K step: 64, or 32 (half the LDS: more blocks per CU)
__global__ __launch_bounds__(256, NT == 3 ? 2 : 1) void wgrad_bf16_kernel(const WgradParams p) {
  static_assert(BK == 64 || BK == 32, "K step of 64 or 32 rows");
  static_assert(NT == 1 || NT == 3, "one tap, or the three taps of a kernel row");
  const bool simple_rows = NT == 1 && p.simple_rows;           // a kernel-row block (NT = 3) never has 1x1 "simple" rows
  constexpr int WR = BK / 4;                                   // k rows staged per wave per stage
  constexpr int TM = BMt / 64, TN = BNt / 64;
  constexpr int A_ROWB = BMt * 2, B_ROWB = BNt * 2;            // bytes per k row
  constexpr int A_RPI = 1024 / A_ROWB, B_RPI = 1024 / B_ROWB;  // k rows per DMA instruction
  constexpr int AJ = WR / A_RPI, BJ = WR / B_RPI;              // instructions per wave per stage (per tap for B)
  constexpr int NP = AJ + BJ;                                  // piece GROUPS: a B group issues NT instructions
  constexpr int B_TILE = BK * B_ROWB;
  constexpr int STAGE = BK * A_ROWB + NT * B_TILE;
  __shared__ __attribute__((aligned(256))) unsigned char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int T = p.KH * p.KW;
  const WgBlock blk = wg_block<BMt, BNt, false>(p, T / NT);    // tap groups per tile (NT = 3: kernel rows)
  const int tap0 = blk.grp * NT;
  const int co0 = blk.co0, ci0 = blk.ci0, ms = blk.ms, me = blk.me;
  const int kh = tap0 / p.KW, kw0 = tap0 - kh * p.KW;
  const int hw = p.Ho * p.Wo;
  const char* Xb = reinterpret_cast<const char*>(p.X);

  // swizzle key of a k row: 4 consecutive rows must land in 4 different 64-byte bank quarters
  //   128 wide (256-byte rows): key = row & 3;   64 wide (128-byte rows, two per bank line): key = (row >> 1) & 1
  // DMA lane -> (k row within the instruction, physical 16-byte slot) -> logical slot = physical ^ 4*key
  const int a_k = lane / (A_ROWB / 16), a_ps = lane % (A_ROWB / 16);
  const int b_k = lane / (B_ROWB / 16), b_ps = lane % (B_ROWB / 16);
  const int a_key = (BMt == 128) ? (a_k & 3) : ((a_k >> 1) & 1);
  const int b_key = (BNt == 128) ? (b_k & 3) : ((b_k >> 1) & 1);
  // Round 3: LDS DMA through buffer descriptors (conv_dev.h, buf_dma16). PMC on the ResNet-34 3x3 layers showed this kernel
  // ISSUE-bound, not bandwidth-bound: 6.8 vector instructions per MFMA (the per-lane 64-bit source pointers of global_load_lds:
  // 64-bit multiply-adds, pointer selects, a 64-bit advance per piece), waves 28 % issuing / 35 % stalled on dependent VALU / 37 %
  // parked, matrix pipe busy 0.37. With a descriptor the per-lane part is a 32-bit byte offset and out-of-range lanes read zeros:
  //   dY (and X of 1x1 stride-1 layers): CONSTANT per-lane offsets, the descriptor advances one K step on the scalar unit and
  //     rows past the split fall off its end — no vector instruction per piece;
  //   X of 3x3 / strided layers: per-lane (oy, ox, frame offset) walk in 32-bit arithmetic, padding taps get an out-of-range
  //     offset; rows past the split need no test (their dY rows are zeros).
  const unsigned a_chan = (unsigned)((co0 + (a_ps ^ (4 * a_key)) * 8) * 2);   // byte offset of this lane's 8 channels inside a dY row
  const unsigned b_chan = (unsigned)((ci0 + (b_ps ^ (4 * b_key)) * 8) * 2);

  WgRows a = wg_rows<2>(p.dY, ms, me, p.Co, 0, BK);             // descriptor: rows [ms + BK * step, me) of dY, whole rows
  unsigned a_voff[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) a_voff[j] = (unsigned)((wave * WR + j * A_RPI + a_k) * p.Co * 2) + a_chan;

  const int q64 = BK / p.Wo, r64 = BK - q64 * p.Wo;          // (oy, ox) advance of one K step
  const bool fast_adv = FAST || (q64 + 1) <= p.Ho;
  const long long img = (long long)p.Hi * p.Wi * p.Ci * 2;
  const unsigned imgb = (unsigned)img;
  const int n0 = ms / hw;                                     // 3x3 / strided: offsets are relative to the split's first frame
  WgRows b;
  b.base = simple_rows ? Xb + (long long)ms * p.Ci * 2 : Xb + (long long)n0 * img;
  {
    const long long rest = simple_rows ? (long long)(me - ms) * p.Ci * 2 : (long long)(p.N - n0) * img;
    b.left = rest < (long long)BUF_OOB ? (int)rest : (int)BUF_OOB;
  }
  b.stepb = BK * p.Ci * 2;
  const int pixb = p.Ci * 2;                                    // bytes between the X rows of neighbouring taps (one pixel)
  const int rowb = p.Wi * pixb;
  const int kh_p = kh - p.pad, kw_p = kw0 - p.pad;
  // 3x3 / strided layers: a lane tracks the INPUT coordinates of its row's output pixel (ys = oy * stride, xs = ox * stride) and
  // their byte position pos = ys * rowb + xs * pixb by additions only (a K step advances (oy, ox) by a block-uniform amount),
  // so there is no integer multiply in the K loop (v_mul_lo_u32 issues at a quarter of the rate: four per piece were ~60 cycles).
  const int xs_wrap = p.Wo * p.stride, ys_wrap = p.Ho * p.stride;
  const int adv_xs = r64 * p.stride, adv_ys = q64 * p.stride;
  const int adv_pos = adv_ys * rowb + adv_xs * pixb;
  const int wrapx_pos = p.stride * rowb - xs_wrap * pixb;       // ox wrapped: one output row down, Wo pixels back
  const int wrapy_pos = ys_wrap * rowb;                         // oy wrapped: next frame (b_off carries the frame)
  const int tap_pos = kh_p * rowb + kw_p * pixb;
  int b_m[BJ];
  unsigned b_off[BJ];      // simple rows: constant per-lane offset; otherwise byte offset of the row's frame from b_base (+ channels)
  int ys[BJ], xs[BJ], pos[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    b_m[j] = ms + wave * WR + j * B_RPI + b_k;
    ys[j] = 0; xs[j] = 0; pos[j] = 0;
    if (simple_rows) {
      b_off[j] = (unsigned)((wave * WR + j * B_RPI + b_k) * p.Ci * 2) + b_chan;
    } else {
      const int n = b_m[j] / hw;
      const int rem = b_m[j] - n * hw;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      ys[j] = oy * p.stride; xs[j] = ox * p.stride;
      pos[j] = ys[j] * rowb + xs[j] * pixb;
      b_off[j] = (unsigned)(n - n0) * imgb + b_chan;
    }
  }

  // NT = 3 runs at the register limit: there the descriptor words are pinned to scalar registers (conv_dev.h buf_dma16_uniform)
  auto dma = [&](const char* base, int bytes, unsigned char* lds, unsigned voff) __attribute__((always_inline)) {
    if constexpr (NT == 3) buf_dma16_uniform(base, bytes, lds, voff);
    else buf_dma16(base, bytes, lds, voff);
  };
  auto issue_piece = [&](int stage, auto pc_c) __attribute__((always_inline)) {
    constexpr int pc = decltype(pc_c)::value;
    if constexpr (pc < AJ) {
      constexpr int j = pc;
      unsigned char* la = smem + stage * STAGE + (wave * WR + j * A_RPI) * A_ROWB;
      dma(a.base, a.left, la, a_voff[j]);
    } else {
      constexpr int j = pc - AJ;
      unsigned char* lb = smem + stage * STAGE + BK * A_ROWB + (wave * WR + j * B_RPI) * B_ROWB;
      if (simple_rows) {
        dma(b.base, b.left, lb, b_off[j]);
      } else {
        const int iy = ys[j] + kh_p, ix0 = xs[j] + kw_p;
        const bool rowok = (unsigned)iy < (unsigned)p.Hi;
        const unsigned off0 = b_off[j] + (unsigned)(pos[j] + tap_pos);           // garbage when the tap is padding: not used then
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const bool in = rowok && ((unsigned)(ix0 + t) < (unsigned)p.Wi);
          dma(b.base, b.left, lb + t * B_TILE, in ? off0 + (unsigned)(t * pixb) : BUF_OOB);
        }
        if (FAST || fast_adv) {
          int x = xs[j] + adv_xs, y = ys[j] + adv_ys, ps = pos[j] + adv_pos;
          const bool cx = x >= xs_wrap;
          x = cx ? x - xs_wrap : x;
          y = cx ? y + p.stride : y;
          ps = cx ? ps + wrapx_pos : ps;
          const bool cy = y >= ys_wrap;
          y = cy ? y - ys_wrap : y;
          ps = cy ? ps - wrapy_pos : ps;
          b_off[j] = cy ? b_off[j] + imgb : b_off[j];
          xs[j] = x; ys[j] = y; pos[j] = ps;
        } else if constexpr (!FAST) {
          b_m[j] += BK;
          const int n = b_m[j] / hw;
          const int rem = b_m[j] - n * hw;
          const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
          ys[j] = oy * p.stride; xs[j] = ox * p.stride;
          pos[j] = ys[j] * rowb + xs[j] * pixb;
          b_off[j] = (unsigned)(n - n0) * imgb + b_chan;
        }
      }
    }
    if constexpr (pc == NP - 1) {             // after the last piece of a K step: the linear descriptors move on (scalar unit)
      a.advance();
      if (simple_rows) b.advance();
    }
  };

  f32x16 acc[NT][TM][TN];
  wg_clear(acc);

  // transpose-read addressing. Lane l: group-local q = l & 15 addresses k row 8*(l>>5) + (q>>2) (+16s + 4r as an immediate),
  // channels [16*((l>>4)&1) + 4*(q&3), +4) of its MFMA tile; the tile's 64-byte group index is XORed with the row key.
  const int q = lane & 15;
  const int frow = 8 * (lane >> 5) + (q >> 2);
  const int fkeyA = (BMt == 128) ? (frow & 3) : ((frow >> 1) & 1);
  const int fkeyB = (BNt == 128) ? (frow & 3) : ((frow >> 1) & 1);
  const int fcol = (16 * ((lane >> 4) & 1) + 4 * (q & 3)) * 2;       // byte offset inside the tile's 64-byte group
  int fa_off[TM], fb_off[TN];
#pragma unroll
  for (int t = 0; t < TM; ++t) fa_off[t] = frow * A_ROWB + (((wm * TM + t) ^ fkeyA) * 64) + fcol;
#pragma unroll
  for (int t = 0; t < TN; ++t) fb_off[t] = BK * A_ROWB + frow * B_ROWB + (((wn * TN + t) ^ fkeyB) * 64) + fcol;

  auto tr_read = [&](const unsigned char* ptr) __attribute__((always_inline)) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)ptr);
  };
  auto frag = [&](const unsigned char* base, int rowb, int sidx) __attribute__((always_inline)) {
    const s16x4 lo = tr_read(base + (16 * sidx) * rowb);
    const s16x4 hi = tr_read(base + (16 * sidx + 4) * rowb);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
  };

  auto mfma_stage = [&](const unsigned char* st, int dma_stage) __attribute__((always_inline)) {
    // the next K step's DMA: all pieces right after the barrier
    if (dma_stage >= 0) static_for<NP>([&](auto pc) __attribute__((always_inline)) { issue_piece(dma_stage, pc); });
    static_for<BK / 16>([&](auto s_c) __attribute__((always_inline)) {
      constexpr int sidx = decltype(s_c)::value;
      bf16x8 a[TM];
#pragma unroll
      for (int t = 0; t < TM; ++t) a[t] = frag(st + fa_off[t], A_ROWB, sidx);
#pragma unroll
      for (int tp = 0; tp < NT; ++tp) {
        bf16x8 b[TN];
#pragma unroll
        for (int t = 0; t < TN; ++t) b[t] = frag(st + tp * B_TILE + fb_off[t], B_ROWB, sidx);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tp][tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[tm], b[tn], acc[tp][tm][tn], 0, 0, 0);
      }
    });
  };

  const int nk = (me - ms + BK - 1) / BK;
  if (nk > 0) static_for<NP>([&](auto pc) __attribute__((always_inline)) { issue_piece(0, pc); });
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    mfma_stage(smem + cur * STAGE, (kt + 1 < nk) ? (cur ^ 1) : -1);
  }

  wg_store<false, false>(p, blk, T, tap0, wm, wn, lane & 31, lane >> 5, acc);
}

// =====================================================================================================
// 3x3 / stride 1 / pad 1 weight gradient with ALL NINE TAPS per block: dW[co, tap, ci] = sum_m dY[m, co] * X[m + shift(tap), ci].
// The per-tap kernel above stages a dY tile and an X tile for every tap (18 rows per contraction row); here a K step of 64
// pixels stages the dY rows once and ONE X window of 64 + 2W + 2 rows that all taps read at their row shift (3.9 rows per
// contraction row at 56x56, 2.5 at 14x14). Block = one 64 (co) x 64 (ci) tile x 9 taps, four waves of 32 x 32 x 9 (144
// accumulator registers per lane), split-K partials as before.
// The border rule varies ALONG the contraction (a pixel at x = 0 has no left neighbour: dx = -1 drops pixels with x = 0, dx = +1
// those with x = W-1, dy = -1 / +1 those with y = 0 / H-1; rows of other frames inside the window are exactly those the dy masks
// remove), so it cannot be a row redirect as in the forward halo kernel — the X fragments are masked in registers. A wave issues
// one instruction per 4 cycles whatever its kind, so the budget is ~135 instructions per k group (9 MFMAs): general per-element
// masks (8-bit drop masks expanded to 16-bit lanes: 550 instructions, even on the scalar unit) ran at 390 TFLOP/s. Restricted to
// image widths that are multiples of 8 the masks collapse to "element 0", "element 7" and "all" per lane half (see below).
// =====================================================================================================
__global__ __launch_bounds__(256, 2) void wgrad3x3_halo_bf16_kernel(const WgradParams p, const int xri) {
  constexpr int BK = 64;
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];
  const int stage_bytes = BK * 128 + xri * 1024;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const WgBlock blk = wg_block<64, 64, false>(p, 1);   // one block per tile: all nine taps
  const int co0 = blk.co0, ci0 = blk.ci0, ms = blk.ms, me = blk.me;
  const int W = p.Wi, H = p.Hi;
  const char* dYb = reinterpret_cast<const char*>(p.dY);
  const char* Xb = reinterpret_cast<const char*>(p.X);

  // DMA lane -> (k row within the instruction, physical 16-byte slot); logical slot = physical ^ 4 * key, key = (row >> 1) & 1
  const int d_k = lane >> 3, d_ps = lane & 7;
  const int d_key = (d_k >> 1) & 1;
  const int a_cb = (co0 + (d_ps ^ (4 * d_key)) * 8) * 2;
  const int b_cb = (ci0 + (d_ps ^ (4 * d_key)) * 8) * 2;
  const char* zl = reinterpret_cast<const char*>(g_zero_bytes) + (lane & 15) * 16;
  int a_m[2];
  const char* a_ptr[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    a_m[j] = ms + wave * 16 + j * 8 + d_k;
    a_ptr[j] = dYb + (long long)a_m[j] * p.Co * 2 + a_cb;
  }
  const long long a_step = (long long)BK * p.Co * 2;
  auto issue = [&](int stage, int mk) __attribute__((always_inline)) {
    unsigned char* st = smem + stage * stage_bytes;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      dma16(sel_ptr(a_ptr[j], zl, a_m[j] < me), st + (wave * 16 + j * 8) * 128);
      a_m[j] += BK;
      a_ptr[j] += a_step;
    }
    for (int i = wave; i < xri; i += 4) {
      const long long q = (long long)mk - (W + 1) + 8 * i + d_k;
      const bool in = q >= 0 && q < (long long)p.M;
      const char* src = Xb + ((in ? q : 0) * p.Ci) * 2 + b_cb;
      dma16(sel_ptr(src, zl, in), st + BK * 128 + i * 1024);
    }
  };

  f32x16 acc[9][1][1];       // (cleared here: wg_clear together with wg_store costs this kernel 15 registers and 352 bytes of scratch)
#pragma unroll
  for (int a = 0; a < 9; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][0][0][r] = 0.f;

  // transpose-read addressing (see wgrad_bf16_kernel): lane -> k row 8*(lane>>5) + (q>>2), 4 channels of its 32-channel group
  const int q16 = lane & 15;
  const int frow = 8 * (lane >> 5) + (q16 >> 2);
  const int fcol = (16 * ((lane >> 4) & 1) + 4 * (q16 & 3)) * 2;
  const int fa_off = frow * 128 + ((wm ^ ((frow >> 1) & 1)) * 64) + fcol;
  int fb_off[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int rowb = frow + (W + 1) + (t / 3 - 1) * W + (t % 3 - 1);       // window row of this lane's first k row at tap t
    fb_off[t] = BK * 128 + rowb * 128 + ((wn ^ ((rowb >> 1) & 1)) * 64) + fcol;
  }
  auto tr_read = [&](const unsigned char* ptr) __attribute__((always_inline)) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)ptr);
  };
  auto frag = [&](const unsigned char* base, int sidx) __attribute__((always_inline)) {
    const s16x4 lo = tr_read(base + (16 * sidx) * 128);
    const s16x4 hi = tr_read(base + (16 * sidx + 4) * 128);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
  };

  // image coordinates of the first pixel of the K step (pixel ms + kt*64): block-uniform, kept in scalar registers
  const int invW = 65536 / W + 1;                       // (v * invW) >> 16 == v / W for v < 4096
  int ox, oy;
  {
    const int row = ms / W;
    ox = __builtin_amdgcn_readfirstlane(ms - row * W);
    oy = __builtin_amdgcn_readfirstlane(row % H);
  }
  const int adv_q = BK / W, adv_r = BK - adv_q * W;
  const bool hi_half = lane >= 32;

  const int nk = (me - ms + BK - 1) / BK;
  if (nk > 0) issue(0, ms);
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) issue(cur ^ 1, ms + (kt + 1) * BK);
    const unsigned char* st = smem + cur * stage_bytes;
    static_for<4>([&](auto s_c) __attribute__((always_inline)) {
      constexpr int sidx = decltype(s_c)::value;
      const bf16x8 a = frag(st + fa_off, sidx);
      // Border masks. W and H*W are multiples of 8 (launcher) and K steps start at multiples of 64 pixels, so the 8 consecutive
      // pixels a lane half holds never straddle an image row: x = 0 can only be its element 0, x = W-1 only its element 7, and
      // the first / last image row covers the run entirely or not at all. Four flags per half on the scalar unit, four per-lane
      // mask dwords, at most four ANDs per tap.
      typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
      unsigned sL[2], sR[2], sT[2], sB[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int xs = ox + 16 * sidx + 8 * h, ys = oy;
        const int qd = (xs * invW) >> 16;
        xs -= qd * W;
        ys += qd;
        ys = ys >= H ? ys - H : ys;     // qd <= 7 (W >= 8, 64-pixel K steps) and H >= 4 (launcher): two wraps cover oy + qd < 3 H
        ys = ys >= H ? ys - H : ys;
        sL[h] = xs == 0 ? 0xffff0000u : 0xffffffffu;          // drop element 0 (left neighbour of x = 0)
        sR[h] = xs + 8 == W ? 0x0000ffffu : 0xffffffffu;      // drop element 7 (right neighbour of x = W-1)
        sT[h] = ys == 0 ? 0u : 0xffffffffu;                   // first image row: nothing above
        sB[h] = ys == H - 1 ? 0u : 0xffffffffu;               // last image row: nothing below
      }
      const unsigned mL = hi_half ? sL[1] : sL[0], mR = hi_half ? sR[1] : sR[0];
      const unsigned mT = hi_half ? sT[1] : sT[0], mB = hi_half ? sB[1] : sB[0];
      static_for<9>([&](auto t_c) __attribute__((always_inline)) {
        constexpr int t = decltype(t_c)::value;
        constexpr int kh = t / 3, kw = t % 3;
        u32x4_t u = __builtin_bit_cast(u32x4_t, frag(st + fb_off[t], sidx));
        if constexpr (kh != 1) {
          const unsigned my = kh == 0 ? mT : mB;
          u[0] &= (kw == 0 ? (my & mL) : my);
          u[1] &= my;
          u[2] &= my;
          u[3] &= (kw == 2 ? (my & mR) : my);
        } else {
          if constexpr (kw == 0) u[0] &= mL;
          if constexpr (kw == 2) u[3] &= mR;
        }
        acc[t][0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, u), acc[t][0][0], 0, 0, 0);
      });
    });
    // next K step: 64 pixels further
    ox += adv_r;
    oy += adv_q;
    if (ox >= W) { ox -= W; ++oy; }
    while (oy >= H) oy -= H;
  }

  wg_store<false, false>(p, blk, 9, 0, wm, wn, lane & 31, lane >> 5, acc);
}

// 3x3 stride-1 weight gradients at image widths that are multiples of 8 go through the all-taps kernel (56x56 x 64 channels at
// 1280 frames: 0.834 -> 0.470 ms; ResNet-50 step -1.1 %, ResNet-34 -4.2 %): 56 x 56 is where the 64-channel layers are, and where the
// per-tap kernel is furthest from its roof
int wgrad_halo_lds_bytes(int W) { return 2 * (64 * 128 + ceil_div(64 + 2 * W + 2, 8) * 1024); }
bool wgrad_halo_eligible(const WgradParams& p) {
  return p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Ho == p.Hi && p.Wo == p.Wi && (p.Wi & 7) == 0 && p.Wi >= 8 &&
         p.Hi >= 4 && p.Wi <= 1024 && wgrad_halo_lds_bytes(p.Wi) <= 80 * 1024;
}

// Launches the instantiation the plan names: all nine taps per block on the 64 x 64 tile, one block per kernel row (round 3: 3-wide
// kernels on the 128 x 128 tile, three taps, dY staged and read once — ResNet-34's 128 / 256 / 512-channel 3x3 layers, stride 1 and
// 2), or one block per tap (128 x 128 tile with K steps of 32 rows, 64 x 64 with 64).
int launch_wgrad_bf16(const WgradParams& p, const WgradPlan& r, hipStream_t s) {
  const dim3 grid(r.gx * r.split);
  if (r.route == WG16_ALL_TAPS) {
    static DynLdsOptIn optin;
    if (int e = ensure_dyn_lds(optin, reinterpret_cast<const void*>(wgrad3x3_halo_bf16_kernel), r.lds_bytes, "wgrad3x3_halo(bf16)")) return e;
    hipLaunchKernelGGL(wgrad3x3_halo_bf16_kernel, grid, dim3(256), r.lds_bytes, s, p, ceil_div(64 + 2 * p.Wi + 2, 8));
  } else if (r.route == WG16_ROWS) {
    if (r.fast) hipLaunchKernelGGL((wgrad_bf16_kernel<128, 128, 32, 3, 1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((wgrad_bf16_kernel<128, 128, 32, 3>), grid, dim3(256), 0, s, p);
  } else if (r.tile == 128) {
    hipLaunchKernelGGL((wgrad_bf16_kernel<128, 128, 32>), grid, dim3(256), 0, s, p);
  } else {
    hipLaunchKernelGGL((wgrad_bf16_kernel<64, 64>), grid, dim3(256), 0, s, p);
  }
  return 0;
}

}  // namespace r3m
