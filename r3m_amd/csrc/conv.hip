// r3m_amd — fp32 forward / input-gradient convolutions for gfx950 (MI355X): NHWC implicit GEMM on the f32-input MFMA
// (v_mfma_f32_32x32x2_f32, exact fp32 == fmaf chain), LDS-staged operand tiles, XCD-aware block order.
//
// Replaces what the reference reaches through torchvision's ResNet -> ATen conv2d / cuDNN (r3m/models/models_r3m.py): forward and
// dgrad of every 1x1 / 3x3 convolution of ResNet-18/34/50 behind the stem, plus nn.Linear of the language reward head
// (r3m/models/models_language.py), which is the same GEMM with a bias epilogue.
//
//   gather-GEMM : out[m, n] = sum_{tap, c} in[pix(m) + off(tap), c] * W[n, tap, c]
//     forward conv (taps = kh,kw; input stride = conv stride), dgrad (taps flipped; stride-2 dgrad is run as 4 output-parity
//     classes so no MFMA work is spent on structural zeros), Linear (1 tap).
//     Epilogues (conv_dev.h gg_epilogue): raw store (+ BatchNorm sum / sum-of-squares partials), accumulate, masked
//     residual-gradient add, bias (+ReLU), ReLU-mask, BatchNorm-backward partials; the window kernel also eval-mode BatchNorm.
//
// launch_gather_gemm = requirements -> gg_prepare (packed taps) -> gg_route (a pure function of the launch) -> switch (route).
// Tiles are 128 x 128 ("wide": Nc a multiple of 128) or 256 x 64. Route numbers are public (r3m_debug_conv_route):
//    1      conv3x3_win_kernel        3x3 / stride 1 / pad 1, wide, W <= 28: the 128- to 512-channel 3x3 layers, forward and dgrad
//   11-13   conv_pw.hip               persistent kernel (pointwise / gather / strided output rows): every other ResNet launch whose
//                                     channel counts are multiples of 64 — the 1x1 layers, the 64-channel and wider-than-28 3x3 layers,
//                                     the stride-2 layers and their parity-class dgrads
//   20      gather_gemm_k16_kernel    wide, one tap, K <= 256, N >= 2 K, where the persistent kernel does not apply: Ci = 32 / 96 / 160 / 224,
//                                     an epilogue it does not build (bias of a Linear), a 1x1 / stride-2 downsample whose output map is
//                                     under 2 rows x 4 columns (frames near 32 x 32)
//   21      gather_gemm_glds2_kernel  every other launch with Ci/32 even, Ci <= 2048; wide <128,128,2,2> or narrow <256,64,4,1>: 3x3 layers on
//                                     maps under 2 x 4 outputs, the 128-wide dgrad with residual join + BatchNorm partials on maps wider than
//                                     28, the Linear layers
//   22      gg_other_kernel():        odd Ci/32 or Ci > 2048 — r3m_conv2d_* / r3m_linear_* and the fuzz tests on 96- and 160-channel sides
//             gather_gemm_glds_kernel             wide
//             gather_gemm_kernel<256,64,4,1>      narrow (global -> VGPR -> LDS, 36-float padded rows)
//             gather_gemm_kernel<128,128,2,2>     probe builds with R3M_GG_GLDS=0 (A/B of the register-staged predecessor)
//   30-33   conv_bf16.hip gg16_route  bf16 plans, handed to launch_gather_gemm_bf16 before any fp32 requirement: 30 gather_gemm_bf16_kernel,
//                                     31 conv3x3_halo_bf16_kernel, 32 conv_row16.hip (kernel rows), 33 conv_pw16.hip (probe builds)
// Also here: the dgrad weight transposes (transpose_w_kernel, transpose_w_all_kernel) and debug_occupancy.
// The weight gradients are in wgrad.hip / wgrad_win.hip (bf16: wgrad_bf16.hip), the 224 x 224 stem in stem.hip.
//
// All staging is branch-free: taps that fall outside the image and rows past the end read a valid dummy address (a
// zero line / a clamped pixel) instead of being skipped, so the loader is straight-line code the compiler can interleave
// with the MFMA stream; the tap table is a dword array in the kernarg segment (scalar loads).
#include "common.h"
#include "conv_dev.h"
#include <utility>
#include <vector>

namespace r3m {

__device__ __attribute__((aligned(128))) float g_zero_line[2048 + 64];


// =====================================================================================================
// gather-GEMM, direct-to-LDS staging (the 128x128 work-horse).
// Block 128 x 128, K step 32, 4 waves as 2 x 2, each wave 64 x 64 = 2 x 2 MFMA tiles of 32x32.
// LDS: two stages of {A[128][32], B[128][32]} floats, rows of exactly 128 B (what global_load_lds needs: the 64 lanes
// of one instruction land at base + lane*16, i.e. 8 consecutive rows), 16-byte slots XOR-swizzled by ((row>>1)&7): the
// swizzle is applied to the per-lane GLOBAL source address and again on the fragment read, never to the LDS
// destination. With it the ds_read_b128 fragment reads (16-lane groups, rows distinct mod 16) are conflict-free.
// Fragments: lane half h = lane>>5 reads k = 8g+4h..+3 of group g; MFMA step j contracts k = {8g+j, 8g+4+j} — A and B use
// the same permutation of k, the sum is unchanged.
// Pipeline: tile t+1's DMA is issued right after the barrier that publishes tile t and lands during tile t's 64 MFMAs
// per wave; one barrier per K step, no staging registers, no ds_write instructions.
// =====================================================================================================
template <int EPI>
__global__ __launch_bounds__(256) void gather_gemm_glds_kernel(const GatherGemmParams p) {
  constexpr int BM = 128, BN = 128, WM = 2, WN = 2, TM = 2, TN = 2;
  constexpr int STAGE = (BM + BN) * 32;                   // floats per stage (32 KiB)
  __shared__ __attribute__((aligned(128))) float smem[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int gridN = (p.Nc + BN - 1) / BN;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = lid / gridN, nt = lid % gridN;  // column tiles of one row panel are neighbours -> same XCD L2
  const int m0 = mt * BM, n0 = nt * BN;

  // staging: wave w fills rows [32w, 32w+32) of A and of B, 8 rows (1 KiB) per instruction
  const int srow = lane >> 3;          // row within the 8-row group
  const int pslot = lane & 7;          // physical 16-byte slot written by this lane
  const int Hb = p.simple_rows ? 1 : p.Hi, Wb = p.simple_rows ? 1 : p.Wi;
  RowDesc ad[4];
  int acol[4];                         // logical k offset (floats) this lane fetches for A/B row group j
  unsigned arow_ok = 0;
  long long bbase[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = wave * 32 + j * 8 + srow;                 // row inside the tile
    acol[j] = (pslot ^ ((r >> 1) & 7)) * 4;
    const int m = m0 + r;
    ad[j] = decode_row(p, m);
    if (m < p.M) arow_ok |= 1u << j;
    const int n = min(n0 + r, p.Nc - 1);                    // columns past Nc are computed on a clamped row, never stored
    bbase[j] = (long long)n * p.T * p.Ci;
  }
  const float* zline = g_zero_line + pslot * 4;

  const int kpt = p.Ci >> 5;          // K tiles per tap
  const int nk = p.ntaps * kpt;

  auto issue_tile = [&](int pack, int chunk, int stage) {
    const int dy = (pack << 24) >> 24, dx = (pack << 16) >> 24, wt = pack >> 16;
    const int c0 = chunk * 32;
    const long long woff = (long long)wt * p.Ci + c0;
    float* la = smem + stage * STAGE + wave * 32 * 32;
    float* lb = la + BM * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int iy = ad[j].iy + dy, ix = ad[j].ix + dx;
      const bool in = ((unsigned)iy < (unsigned)Hb) && ((unsigned)ix < (unsigned)Wb) && ((arow_ok >> j) & 1u);
      const int iyc = min(max(iy, 0), Hb - 1), ixc = min(max(ix, 0), Wb - 1);
      const float* src = p.A + ad[j].base + ((long long)iyc * p.Wi + ixc) * p.Ci + c0 + acol[j];
      // bitwise select keeps the loader straight-line (a ?: here is turned back into an exec-masked branch)
      const unsigned long long msk = in ? ~0ull : 0ull;
      src = reinterpret_cast<const float*>((reinterpret_cast<unsigned long long>(src) & msk) |
                                           (reinterpret_cast<unsigned long long>(zline) & ~msk));
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(la + j * 8 * 32), 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* src = p.B + bbase[j] + woff + acol[j];
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(lb + j * 8 * 32), 16, 0, 0);
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // fragment addressing: row = lrow (+32 per MFMA tile), logical slot 2g+h, physical slot = logical ^ ((row>>1)&7)
  const int lrow = lane & 31, lh = lane >> 5;
  const int xr = (lrow >> 1) & 7;
  int goff[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) goff[g] = ((2 * g + lh) ^ xr) * 4;
  const float* fragA0 = smem + (wm * 64 + lrow) * 32;
  const float* fragB0 = smem + BM * 32 + (wn * 64 + lrow) * 32;

  int tap_n = 0, chunk_n = 0;
  int pack_cur = nk > 0 ? p.tap[0] : 0;
  int pack_next = p.ntaps > 1 ? p.tap[1] : pack_cur;
  if (nk > 0) issue_tile(pack_cur, 0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = (R3M_PROBE(p) == 0) ? (kt & 1) : 0;       // timing probes read stage 0 only
    if (R3M_PROBE(p) != 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // my share of tile kt has landed
    if (R3M_PROBE(p) != 2) __syncthreads();                   // everyone's has; and everyone is done reading stage cur^1
    if (kt + 1 < nk && R3M_PROBE(p) != 1) {
      if (++chunk_n == kpt) {
        chunk_n = 0;
        ++tap_n;
        pack_cur = pack_next;
        pack_next = p.tap[min(tap_n + 1, p.ntaps - 1)];
      }
      issue_tile(pack_cur, chunk_n, (R3M_PROBE(p) == 0) ? (cur ^ 1) : 1);
    }
    const float* fa = fragA0 + cur * STAGE;
    const float* fb = fragB0 + cur * STAGE;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 a[TM], b[TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) a[t] = *reinterpret_cast<const f32x4*>(fa + t * 32 * 32 + goff[g]);
#pragma unroll
      for (int t = 0; t < TN; ++t) b[t] = *reinterpret_cast<const f32x4*>(fb + t * 32 * 32 + goff[g]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][j], b[tn][j], acc[tm][tn], 0, 0, 0);
    }
  }
  __syncthreads();   // all fragment reads done before the epilogue reuses the stages

  gg_epilogue<BM, BN, WM, WN, EPI, 2 * STAGE>(p, acc, smem, m0, n0, mt);
}

// =====================================================================================================
// gather-GEMM, direct-to-LDS staging, low-VALU main loop (used whenever Ci/32 is even — every ResNet layer).
// On gfx950 the f32-input MFMA runs at the fp32 VECTOR rate and, measured here, does NOT overlap with VALU work of
// co-resident waves: every VALU instruction in the K loop costs MFMA time (loads issued but never waited for cost the
// same 12 % as the full pipeline; removing the loader entirely gives 139-149 TF). So this variant strips the loop of
// vector ALU work: per-lane source POINTERS are kept per staged row and advanced by 256 B every second K step, the odd
// step uses the instruction's immediate offset (+128 B), validity is folded into the pointer once per tap (invalid rows
// walk along a zero buffer), the K loop is unrolled by two so LDS stage and fragment offsets are immediates, and the
// wave-uniform LDS destinations live in SGPRs. ~8 VALU instructions per K step instead of ~160.
// =====================================================================================================
template <int BM, int BN, int STG, int IMM>
__device__ __forceinline__ void glds_issue(const float* const (&pa)[BM / 32], const float* const (&pb)[BN / 32], float* smem,
                                           int wave_s) {
  constexpr int STAGE = (BM + BN) * 32;
  // the instruction's immediate offset is added to BOTH the global address and the LDS address (M0 base + offset +
  // lane*16), so the LDS destination is pre-biased by -IMM
  float* la = smem + STG * STAGE + wave_s * (BM / 4) * 32 - IMM / 4;
  float* lb = smem + STG * STAGE + BM * 32 + wave_s * (BN / 4) * 32 - IMM / 4;
#pragma unroll
  for (int j = 0; j < BM / 32; ++j)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pa[j],
                                     (__attribute__((address_space(3))) void*)(la + j * 8 * 32), 16, IMM, 0);
#pragma unroll
  for (int j = 0; j < BN / 32; ++j)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pb[j],
                                     (__attribute__((address_space(3))) void*)(lb + j * 8 * 32), 16, IMM, 0);
}

template <int BM, int BN, int STG>
__device__ __forceinline__ void glds_mfma(f32x16 (&acc)[2][2], const float* const (&fa)[4], const float* const (&fb)[4]) {
  constexpr int STAGE = (BM + BN) * 32;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) a[t] = *reinterpret_cast<const f32x4*>(fa[g] + STG * STAGE + t * 32 * 32);
#pragma unroll
    for (int t = 0; t < 2; ++t) b[t] = *reinterpret_cast<const f32x4*>(fb[g] + STG * STAGE + t * 32 * 32);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][j], b[tn][j], acc[tm][tn], 0, 0, 0);
  }
}

// MFMAs of the tile in stage STG_M with the NEXT tile's DMA pieces interleaved: one piece after every 64/NP MFMAs. A DMA
// instruction costs the issuing wave ~60-180 cycles of issue time (MI355X_MICROARCH.md); spread between MFMAs (each holds
// the matrix pipe 64 cycles) that cost hides behind the wave's own MFMAs instead of delaying their start.
template <int BM, int BN, int STG_M, int STG_D, int IMM>
__device__ __forceinline__ void glds_mfma_dma(f32x16 (&acc)[2][2], const float* const (&fa)[4], const float* const (&fb)[4],
                                              const float* const (&pa)[BM / 32], const float* const (&pb)[BN / 32], float* smem,
                                              int wave_s, bool do_dma) {
  constexpr int STAGE = (BM + BN) * 32;
  constexpr int AJ = BM / 32, BJ = BN / 32, NP = AJ + BJ;   // DMA pieces per wave per tile
  static_assert(NP == 8 || NP == 10, "piece schedule assumes 8 (128x128) or 10 (256x64) pieces");
  float* la = smem + STG_D * STAGE + wave_s * (BM / 4) * 32 - IMM / 4;
  float* lb = smem + STG_D * STAGE + BM * 32 + wave_s * (BN / 4) * 32 - IMM / 4;
  auto dma_one = [&](int pc) {
    if (pc < AJ)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pa[pc],
                                       (__attribute__((address_space(3))) void*)(la + pc * 8 * 32), 16, IMM, 0);
    else
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pb[pc - AJ],
                                       (__attribute__((address_space(3))) void*)(lb + (pc - AJ) * 8 * 32), 16, IMM, 0);
  };
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) a[t] = *reinterpret_cast<const f32x4*>(fa[g] + STG_M * STAGE + t * 32 * 32);
#pragma unroll
    for (int t = 0; t < 2; ++t) b[t] = *reinterpret_cast<const f32x4*>(fb[g] + STG_M * STAGE + t * 32 * 32);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][j], b[tn][j], acc[tm][tn], 0, 0, 0);
      if (do_dma) {
        // 16 slots (one per 4 MFMAs); use every second slot for 8 pieces, and slots 0..9 of the odd/even mix for 10
        const int slot = g * 4 + j;   // compile-time after unrolling: the piece index must be too (no scratch arrays)
        const bool fire = (NP == 8) ? ((slot & 1) == 1) : (slot < 12 && (slot % 6) != 5);
        const int piece = (NP == 8) ? (slot >> 1) : (slot - (slot > 5 ? 1 : 0));
        if (fire) {
          __builtin_amdgcn_sched_barrier(0);
          dma_one(piece);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
}

// Block BM x BN with 4 waves laid out WM x WN, every wave a 64 x 64 sub-tile: <128,128,2,2> and <256,64,4,1>.
template <int BM, int BN, int WM, int WN, int EPI>
__global__ __launch_bounds__(256) void gather_gemm_glds2_kernel(const GatherGemmParams p) {
  constexpr int TM = 2, TN = 2;
  static_assert(BM / WM == 64 && BN / WN == 64 && WM * WN == 4, "wave tile is 64 x 64");
  constexpr int STAGE = (BM + BN) * 32;
  constexpr int AJ = BM / 32, BJ = BN / 32;     // DMA instructions per wave per stage (8 rows each)
  __shared__ __attribute__((aligned(128))) float smem[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave id in an SGPR: LDS destinations stay scalar
  const int wm = wave_s / WN, wn = wave_s % WN;
  const int gridN = (p.Nc + BN - 1) / BN;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = lid / gridN, nt = lid % gridN;
  const int m0 = mt * BM, n0 = nt * BN;

  const int srow = lane >> 3, pslot = lane & 7;
  const int Hb = p.simple_rows ? 1 : p.Hi, Wb = p.simple_rows ? 1 : p.Wi;
  RowDesc ad[AJ];
  int acol[AJ];
  unsigned arow_ok = 0;
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    const int r = wave_s * (BM / 4) + j * 8 + srow;
    acol[j] = (pslot ^ ((r >> 1) & 7)) * 4;
    const int m = m0 + r;
    ad[j] = decode_row(p, m);
    if (m < p.M) arow_ok |= 1u << j;
  }
  const float* bptr[BJ];               // weight row pointers (tap 0, chunk 0)
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int r = wave_s * (BN / 4) + j * 8 + srow;
    const int n = min(n0 + r, p.Nc - 1);
    bptr[j] = p.B + (long long)n * p.T * p.Ci + (pslot ^ ((r >> 1) & 7)) * 4;
  }

  const int kpt = p.Ci >> 5;          // K tiles per tap (even)
  const int hpt = kpt >> 1;           // tile pairs per tap
  const int npairs = p.ntaps * hpt;

  const float* pa[AJ];
  const float* pb[BJ];
  auto set_tap = [&](int pack) {
    const int dy = (pack << 24) >> 24, dx = (pack << 16) >> 24, wt = pack >> 16;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int iy = ad[j].iy + dy, ix = ad[j].ix + dx;
      const bool in = ((unsigned)iy < (unsigned)Hb) && ((unsigned)ix < (unsigned)Wb) && ((arow_ok >> j) & 1u);
      const int iyc = min(max(iy, 0), Hb - 1), ixc = min(max(ix, 0), Wb - 1);
      const float* src = p.A + ad[j].base + ((long long)iyc * p.Wi + ixc) * p.Ci + acol[j];
      const unsigned long long msk = in ? ~0ull : 0ull;
      pa[j] = reinterpret_cast<const float*>((reinterpret_cast<unsigned long long>(src) & msk) |
                                             (reinterpret_cast<unsigned long long>(g_zero_line + acol[j]) & ~msk));
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) pb[j] = bptr[j] + (long long)wt * p.Ci;
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int lrow = lane & 31, lh = lane >> 5;
  const int xr = (lrow >> 1) & 7;
  const float* fa[4];
  const float* fb[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int go = ((2 * g + lh) ^ xr) * 4;
    fa[g] = smem + (wm * 64 + lrow) * 32 + go;
    fb[g] = smem + BM * 32 + (wn * 64 + lrow) * 32 + go;
  }

  int tap_n = 0, cp = 0;
  if (npairs > 0) {
    set_tap(p.tap[0]);
    glds_issue<BM, BN, 0, 0>(pa, pb, smem, wave_s);               // tile 0
  }
  int pack_next = p.ntaps > 1 ? p.tap[1] : 0;
  if (R3M_PROBE(p) == 8) {   // clustered DMA issue (kept for A/B: R3M_GG_DEBUG=8)
    for (int pr = 0; pr < npairs; ++pr) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      glds_issue<BM, BN, 1, 128>(pa, pb, smem, wave_s);
      glds_mfma<BM, BN, 0>(acc, fa, fb);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (pr + 1 < npairs) {
        if (++cp == hpt) {
          cp = 0;
          ++tap_n;
          set_tap(pack_next);
          pack_next = p.tap[min(tap_n + 1, p.ntaps - 1)];
        } else {
#pragma unroll
          for (int j = 0; j < AJ; ++j) pa[j] += 64;
#pragma unroll
          for (int j = 0; j < BJ; ++j) pb[j] += 64;
        }
        glds_issue<BM, BN, 0, 0>(pa, pb, smem, wave_s);
      }
      glds_mfma<BM, BN, 1>(acc, fa, fb);
    }
  } else {
    for (int pr = 0; pr < npairs; ++pr) {
      // ---- even tile (stage 0): its MFMAs carry the DMA of the odd tile (same tap, next 32 channels, stage 1) ----
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      glds_mfma_dma<BM, BN, 0, 1, 128>(acc, fa, fb, pa, pb, smem, wave_s, true);
      // ---- odd tile (stage 1): carries the DMA of the next pair's even tile (stage 0) ----
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const bool more = pr + 1 < npairs;
      if (more) {
        if (++cp == hpt) {
          cp = 0;
          ++tap_n;
          set_tap(pack_next);
          pack_next = p.tap[min(tap_n + 1, p.ntaps - 1)];
        } else {
#pragma unroll
          for (int j = 0; j < AJ; ++j) pa[j] += 64;
#pragma unroll
          for (int j = 0; j < BJ; ++j) pb[j] += 64;
        }
      }
      glds_mfma_dma<BM, BN, 1, 0, 0>(acc, fa, fb, pa, pb, smem, wave_s, more);
    }
  }
  __syncthreads();

  gg_epilogue<BM, BN, WM, WN, EPI, 2 * STAGE>(p, acc, smem, m0, n0, mt);
}

// =====================================================================================================
// gather-GEMM 128 x 128 with 16-wide K tiles (64-byte LDS rows) for launches whose main loop is SHORT: the expanding 1x1
// convolutions (K = Cin = 64 / 128 / 256 against N = 4 Cin) and the 1x1 downsample convolutions. There a block's life is
// prologue latency + 2-8 K steps + a 64 KB epilogue, and with the 64 KB of the 32-wide two-stage ring only two blocks share a
// CU, so nothing hides the one's loads / stores behind the other's (measured round 1: 62.6 / 87 / 110 TFLOP/s for K = 64 / 128 /
// 256 against 117 for the class; these launches sit at the HBM ridge — 25 FLOP/B for K = 64). With 16-wide tiles the ring is
// 2 x 16 KB and the LDS footprint is the 34 KB epilogue slab: three to four blocks per CU (registers: 128 per lane).
// Layout: rows of 16 floats = four 16-byte slots, slot XOR ((row >> 2) & 3) — a ds_read_b128 lane group (16 lanes, MI355X
// guide) then touches 16 distinct slots of the 256-byte bank row; one DMA instruction lands 16 rows (lane -> row lane>>2,
// slot lane&3; the swizzle is applied to the global source column). Fragments and MFMA order as in the 32-wide kernel
// (k = 8g + 4h .. +3 per lane half h, groups g = 0, 1), so results are bit-identical to it.
// =====================================================================================================
template <int EPI>
__global__ __launch_bounds__(256, 4) void gather_gemm_k16_kernel(const GatherGemmParams p) {
  constexpr int BM = 128, BN = 128, WM = 2, WN = 2;
  constexpr int STAGE = (BM + BN) * 16;                  // floats per stage (16 KiB)
  constexpr int SMEM = 4 * 32 * (64 + 4);                // the epilogue slab (8704 floats) >= the two stages (8192)
  static_assert(SMEM >= 2 * STAGE, "ring must fit under the epilogue slab");
  __shared__ __attribute__((aligned(128))) float smem[SMEM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave_s / WN, wn = wave_s % WN;
  const int gridN = (p.Nc + BN - 1) / BN;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = lid / gridN, nt = lid % gridN;
  const int m0 = mt * BM, n0 = nt * BN;

  // staging: a wave owns 32 A rows and 32 B rows = 2 + 2 DMA instructions of 16 rows per tile
  const int srow = lane >> 2;
  const int scol = ((lane & 3) ^ ((lane >> 4) & 3)) * 4;   // (row >> 2) & 3 == (lane >> 4) & 3: row = 32 w + 16 j + (lane >> 2)
  const int Hb = p.simple_rows ? 1 : p.Hi, Wb = p.simple_rows ? 1 : p.Wi;
  RowDesc ad[2];
  unsigned arow_ok = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wave_s * 32 + j * 16 + srow;
    ad[j] = decode_row(p, m);
    if (m < p.M) arow_ok |= 1u << j;
  }
  const float* bptr[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = min(n0 + wave_s * 32 + j * 16 + srow, p.Nc - 1);
    bptr[j] = p.B + (long long)n * p.T * p.Ci + scol;
  }
  const int kpt = p.Ci >> 4;          // 16-wide tiles per tap (even: Ci is a multiple of 32)
  const int hpt = kpt >> 1;
  const int npairs = p.ntaps * hpt;

  const float* pa[2];
  const float* pb[2];
  auto set_tap = [&](int pack) {
    const int dy = (pack << 24) >> 24, dx = (pack << 16) >> 24, wt = pack >> 16;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int iy = ad[j].iy + dy, ix = ad[j].ix + dx;
      const bool in = ((unsigned)iy < (unsigned)Hb) && ((unsigned)ix < (unsigned)Wb) && ((arow_ok >> j) & 1u);
      const int iyc = min(max(iy, 0), Hb - 1), ixc = min(max(ix, 0), Wb - 1);
      const float* src = p.A + ad[j].base + ((long long)iyc * p.Wi + ixc) * p.Ci + scol;
      const unsigned long long msk = in ? ~0ull : 0ull;
      pa[j] = reinterpret_cast<const float*>((reinterpret_cast<unsigned long long>(src) & msk) |
                                             (reinterpret_cast<unsigned long long>(g_zero_line + scol) & ~msk));
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) pb[j] = bptr[j] + (long long)wt * p.Ci;
  };
  // stage STG, the instruction's immediate IMM (bytes) is added to BOTH addresses -> LDS destination pre-biased by -IMM
  auto issue = [&](auto stg_c, auto imm_c) __attribute__((always_inline)) {
    constexpr int STG = decltype(stg_c)::value, IMM = decltype(imm_c)::value;
    float* la = smem + STG * STAGE + wave_s * 32 * 16 - IMM / 4;
    float* lb = smem + STG * STAGE + BM * 16 + wave_s * 32 * 16 - IMM / 4;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pa[j],
                                       (__attribute__((address_space(3))) void*)(la + j * 16 * 16), 16, IMM, 0);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pb[j],
                                       (__attribute__((address_space(3))) void*)(lb + j * 16 * 16), 16, IMM, 0);
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int lrow = lane & 31, lh = lane >> 5;
  const int xr = (lrow >> 2) & 3;
  const float* fa[2];
  const float* fb[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int go = ((2 * g + lh) ^ xr) * 4;
    fa[g] = smem + (wm * 64 + lrow) * 16 + go;
    fb[g] = smem + BM * 16 + (wn * 64 + lrow) * 16 + go;
  }
  auto mfma_tile = [&](auto stg_c) __attribute__((always_inline)) {
    constexpr int STG = decltype(stg_c)::value;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      f32x4 a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) a[t] = *reinterpret_cast<const f32x4*>(fa[g] + STG * STAGE + t * 32 * 16);
#pragma unroll
      for (int t = 0; t < 2; ++t) b[t] = *reinterpret_cast<const f32x4*>(fb[g] + STG * STAGE + t * 32 * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int tn = 0; tn < 2; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][j], b[tn][j], acc[tm][tn], 0, 0, 0);
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I64 = std::integral_constant<int, 64>;

  int tap_n = 0, cp = 0;
  if (npairs > 0) {
    set_tap(p.tap[0]);
    issue(I0{}, I0{});                                    // tile 0 -> stage 0
  }
  int pack_next = p.ntaps > 1 ? p.tap[1] : 0;
  for (int pr = 0; pr < npairs; ++pr) {
    // even tile (stage 0): issue the odd tile (same tap, next 16 channels: +64 B immediate) first, then the MFMAs
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    issue(I1{}, I64{});
    mfma_tile(I0{});
    // odd tile (stage 1): issue the next pair's even tile
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (pr + 1 < npairs) {
      if (++cp == hpt) {
        cp = 0;
        ++tap_n;
        set_tap(pack_next);
        pack_next = p.tap[min(tap_n + 1, p.ntaps - 1)];
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) { pa[j] += 32; pb[j] += 32; }
      }
      issue(I0{}, I0{});
    }
    mfma_tile(I1{});
  }
  __syncthreads();
  gg_epilogue<BM, BN, WM, WN, EPI, SMEM>(p, acc, smem, m0, n0, mt);
}

// =====================================================================================================
// gather-GEMM, register staging (256x64 tiles for 64-channel layers; also the 128x128 fallback R3M_GG_GLDS=0).
// Operand tiles live in LDS as [row][k] with a 36-float row stride (conflict-free b128 writes and fragment reads).
// Single LDS stage; the next tile's global loads fly during the MFMA phase.
// =====================================================================================================
template <int BM, int BN, int WM, int WN, int EPI>
__global__ __launch_bounds__(WM * WN * 64) void gather_gemm_kernel(const GatherGemmParams p) {
  constexpr int NT = WM * WN * 64;      // threads
  constexpr int RPP = NT / 8;           // staging rows per pass (8 lanes x float4 cover one 32-float row)
  constexpr int S = 36;
  constexpr int STAGE = (BM + BN) * S;
  constexpr int TM = BM / WM / 32;
  constexpr int TN = BN / WN / 32;
  constexpr int AJ = BM / RPP;  // float4 staging loads per thread (A)
  constexpr int BJ = BN / RPP;  // float4 staging loads per thread (B)
  __shared__ __attribute__((aligned(16))) float smem[STAGE];
  float* sA = smem;
  float* sB = smem + BM * S;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int gridN = (p.Nc + BN - 1) / BN;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = lid / gridN, nt = lid % gridN;
  const int m0 = mt * BM, n0 = nt * BN;

  const int c4 = tid & 7;   // which float4 of the 32-float k slice
  const int r0 = tid >> 3;  // staging row (0..RPP-1), + RPP*j

  const int Hb = p.simple_rows ? 1 : p.Hi, Wb = p.simple_rows ? 1 : p.Wi;
  RowDesc ad[AJ];
  unsigned arow_ok = 0;
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    const int m = m0 + r0 + RPP * j;
    ad[j] = decode_row(p, m);
    if (m < p.M) arow_ok |= 1u << j;
  }
  long long bbase[BJ];
  unsigned brow_ok = 0;
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    int n = n0 + r0 + RPP * j;
    if (n < p.Nc) brow_ok |= 1u << j; else n = p.Nc - 1;
    bbase[j] = (long long)n * p.T * p.Ci;
  }

  const int kpt = p.Ci >> 5;          // K tiles per tap
  const int nk = p.ntaps * kpt;

  f32x4 ra[AJ], rb[BJ];
  unsigned a_ok = 0;                  // validity bits of the tile currently held in ra[]
  auto load_tile = [&](int pack, int chunk) {
    const int dy = (pack << 24) >> 24, dx = (pack << 16) >> 24, wt = pack >> 16;
    const int c0 = chunk * 32 + c4 * 4;
    const long long woff = (long long)wt * p.Ci + c0;
    unsigned ok = 0;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int iy = ad[j].iy + dy, ix = ad[j].ix + dx;
      const bool in = ((unsigned)iy < (unsigned)Hb) && ((unsigned)ix < (unsigned)Wb);
      ok |= (in ? 1u : 0u) << j;
      const int iyc = min(max(iy, 0), Hb - 1), ixc = min(max(ix, 0), Wb - 1);
      ra[j] = ldg4(p.A + ad[j].base + ((long long)iyc * p.Wi + ixc) * p.Ci + c0);
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) rb[j] = ldg4(p.B + bbase[j] + woff);
    a_ok = ok & arow_ok;
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int lrow = lane & 31;
  const int lh4 = (lane >> 5) * 4;
  const float* fragA = sA + (wm * TM * 32 + lrow) * S + lh4;
  const float* fragB = sB + (wn * TN * 32 + lrow) * S + lh4;

  int tap_n = 0, chunk_n = 0;
  int pack_cur = nk > 0 ? p.tap[0] : 0;
  int pack_next = p.ntaps > 1 ? p.tap[1] : pack_cur;
  if (nk > 0) load_tile(pack_cur, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < AJ; ++j)
      *reinterpret_cast<f32x4*>(sA + (r0 + RPP * j) * S + c4 * 4) = ((a_ok >> j) & 1u) ? ra[j] : zero4;
#pragma unroll
    for (int j = 0; j < BJ; ++j)
      *reinterpret_cast<f32x4*>(sB + (r0 + RPP * j) * S + c4 * 4) = ((brow_ok >> j) & 1u) ? rb[j] : zero4;
    __syncthreads();
    if (kt + 1 < nk) {
      if (++chunk_n == kpt) {
        chunk_n = 0;
        ++tap_n;
        pack_cur = pack_next;
        pack_next = p.tap[min(tap_n + 1, p.ntaps - 1)];
      }
      load_tile(pack_cur, chunk_n);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 a[TM], b[TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) a[t] = *reinterpret_cast<const f32x4*>(fragA + t * 32 * S + g * 8);
#pragma unroll
      for (int t = 0; t < TN; ++t) b[t] = *reinterpret_cast<const f32x4*>(fragB + t * 32 * S + g * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][j], b[tn][j], acc[tm][tn], 0, 0, 0);
    }
    __syncthreads();
  }

  gg_epilogue<BM, BN, WM, WN, EPI, STAGE>(p, acc, smem, m0, n0, mt);
}

// =====================================================================================================
// 3x3 / stride 1 / pad 1 convolutions (forward and dgrad) on 128-wide outputs with an INPUT WINDOW in LDS (round 3).
// The gather kernel stages the 128-row A tile once per tap: 4 of its 8 DMA instructions per 64 MFMAs, and on this chip DMA issue
// is what keeps the fp32 main loop at 0.83 instead of the 0.9+ of a no-load loop (the weight gradient gained 6 % from 8 -> 5.3
// DMA instructions per 64 MFMAs). Here the nine taps of a tile of 128 consecutive output pixels read ONE window of 128 + 2W + 2
// input pixels per 32-channel chunk — staged once per chunk, double-buffered, one DMA instruction per tap step — plus the nine
// weight tiles: 4.7 DMA instructions per 64 MFMAs.
//   LDS (80 KB, two blocks per CU): 2 window buffers of 192 rows x 128 B (same 16-byte-slot XOR swizzle as the gather kernel),
//   2 weight stages of 128 x 128 B. Window row 191 is never inside the window (W <= 28): its DMA lanes are out of range, it holds
//   zeros, and a lane whose pixel has no (y + dy, x + dx) inside the image reads IT — the gather kernel's border arithmetic.
//   The A-fragment addresses of all 9 taps x 2 row tiles x 4 K groups are per-lane constants (72 registers), so the K loop has no
//   vector work: DMA offsets are constants, the (tap, chunk) position rides in the instructions' scalar offset.
// Summation order: (chunk, tap) instead of the gather kernel's (tap, chunk) — an fp32 reassociation, inside every gate.
// =====================================================================================================
// In use: <128,128,2,2,192> (W <= 28: the 128/256/512-channel layers; 80 KB, two blocks of 4 waves per CU): 126 -> 131, 133 -> 140,
// 133 -> 141 TFLOP/s at 14^2 / 28^2 / 7^2 (profiles/r03_win_ab.txt). The template also instantiates as <256,64,4,2,376> (the
// 64-channel layers at 56 x 56: 112 KB, ONE block of 8 waves per CU); measured 122 against the gather kernel's 124 there
// (a 370-row window per 2 chunks of 9 taps amortises less, and one block per CU exposes the chunk boundary) — not dispatched.
template <int BM, int BN, int WIN_ROWS>
struct WinCfg {
  static constexpr int WIN_BYTES = WIN_ROWS * 128;
  static constexpr int LDS = 2 * WIN_BYTES + 2 * BN * 128;
};

template <int BM, int BN, int WM, int WN, int WIN_ROWS, int EPI>
__global__ __launch_bounds__(WM * WN * 64, WM * WN == 4 ? 2 : 1) void conv3x3_win_kernel(const GatherGemmParams p) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  static_assert(TM == 2 && (TN == 1 || TN == 2), "wave tile 64 x 32 or 64 x 64");
  constexpr int WIN_BYTES = WIN_ROWS * 128;
  constexpr int BSTAGE = BN * 128;                               // bytes of one weight stage
  constexpr int LDSB = 2 * WIN_BYTES + 2 * BSTAGE;
  extern __shared__ __attribute__((aligned(128))) unsigned char wsm[];
  unsigned char* bst = wsm + 2 * WIN_BYTES;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave_s / WN, wn = wave_s % WN;
  const int gridN = (p.Nc + BN - 1) / BN;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = lid / gridN, nt = lid % gridN;
  const int m0 = mt * BM, n0 = nt * BN;
  const int W = p.Wi, H = p.Hi, HW = H * W;
  const int HR = BM + 2 * W + 2;                                 // window rows in use (< WIN_ROWS)
  constexpr int ZR = WIN_ROWS - 1;                               // the zero row

  // ---- A fragment byte offsets inside a window buffer: [tap][row tile][K group] ----
  const int lrow = lane & 31, lh = lane >> 5;
  unsigned fa[9][TM][4];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int r = wm * (BM / WM) + t * 32 + lrow;
    const int m = m0 + r;
    int y = 0, x = 0;
    if (m < p.M) {
      const int rem = m % HW;
      y = rem / W;
      x = rem - y * W;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int pk = p.tap[k];
      const int dy = (pk << 24) >> 24, dx = (pk << 16) >> 24;
      const bool ok = (m < p.M) && ((unsigned)(y + dy) < (unsigned)H) && ((unsigned)(x + dx) < (unsigned)W);
      const unsigned wr = ok ? (unsigned)(r + (W + 1) + dy * W + dx) : (unsigned)ZR;
      const unsigned base = (wr << 7) | (((wr >> 1) & 7u) << 4);
#pragma unroll
      for (int g = 0; g < 4; ++g) fa[k][t][g] = base ^ ((unsigned)(2 * g + lh) << 4);
    }
  }
  // ---- B fragment byte offsets inside a weight stage ----
  unsigned fb[4];
  {
    const int xr = (lrow >> 1) & 7;
#pragma unroll
    for (int g = 0; g < 4; ++g) fb[g] = (unsigned)((wn * TN * 32 + lrow) * 128 + (((2 * g + lh) ^ xr) << 4));
  }

  // ---- DMA: window pieces (8 rows each; this wave owns pieces wave_s + NW q) and weight pieces (8 rows each) ----
  const int srow = lane >> 3, pslot = lane & 7;
  const long long px00 = (long long)m0 - (W + 1);                // pixel of window row 0
  const long long pxb = px00 > 0 ? px00 : 0;                     // descriptor base pixel
  const float* a_base = p.A + pxb * p.Ci;
  int a_bytes;
  {
    const long long rest = ((long long)p.M - pxb) * p.Ci * 4;
    a_bytes = rest <= 0 ? 0 : (rest < (long long)BUF_OOB ? (int)rest : (int)BUF_OOB);
  }
  constexpr int NWP_ALL = WIN_ROWS / 8;                          // window pieces of a full buffer
  constexpr int NWQ = (NWP_ALL + NW - 1) / NW;                   // per wave (6)
  static_assert(NWQ <= 9, "one window piece per tap step");
  unsigned woff[NWQ];
#pragma unroll
  for (int q = 0; q < NWQ; ++q) {
    const int hr = 8 * (wave_s + NW * q) + srow;
    const long long px = px00 + hr;
    const bool ok = hr < HR && px >= 0;                          // px >= M falls off the descriptor
    woff[q] = ok ? (unsigned)((int)(px - pxb) * p.Ci * 4) + (unsigned)((pslot ^ ((hr >> 1) & 7)) << 4) : BUF_OOB;
  }
  const int nwp = (HR + 7) / 8;                                  // pieces that hold window rows; the last piece (zero row) always goes
  constexpr int BJ = BN / 8 / NW;                                // weight pieces per wave (4 or 1)
  static_assert(BJ >= 1 && BJ * 8 * NW == BN, "weight rows split over the waves");
  unsigned bvoff[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int r = wave_s * (BN / NW) + j * 8 + srow;
    const int n = min(n0 + r, p.Nc - 1);
    bvoff[j] = (unsigned)(n * p.T * p.Ci * 4) + (unsigned)((pslot ^ ((r >> 1) & 7)) << 4);
  }
  const int b_bytes = p.Nc * p.T * p.Ci * 4;

  auto issue_window_piece = [&](int q, int chunk, int buf) __attribute__((always_inline)) {
    const int i = wave_s + NW * q;
    if (R3M_PROBE(p) & 8) return;                                // timing probe: no window DMA (stale LDS)
    if (i < nwp || i == NWP_ALL - 1)
      buf_dma16(a_base, a_bytes, wsm + buf * WIN_BYTES + i * 1024, woff[q], chunk * 128);
  };
  auto issue_b_piece = [&](int j, int tapk, int chunk, int stage) __attribute__((always_inline)) {
    const int wt = p.tap[tapk] >> 16;
    if (R3M_PROBE(p) & 16) return;                               // timing probe: no weight DMA
    buf_dma16(p.B, b_bytes, bst + stage * BSTAGE + (wave_s * (BN / NW) + j * 8) * 128, bvoff[j], (wt * p.Ci + chunk * 32) * 4);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int nchunks = p.Ci >> 5;
  // one tap step: the MFMAs of window buffer WB (tap K) x weight stage ST, carrying the DMA of the NEXT step's weights and one
  // window piece of the next chunk
  auto step = [&](auto k_c, auto wb_c, auto st_c, int chunk) __attribute__((always_inline)) {
    constexpr int K = decltype(k_c)::value, WB = decltype(wb_c)::value, ST = decltype(st_c)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool last_chunk = chunk + 1 >= nchunks;
    const bool more_b = !(last_chunk && K == 8);
    const int nk = K == 8 ? 0 : K + 1, nc = K == 8 ? chunk + 1 : chunk;
    static_for<4>([&](auto g_c) __attribute__((always_inline)) {
      constexpr int g = decltype(g_c)::value;
      f32x4 a[TM], b[TN];
#pragma unroll
      for (int t = 0; t < TM; ++t)
        a[t] = *reinterpret_cast<const f32x4*>(wsm + WB * WIN_BYTES + fa[K][t][g]);
#pragma unroll
      for (int t = 0; t < TN; ++t)
        b[t] = *reinterpret_cast<const f32x4*>(bst + ST * BSTAGE + t * 32 * 128 + fb[g]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][j], b[tn][j], acc[tm][tn], 0, 0, 0);
        if (j == 1) {
          __builtin_amdgcn_sched_barrier(0);
          if (g < BJ && more_b) issue_b_piece(g, nk, nc, ST ^ 1);
          if (g == 3 && K < NWQ && !last_chunk) issue_window_piece(K, chunk + 1, WB ^ 1);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    });
  };
  auto chunk_steps = [&](auto wb_c, int chunk) __attribute__((always_inline)) {
    constexpr int WB = decltype(wb_c)::value;                  // window buffer = chunk parity; weight stage = (chunk + tap) parity
    static_for<9>([&](auto k_c) __attribute__((always_inline)) {
      constexpr int K = decltype(k_c)::value;
      step(k_c, wb_c, std::integral_constant<int, (WB + K) & 1>{}, chunk);
    });
  };

  if (nchunks > 0) {
#pragma unroll
    for (int q = 0; q < NWQ; ++q) issue_window_piece(q, 0, 0);
#pragma unroll
    for (int j = 0; j < BJ; ++j) issue_b_piece(j, 0, 0, 0);
  }
  int c = 0;
  for (; c + 1 < nchunks; c += 2) {
    chunk_steps(std::integral_constant<int, 0>{}, c);
    chunk_steps(std::integral_constant<int, 1>{}, c + 1);
  }
  if (c < nchunks) chunk_steps(std::integral_constant<int, 0>{}, c);
  __syncthreads();

  gg_epilogue<BM, BN, WM, WN, EPI, LDSB / 4>(p, acc, reinterpret_cast<float*>(wsm), m0, n0, mt);
}

// 3x3 / stride 1 / pad 1 on the full pixel grid with the taps being exactly {-1,0,1}^2, 128-wide outputs, W <= 28
static bool conv3x3_win_eligible(const GatherGemmParams& p, int maxW) {
  if (p.ntaps != 9 || p.is != 1 || p.os != 1 || p.simple_rows || p.Hg != p.Hi || p.Wg != p.Wi || p.Ho != p.Hi || p.Wo != p.Wi) return false;
  if (p.Wi > maxW || p.Wi < 1 || (p.Ci & 31)) return false;
  unsigned seen = 0;
  for (int t = 0; t < 9; ++t) {
    if (p.dy[t] < -1 || p.dy[t] > 1 || p.dx[t] < -1 || p.dx[t] > 1) return false;
    seen |= 1u << ((p.dy[t] + 1) * 3 + (p.dx[t] + 1));
  }
  return seen == 0x1ffu && (long long)p.Nc * p.T * p.Ci * 4 < 0x7FFFF000LL;
}

static inline bool gg_wide(int Nc) { return (Nc % 128) == 0; }

int gather_gemm_grid_m(int M, int Nc) { return gg_wide(Nc) ? ceil_div(M, 128) : ceil_div(M, 256); }

// R3M_GG_GLDS: 2 (default) low-VALU direct-to-LDS kernel, 1 generic direct-to-LDS kernel, 0 register staging
static int gg_use_glds() {
  const int v = R3M_ENV_INT("R3M_GG_GLDS", 2);
  return v;
}

#define GG_EPI_SWITCH(LAUNCH)                                                       \
  switch (p.flags) {                                                                \
    case 0: LAUNCH(0); break;                                                       \
    case EPI_STATS: LAUNCH(EPI_STATS); break;                                       \
    case EPI_ACCUM: LAUNCH(EPI_ACCUM); break;                                       \
    case EPI_MASKED_ADD: LAUNCH(EPI_MASKED_ADD); break;                             \
    case EPI_BIAS: LAUNCH(EPI_BIAS); break;                                         \
    case EPI_RELU: LAUNCH(EPI_RELU); break;                                         \
    case EPI_BIAS | EPI_RELU: LAUNCH(EPI_BIAS | EPI_RELU); break;                   \
    case EPI_MASK_OUT: LAUNCH(EPI_MASK_OUT); break;                                 \
    case EPI_BNRED: LAUNCH(EPI_BNRED); break;                                       \
    case EPI_BNRED | EPI_MASKED_ADD: LAUNCH(EPI_BNRED | EPI_MASKED_ADD); break;     \
    default:                                                                        \
      set_last_error("gather_gemm: unsupported epilogue flag combination %d", p.flags); \
      return 1;                                                                     \
  }

// algorithmic HBM bytes of one gather-GEMM launch: the input tensor once, the weights once, the result once (+ the tensors
// a read-modify-write epilogue adds: the old result / the residual gradient and its 1-bit mask)
// The input counts the pixels some (GEMM row, tap) pair of the launch reads: padding is no traffic, nor are the pixels no tap reaches
// (three quarters of the input of a 1x1 / stride-2 convolution, all of dY for a parity class without taps). Per-channel operands
// (bias, eval-BatchNorm scale / shift, the BatchNorm-backward mean and mask coefficients) and the statistics rows are fp32.
// Only evaluated while a bracket is open (prof_open).
static double gather_gemm_pixels_read(const GatherGemmParams& p) {
  if (p.simple_rows) return (double)p.M;
  std::vector<char> row(p.Hi > 0 ? p.Hi : 0, 0), col(p.Wi > 0 ? p.Wi : 0, 0);
  for (int t = 0; t < p.ntaps; ++t) {
    for (int gy = 0; gy < p.Hg; ++gy) {
      const int iy = gy * p.is + p.dy[t];
      if (iy >= 0 && iy < p.Hi) row[iy] = 1;
    }
    for (int gx = 0; gx < p.Wg; ++gx) {
      const int ix = gx * p.is + p.dx[t];
      if (ix >= 0 && ix < p.Wi) col[ix] = 1;
    }
  }
  long long rows = 0, cols = 0;      // the taps of a launch are a product set (kernel rows x kernel columns): so are the pixels read
  for (char c : row) rows += c;
  for (char c : col) cols += c;
  return (double)p.N * (double)rows * (double)cols;
}
double gather_gemm_alg_bytes(const GatherGemmParams& p, int elem) {
  const double in = gather_gemm_pixels_read(p) * p.Ci;
  const double out = (double)p.M * p.Nc;
  double b = elem * (in + out + (double)p.Nc * p.ntaps * p.Ci);
  if (p.flags & EPI_STATS) b += 8.0 * gather_gemm_grid_m(p.M, p.Nc) * p.Nc;
  if (p.flags & EPI_BIAS) b += 4.0 * p.Nc;
  if (p.flags & EPI_AFFINE) b += 8.0 * p.Nc;
  if (p.flags & EPI_ACCUM) b += elem * out;
  if (p.flags & EPI_MASKED_ADD) b += elem * out + out / 8.0;
  if (p.flags & EPI_MASK_OUT) b += elem * out;
  if (p.flags & EPI_BNRED)      // + y, the mask (bits, or scale and shift to recompute it), the mean, the partial rows
    b += elem * out + (p.bn_bits ? out / 8.0 : 8.0 * p.Nc) + 4.0 * p.Nc + 8.0 * bnred_partial_rows(p.M) * p.Nc;
  return b;
}

static thread_local unsigned* t_tile_ctr = nullptr;
static thread_local int t_tile_ctr_sets = 0;   // further sets of 8 counters behind t_tile_ctr (the parity-class launches of a stride-2 dgrad)
static int g_dynamic_tiles = 1;          // diagnostic (tools/occupy_ab.py): plain int, written before launches from the same thread
void gg_set_tile_counters(unsigned* ctr8, int sets) {
  t_tile_ctr = g_dynamic_tiles ? ctr8 : nullptr;
  t_tile_ctr_sets = t_tile_ctr ? sets : 0;
}
int gg_set_dynamic_tiles(int on) { const int old = g_dynamic_tiles; g_dynamic_tiles = on ? 1 : 0; return old; }

// Which kernel family a launch runs (a pure function of the launch parameters; taps must be packed). Also what
// r3m_debug_conv_route reports, so that the dispatch DESIGN.md describes is checked on CPU (tests/test_host.py).
enum : int { GG_ROUTE_WIN = 1, GG_ROUTE_PW = 10 /* + pw_gemm_form: 11 pointwise, 12 gather, 13 strided output */, GG_ROUTE_K16 = 20,
             GG_ROUTE_GLDS2 = 21, GG_ROUTE_OTHER = 22, GG_ROUTE_BF16 = 30 };
static int gg_route(const GatherGemmParams& p) {
  if (p.dtype == DT_BF16) return GG_ROUTE_BF16;
  const bool glds2 = gg_use_glds() == 2 && ((p.Ci >> 5) & 1) == 0 && p.Ci <= 2048;
  if (gg_wide(p.Nc)) {
    if (R3M_ENV_INT("R3M_GG_WIN", 1) && conv3x3_win_eligible(p, 28)) return GG_ROUTE_WIN;   // probe builds: 0 = gather kernel for 3x3 / stride 1 too
    if (R3M_ENV_INT("R3M_GG_PW", 1) && pw_gemm_eligible(p)) return GG_ROUTE_PW + pw_gemm_form(p);
    // short main loop + wide output: single tap, K <= 256, N >= 2 K (expanding / downsample 1x1 convolutions) -> 16-wide K tiles
    // R3M_GG_K16 (probe builds): 0 = never, 1 = the rule above, 2 = every wide launch (experiment: 4 blocks per CU everywhere)
    const int k16_mode = R3M_ENV_INT("R3M_GG_K16", 1);
    if ((p.Ci & 31) == 0 && (k16_mode == 2 || (k16_mode == 1 && p.ntaps == 1 && p.Ci <= 256 && p.Nc >= 2 * p.Ci))) return GG_ROUTE_K16;
    return glds2 ? GG_ROUTE_GLDS2 : GG_ROUTE_OTHER;
  }
  if (R3M_ENV_INT("R3M_GG_PW", 1) && pw_gemm_eligible(p)) return GG_ROUTE_PW + pw_gemm_form(p);
  return glds2 ? GG_ROUTE_GLDS2 : GG_ROUTE_OTHER;
}

// What launch_gather_gemm and gather_gemm_fuses_affine do to their copy of the parameters before anything looks at it: the packed tap
// table the kernels and gg_route read, and the probe switch. It checks nothing, so the query answers for any parameters.
static void gg_prepare(GatherGemmParams& p) {
  for (int t = 0; t < p.ntaps; ++t)
    p.tap[t] = (int)((unsigned)(unsigned char)p.dy[t] | ((unsigned)(unsigned char)p.dx[t] << 8) | ((unsigned)p.wt[t] << 16));
  p.debug = R3M_ENV_INT("R3M_GG_DEBUG", 0);   // timing probes only (wrong results when != 0)
}

// inference forward: can this launch apply eval-mode BatchNorm (+ residual) (+ ReLU) where it stores (EPI_AFFINE family)? True for the
// kernels every ResNet layer runs (the persistent kernel, the 3x3 window kernel; every bf16 kernel); the engine falls back to
// conv + bn_act_fwd for anything else (odd shapes of the fuzz tests).
bool gather_gemm_fuses_affine(const GatherGemmParams& p_in) {
  GatherGemmParams p = p_in;
  gg_prepare(p);
  if (p.dtype == DT_BF16) return (p.Nc & 7) == 0 && (p.Ci & 63) == 0 && gg16_route_builds(gg16_route(p), p.flags);
  const int r = gg_route(p);
  if (r == GG_ROUTE_WIN) return p.flags == (EPI_AFFINE | EPI_RELU) || p.flags == (EPI_AFFINE | EPI_ACCUM | EPI_RELU);
  return r > GG_ROUTE_PW && r < GG_ROUTE_K16;
}
static thread_local int* t_route_out = nullptr;      // dry run (r3m_debug_conv_route): record the route of every launch, launch nothing
static thread_local int t_route_n = 0, t_route_cap = 0;
void gg_route_record_begin(int* out, int cap) { t_route_out = out; t_route_n = 0; t_route_cap = cap; }
int gg_route_record_end() { const int n = t_route_n; t_route_out = nullptr; t_route_n = t_route_cap = 0; return n; }
static int gg_route_record(int route) {
  if (t_route_n < t_route_cap) t_route_out[t_route_n] = route;
  ++t_route_n;
  return 0;
}

// The three kernels behind GG_ROUTE_OTHER (launches gg_route leaves to neither the window, the persistent, the 16-wide-K nor the
// low-VALU kernel; no ResNet layer, but r3m_conv2d_* / r3m_linear_* and the fuzz tests on 96- and 160-channel sides):
//   GG_OTHER_GLDS   wide, odd Ci/32 (or Ci > 2048; probe builds: R3M_GG_GLDS=1)    gather_gemm_glds_kernel
//   GG_OTHER_NARROW narrow (Nc no multiple of 128)                                  gather_gemm_kernel<256,64,4,1>
//   GG_OTHER_REG    wide, probe build with R3M_GG_GLDS=0                            gather_gemm_kernel<128,128,2,2>
enum : int { GG_OTHER_GLDS, GG_OTHER_NARROW, GG_OTHER_REG };
static int gg_other_kernel(bool wide) {
  if (!wide) return GG_OTHER_NARROW;
#ifdef R3M_PROBES
  if (!gg_use_glds()) return GG_OTHER_REG;
#endif
  return GG_OTHER_GLDS;
}

int launch_gather_gemm(const GatherGemmParams& p_in, hipStream_t s) {
  GatherGemmParams p = p_in;
  p.tile_ctr = t_tile_ctr;     // one set of counters serves ONE launch: the parity-class launches of a stride-2 dgrad take the next
  if (t_tile_ctr && --t_tile_ctr_sets > 0) t_tile_ctr += 8;   // set each, and the next layer must not reuse any of them
  else { t_tile_ctr = nullptr; t_tile_ctr_sets = 0; }
  R3M_REQUIRE(p.ntaps >= 0 && p.ntaps <= MAX_TAPS, "gather_gemm: ntaps=%d", p.ntaps);     // both precisions
  R3M_REQUIRE(p.M > 0 && p.Nc > 0, "gather_gemm: empty problem M=%d Nc=%d", p.M, p.Nc);
  gg_prepare(p);
  if (p.dtype == DT_BF16) {
    if (t_route_out) return gg_route_record(gg16_route(p));    // 30 gather, 31 halo, 32 kernel-row, 33 probe-build persistent (GG_ROUTE_BF16 + family)
    return launch_gather_gemm_bf16(p, s);
  }
  R3M_REQUIRE(p.Ci % 32 == 0, "gather_gemm: Ci=%d must be a multiple of 32", p.Ci);
  R3M_REQUIRE(p.Nc % 4 == 0, "gather_gemm: Nc=%d must be a multiple of 4", p.Nc);
  R3M_REQUIRE((reinterpret_cast<uintptr_t>(p.A) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.B) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(p.out) & 15) == 0,
              "gather_gemm: operands must be 16-byte aligned");
  const int route = gg_route(p);
  if (t_route_out) return gg_route_record(route);
  const bool wide = gg_wide(p.Nc);       // 128 x 128 tiles, or 256 x 64 for outputs that are no multiple of 128 wide
  const int grid = wide ? ceil_div(p.M, 128) * ceil_div(p.Nc, 128) : ceil_div(p.M, 256) * ceil_div(p.Nc, 64);
  const double flops = 2.0 * (double)p.M * (double)p.Nc * ((double)p.ntaps * p.Ci);
  prof_begin(wide ? KC_GEMM_WIDE : KC_GEMM_NARROW, flops, p.M, p.Nc, p.Ci, p.ntaps, s);
  const char* what = "gather_gemm";
#define LAUNCH_GG(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(grid), dim3(256), 0, s, p)
  switch (route) {
    case GG_ROUTE_WIN: {
      typedef WinCfg<128, 128, 192> Cfg;
#define LAUNCH_WIN(E)                                                                                                        \
  do {                                                                                                                       \
    static DynLdsOptIn oi;                                                                                                   \
    if (int e = ensure_dyn_lds(oi, reinterpret_cast<const void*>(conv3x3_win_kernel<128, 128, 2, 2, 192, E>), Cfg::LDS, "conv3x3_win")) return e; \
    hipLaunchKernelGGL((conv3x3_win_kernel<128, 128, 2, 2, 192, E>), dim3(grid), dim3(256), Cfg::LDS, s, p);                 \
  } while (0)
      switch (p.flags) {                       // inference forward (round 6): eval-mode BatchNorm (+ residual in `out`) + ReLU at the store
        case EPI_AFFINE | EPI_RELU: LAUNCH_WIN(EPI_AFFINE | EPI_RELU); break;
        case EPI_AFFINE | EPI_ACCUM | EPI_RELU: LAUNCH_WIN(EPI_AFFINE | EPI_ACCUM | EPI_RELU); break;
        default:
          GG_EPI_SWITCH(LAUNCH_WIN)
      }
#undef LAUNCH_WIN
      what = "conv3x3_win";
      break;
    }
    case GG_ROUTE_PW + 1:
    case GG_ROUTE_PW + 2:
    case GG_ROUTE_PW + 3:     // dense or parity-strided output rows: persistent kernel (conv_pw.hip), four-wave 128-wide or eight-wave 64-wide tile
      if (int e = launch_pw_gemm(p, s)) return e;
      what = "pw_gemm";
      break;
    case GG_ROUTE_K16: {
#define LAUNCH_K16(E) LAUNCH_GG(gather_gemm_k16_kernel<E>)
      GG_EPI_SWITCH(LAUNCH_K16)
#undef LAUNCH_K16
      break;
    }
    case GG_ROUTE_GLDS2: {
#define LAUNCH_GLDS2(E) LAUNCH_GG(gather_gemm_glds2_kernel<128, 128, 2, 2, E>)
#define LAUNCH_NARROW2(E) LAUNCH_GG(gather_gemm_glds2_kernel<256, 64, 4, 1, E>)
      if (wide) { GG_EPI_SWITCH(LAUNCH_GLDS2) }
      else { GG_EPI_SWITCH(LAUNCH_NARROW2) }
#undef LAUNCH_GLDS2
#undef LAUNCH_NARROW2
      break;
    }
    case GG_ROUTE_OTHER:
    default: {                // gg_route returns nothing else; as before, a route that is none of the above runs a gather kernel
#define LAUNCH_GLDS(E) LAUNCH_GG(gather_gemm_glds_kernel<E>)
#define LAUNCH_NARROW(E) LAUNCH_GG(gather_gemm_kernel<256, 64, 4, 1, E>)
#define LAUNCH_REG(E) LAUNCH_GG(gather_gemm_kernel<128, 128, 2, 2, E>)
      switch (gg_other_kernel(wide)) {
        case GG_OTHER_NARROW: GG_EPI_SWITCH(LAUNCH_NARROW) break;
#ifdef R3M_PROBES
        case GG_OTHER_REG: GG_EPI_SWITCH(LAUNCH_REG) break;
#endif
        default: GG_EPI_SWITCH(LAUNCH_GLDS) break;
      }
#undef LAUNCH_GLDS
#undef LAUNCH_NARROW
#undef LAUNCH_REG
      break;
    }
  }
#undef LAUNCH_GG
  if (prof_open()) prof_bytes(gather_gemm_alg_bytes(p, 4));
  prof_end(s);
  return check_launch(what);
}

// debugging aid: resident blocks per CU the runtime predicts for the main kernel variants (the fourth is wgrad.hip's)
int debug_occupancy(int* out4) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gather_gemm_glds2_kernel<128, 128, 2, 2, EPI_STATS>, 256, 0) != hipSuccess) return 1;
  out4[0] = n;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gather_gemm_kernel<128, 128, 2, 2, EPI_STATS>, 256, 0) != hipSuccess) return 1;
  out4[1] = n;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gather_gemm_glds2_kernel<256, 64, 4, 1, EPI_STATS>, 256, 0) != hipSuccess) return 1;
  out4[2] = n;
  return wgrad_debug_occupancy(&out4[3]);
}

// Wt[ci][t][co] = W[co][t][ci]   (dgrad wants the contraction index co contiguous)
__global__ __launch_bounds__(256) void transpose_w_kernel(const float* __restrict__ W, float* __restrict__ Wt, int Co, int T, int Ci) {
  __shared__ float tile[32][33];
  const int t = blockIdx.z;
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    tile[r][tx] = (co < Co && ci < Ci) ? W[((long long)co * T + t) * Ci + ci] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < Ci && co < Co) Wt[((long long)ci * T + t) * Co + co] = tile[tx][r];
  }
}

// Every dgrad weight image of a network in ONE launch (the engine ran one 5 us transpose per conv layer and step: 52 launches for
// ResNet-50). tab[l] = {w_off, wt_off, Co, T, Ci}: Wt_l[ci][t][co] = W_l[co][t][ci] with W_l at params + w_off and Wt_l at
// wt + wt_off (elements of the output type); tile0[l] = first 32 x 32 tile (block) of layer l, tile0[n] = grid size.
template <class OT>
__global__ __launch_bounds__(256) void transpose_w_all_kernel(const float* __restrict__ params, OT* __restrict__ wt,
                                                               const WtEntry* __restrict__ tab, const int* __restrict__ tile0, int n) {
  __shared__ float tile[32][33];
  int lo = 0, hi = n - 1;                 // last l with tile0[l] <= blockIdx.x (block-uniform binary search)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const WtEntry e = tab[lo];
  const int local = blockIdx.x - tile0[lo];
  const int tci = (e.Ci + 31) / 32, tco = (e.Co + 31) / 32;
  const int ci0 = (local % tci) * 32, co0 = ((local / tci) % tco) * 32, t = local / (tci * tco);
  const float* W = params + e.w_off;
  OT* Wt = wt + e.wt_off;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    tile[r][tx] = (co < e.Co && ci < e.Ci) ? W[((long long)co * e.T + t) * e.Ci + ci] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < e.Ci && co < e.Co) Wt[((long long)ci * e.T + t) * e.Co + co] = (OT)tile[tx][r];
  }
}

int launch_transpose_w_all(const float* params, void* wt, const WtEntry* tab, const int* tile0, int n, int tiles, int dt, hipStream_t s) {
  if (n <= 0 || tiles <= 0) return 0;
  if (dt == DT_BF16)
    hipLaunchKernelGGL((transpose_w_all_kernel<bf16_t>), dim3(tiles), dim3(256), 0, s, params, static_cast<bf16_t*>(wt), tab, tile0, n);
  else
    hipLaunchKernelGGL((transpose_w_all_kernel<float>), dim3(tiles), dim3(256), 0, s, params, static_cast<float*>(wt), tab, tile0, n);
  return check_launch("transpose_w_all");
}

int launch_transpose_w(const float* W, float* Wt, int Co, int T, int Ci, hipStream_t s) {
  hipLaunchKernelGGL(transpose_w_kernel, dim3(ceil_div(Ci, 32), ceil_div(Co, 32), T), dim3(256), 0, s, W, Wt, Co, T, Ci);
  return check_launch("transpose_w");
}

}  // namespace r3m
