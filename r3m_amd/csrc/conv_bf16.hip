// r3m_amd — bf16-activation convolution path for gfx950 (BASELINE configs[2], [4]: "bf16"), forward and input gradient: the same
// implicit GEMMs as conv.hip with bf16 operands in HBM/LDS, fp32 accumulation on v_mfma_f32_32x32x16_bf16, fp32 BatchNorm partials
// taken from the accumulators. Master weights, optimizer state and every per-channel statistic stay fp32 (r3m_amd/encoder.py
// precision="bf16" is the mixed-precision counterpart of torch.autocast around the reference's encoder call,
// r3m/models/models_r3m.py:99; the reference itself trains in fp32). The fp32 weight gradients of this path are in wgrad_bf16.hip.
//
//   gather_gemm_bf16_kernel : forward / dgrad. LDS rows are 64 bf16 = 128 B, the very byte image of the fp32 kernel
//       (8 rows per global_load_lds instruction, 16-byte slots XOR-swizzled by (row>>1)&7), so the fragment of MFMA step g
//       is ONE ds_read_b128 = 8 consecutive k of one row — exactly the 32x32x16 operand layout (k = 8*(lane>>5)..+7).
//   conv3x3_halo_bf16_kernel : 3x3 / stride 1 / pad 1 with one staged window per tile instead of nine tap tiles.
//
// launch_gather_gemm_bf16 = requirements -> gg16_route (a pure function of the launch) -> switch (route). Route numbers are public
// (r3m_debug_conv_route):
//   30  gather_gemm_bf16_kernel    everything the routes below leave
//   31  conv3x3_halo_bf16_kernel   3x3 / stride 1 / pad 1 where the kernel-row kernel does not apply (or is switched off)
//   32  conv_row16.hip             persistent kernel-row kernel: 3x3 / stride 1 / pad 1, 128-multiple-wide or 64-wide outputs
//   33  conv_pw16.hip              probe builds only: persistent warp-specialised kernel (dense / parity-strided output rows)
// Also here: the two bf16 weight images (convert_bf16_kernel: forward, transpose_w_bf16_kernel: dgrad).
#include "common.h"
#include "conv_dev.h"
#include <cstdlib>
#include <cstring>

namespace r3m {

// =====================================================================================================
// gather-GEMM on bf16 operands. Block BM x BN, K tiles of BK elements (one LDS row per GEMM row), WM x WN waves.
// LDS: a ring of NST stages of {A[BM][BK], B[BN][BK]} bf16 (dynamic LDS). Tile t + NST - 1 is issued right after the barrier that
// publishes tile t (all DMA pieces at once: with the 16x faster MFMA there is no issue cost worth hiding), so up to NST - 1 tiles
// are in flight per block; a wave waits only for ITS pieces of the oldest tile (s_waitcnt vmcnt(pieces of the newer tile), loads
// retire in order). BK = 64: 128-byte rows, 8 rows per DMA instruction, 16-byte slots swizzled by (row>>1)&7; BK = 32: 64-byte
// rows, 16 rows per instruction, slots swizzled by (row>>2)&3 — also conflict-free for ds_read_b128. Configurations in use
// (launch_gather_gemm_bf16 picks per shape):
//   4 waves, 2 stages, BK = 64 (64-80 KB: 2 blocks/CU)   — main-loop-bound launches: 3x3 convs, contracting 1x1 convs
//   4 waves, 2 stages, BK = 32 (ring 32-40 KB <= the epilogue slab: 3-4 blocks/CU) — expanding 1x1 convs, read-modify-write epilogues
//   4 waves, 1 stage,  BK = 64 (launches with ONE K tile: 1x1 convs with Cin = 64; LDS = the epilogue slab)
//   experiments: 256x128 tile (R3M_BF16_BIG), 8 waves with a 3-stage ring at 1 block/CU (R3M_BF16_RING: the L2 -> LDS DMA path
//     delivers 17 TB/s with 8 waves x 8 KB outstanding per CU, tools/micro/l2dma.hip, but one block per CU loses more in uncovered
//     prologue/epilogue than the deeper ring wins) — measurements in DESIGN.md section 5
// =====================================================================================================
//
// Register budget: the configurations whose LDS is just the 37-40 KB epilogue slab (32-wide K tiles; single stage) can share a CU
// three or four ways, but left alone the compiler gives the plain-store epilogue 117-152 VGPRs + 64 AGPRs = two waves per SIMD.
// __launch_bounds__'s second argument states the blocks per CU the kernel is budgeted for (168 registers per lane for three, 128
// for four — the latter with 8-56 bytes of scratch in the epilogue, still the faster choice for the 128x128 tile).
#ifndef R3M_GG16_OCC_WIDE
#define R3M_GG16_OCC_WIDE 4      // 128x128 tile (0 = compiler's choice)
#endif
#ifndef R3M_GG16_OCC_NARROW
#define R3M_GG16_OCC_NARROW 3    // 256x64 tile
#endif
template <int BM, int BN, int WM, int WN, int EPI, int NST, int BK = 64>
__global__ __launch_bounds__(WM * WN * 64, (BM == 256 && BN == 128) ? (BK == 32 ? 2 : 1)
                                           : !(BK == 32 || NST == 1) ? 1
                                           : (BN == 128 ? (R3M_GG16_OCC_WIDE ? R3M_GG16_OCC_WIDE : 1) : (R3M_GG16_OCC_NARROW ? R3M_GG16_OCC_NARROW : 1)))
void gather_gemm_bf16_kernel(const GatherGemmParams p) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int RB = BK * 2;                             // bytes per LDS row
  constexpr int RPI = 1024 / RB;                         // rows per DMA instruction (8 or 16)
  constexpr int SPR = RB / 16;                           // 16-byte slots per row (8 or 4)
  constexpr int NG = BK / 16;                            // MFMA K groups per tile (4 or 2)
  constexpr int AJ = BM / (RPI * NW), BJ = BN / (RPI * NW);  // DMA instructions per wave per tile
  static_assert(BK == 64 || BK == 32, "K tile of 64 or 32");
  static_assert(AJ * RPI * NW == BM && BJ * RPI * NW == BN, "every wave stages whole DMA row groups");
  static_assert(NST >= 1 && NST <= 3, "ring of 1 (single K tile launches only), 2 or 3 stages");
  constexpr int NP = AJ + BJ;
  constexpr int STAGE = (BM + BN) * RB;                  // bytes
  extern __shared__ __attribute__((aligned(128))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int gridN = (p.Nc + BN - 1) / BN;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = lid / gridN, nt = lid % gridN;
  const int m0 = mt * BM, n0 = nt * BN;
  const char* Ab = reinterpret_cast<const char*>(p.A);
  const char* Bb = reinterpret_cast<const char*>(p.B);

  const int srow = lane / SPR, pslot = lane % SPR;
  auto swz = [](int r) __attribute__((always_inline)) { return BK == 64 ? ((r >> 1) & 7) : ((r >> 2) & 3); };
  const int Hb = p.simple_rows ? 1 : p.Hi, Wb = p.simple_rows ? 1 : p.Wi;
  // Round 3: both operands arrive through buffer descriptors (conv_dev.h buf_dma16; see wgrad_bf16_kernel for the measurement that
  // motivated it: these kernels are instruction-issue-bound and the per-lane 64-bit source pointers were most of the vector work).
  //   weights: constant per-lane offset; the (tap, K chunk) offset is wave-uniform and rides in the instruction's scalar offset;
  //   activations: per-lane 32-bit offset relative to the frame of the tile's first row, recomputed only when the TAP changes
  //     (padding -> out of range -> zeros); the K chunk inside the tap is the scalar offset again.
  const long long imgA = (long long)p.Hi * p.Wi * p.Ci * 2;               // bytes per frame of A (simple rows: unused)
  const int hwg = p.Hg * p.Wg;
  const int nfirst = p.simple_rows ? 0 : (m0 < p.M ? m0 / hwg : 0);
  const char* a_base = p.simple_rows ? Ab + (long long)m0 * p.Ci * 2 : Ab + (long long)nfirst * imgA;
  int a_bytes;
  {
    const long long rest = p.simple_rows ? (long long)(p.M - m0) * p.Ci * 2 : (long long)(p.N - nfirst) * imgA;
    a_bytes = rest <= 0 ? 0 : (rest < (long long)BUF_OOB ? (int)rest : (int)BUF_OOB);
  }
  RowDesc ad[AJ];
  unsigned arel[AJ];                   // byte offset of the row's frame (simple rows: of the row) from a_base + swizzled slot, or BUF_OOB
  unsigned avoff[AJ];                  // offset of the current tap's pixel (per lane), refreshed by set_tap
  unsigned bvoff[BJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    const int r = wave * (BM / NW) + j * RPI + srow;
    const unsigned col = (unsigned)((pslot ^ swz(r)) * 16);
    const int m = m0 + r;
    ad[j] = decode_row(p, m);
    if (m >= p.M) arel[j] = BUF_OOB;
    else if (p.simple_rows) arel[j] = (unsigned)(r * p.Ci * 2) + col;
    else arel[j] = (unsigned)(m / hwg - nfirst) * (unsigned)imgA + col;
    avoff[j] = arel[j];
  }
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int r = wave * (BN / NW) + j * RPI + srow;
    const int n = min(n0 + r, p.Nc - 1);                  // columns past Nc are computed on a clamped row, never stored
    bvoff[j] = (unsigned)(n * p.T * p.Ci * 2) + (unsigned)((pslot ^ swz(r)) * 16);
  }
  const int b_bytes = p.Nc * p.T * p.Ci * 2;

  const int kpt = p.Ci / BK;          // K tiles per tap
  const int nk = p.ntaps * kpt;

  // issue cursor: the tile the next DMA pieces belong to
  int tap_n = 0, chunk_n = 0;
  int pack_cur = nk > 0 ? p.tap[0] : 0;
  int pack_next = p.ntaps > 1 ? p.tap[1] : pack_cur;
  auto set_tap = [&](int pack) __attribute__((always_inline)) {
    if (p.simple_rows) return;
    const int dy = (pack << 24) >> 24, dx = (pack << 16) >> 24;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int iy = ad[j].iy + dy, ix = ad[j].ix + dx;
      const bool in = ((unsigned)iy < (unsigned)Hb) && ((unsigned)ix < (unsigned)Wb) && (arel[j] < BUF_OOB);
      avoff[j] = in ? arel[j] + (unsigned)((iy * p.Wi + ix) * p.Ci * 2) : BUF_OOB;
    }
  };
  if (nk > 0) set_tap(pack_cur);
  auto advance = [&]() __attribute__((always_inline)) {
    if (++chunk_n == kpt) {
      chunk_n = 0;
      ++tap_n;
      pack_cur = pack_next;
      pack_next = p.tap[min(tap_n + 1, p.ntaps - 1)];
      set_tap(pack_cur);
    }
  };
  // one DMA piece of the cursor's tile into ring slot `stage`
  auto issue_piece = [&](int stage, auto pc_c) __attribute__((always_inline)) {
    constexpr int pc = decltype(pc_c)::value;
    const int c0b = chunk_n * RB;
    unsigned char* la = smem + stage * STAGE + wave * (BM / NW) * RB;
    unsigned char* lb = smem + stage * STAGE + BM * RB + wave * (BN / NW) * RB;
    if constexpr (pc < AJ) {
      constexpr int j = pc;
      if (R3M_PROBE(p) & 24) {
        const int dy = (pack_cur << 24) >> 24, dx = (pack_cur << 16) >> 24;
        if ((R3M_PROBE(p) & 8) && dx != 0) return;     // probe 8: stage the A tile of the centre-column taps only (bytes-per-flop what-if)
        if ((R3M_PROBE(p) & 16) && (dx != 0 || dy != 0)) return;   // probe 16: ... of the centre tap only
      }
      buf_dma16(a_base, a_bytes, la + j * 1024, avoff[j], c0b);
    } else {
      constexpr int j = pc - AJ;
      const int wt = pack_cur >> 16;
      buf_dma16(Bb, b_bytes, lb + j * 1024, bvoff[j], wt * p.Ci * 2 + c0b);
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
  const int xr = swz(lrow);           // tile row offsets are multiples of 32: the swizzle key only depends on lrow
  int goff[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) goff[g] = ((2 * g + lh) ^ xr) * 16;
  const unsigned char* fragA0 = smem + (wm * TM * 32 + lrow) * RB;
  const unsigned char* fragB0 = smem + BM * RB + (wn * TN * 32 + lrow) * RB;

  // prologue: tiles 0 .. NST-2 (NST == 1: the launch has ONE K tile — 1x1 convs with Cin = 64 — and it is simply loaded; the
  // block then needs 37 instead of 64 KB of LDS, so three blocks share a CU instead of two)
  int istage = 0;                         // ring slot the cursor's tile goes to
  if (NST == 1 && nk > 0) static_for<NP>([&](auto pc) __attribute__((always_inline)) { issue_piece(0, pc); });
#pragma unroll
  for (int t = 0; t < NST - 1; ++t) {
    if (t < nk) {
      static_for<NP>([&](auto pc) __attribute__((always_inline)) { issue_piece(istage, pc); });
      advance();
      istage = (istage + 1 == NST) ? 0 : istage + 1;
    }
  }
  int cstage = 0;                         // ring slot of the tile being multiplied
  for (int kt = 0; kt < nk; ++kt) {
    // my pieces of tile kt have landed; the pieces of one newer tile (NST == 3) may still be in flight
    if (NST == 3 && kt + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // everyone's have; and everyone is done reading ring slot istage
    const bool more = NST > 1 && (kt + NST - 1 < nk) && !(R3M_PROBE(p) & 2);   // probe 2: no DMA after the prologue
    const unsigned char* fa = fragA0 + cstage * STAGE;
    const unsigned char* fb = fragB0 + cstage * STAGE;
    // all DMA pieces right after the barrier: with the 16x faster MFMA there is no issue cost worth hiding, and the earlier
    // the loads leave the sooner they land (+2..8 % over spreading them between the MFMA groups; probe 4 = spread)
    const bool clustered = (R3M_PROBE(p) & 4) == 0;
    if (more && clustered) static_for<NP>([&](auto pc) __attribute__((always_inline)) { issue_piece(istage, pc); });
    static_for<NG>([&](auto g_c) __attribute__((always_inline)) {
      constexpr int g = decltype(g_c)::value;
      bf16x8 a[TM], b[TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) a[t] = *reinterpret_cast<const bf16x8*>(fa + t * 32 * RB + goff[g]);
#pragma unroll
      for (int t = 0; t < TN; ++t) b[t] = *reinterpret_cast<const bf16x8*>(fb + t * 32 * RB + goff[g]);
      if (more && !clustered) {   // DMA pieces of tile kt + NST - 1, spread over the MFMA groups
        constexpr int P0 = g * NP / NG, P1 = (g + 1) * NP / NG;
        static_for<P1 - P0>([&](auto q_c) __attribute__((always_inline)) {
          issue_piece(istage, std::integral_constant<int, P0 + decltype(q_c)::value>{});
        });
      }
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
    });
    if (more) {
      advance();
      istage = (istage + 1 == NST) ? 0 : istage + 1;
    }
    cstage = (cstage + 1 == NST) ? 0 : cstage + 1;
  }
  __syncthreads();   // all fragment reads done before the epilogue reuses the stages

  if (R3M_PROBE(p) & 1) {   // probe 1: no epilogue (one store keeps the accumulators alive)
    if (acc[0][0][0] + acc[TM - 1][TN - 1][3] == 123.456f) reinterpret_cast<float*>(p.out)[0] = 1.f;
    return;
  }
  // a 256-row tile writes one partial row per 128-row half (same partial geometry as the 128-row tiles)
  if (EPI & EPI_STATS) gg_stats<BM, BN, WM, WN, (BM == 256 && BN == 128)>(p, acc, reinterpret_cast<float*>(smem), n0, mt);
  // the launcher sizes the dynamic LDS as max(ring, epilogue slabs): with NST == 1 the slabs are the larger
  constexpr int SMEM_F = (NST * STAGE < 40960 ? 40960 : NST * STAGE) / 4;
  if ((p.Nc & 7) == 0) gg_store_bf16<BM, BN, WM, WN, EPI, SMEM_F>(p, acc, reinterpret_cast<float*>(smem), m0, n0);
  else gg_epilogue<BM, BN, WM, WN, EPI & ~EPI_STATS, SMEM_F, bf16_t>(p, acc, reinterpret_cast<float*>(smem), m0, n0, mt);
}

// =====================================================================================================
// 3x3 / stride 1 / pad 1 convolutions (forward and dgrad) with a HALO tile: the nine taps of a tile of BM consecutive output
// pixels read input pixels m0 - (W+1) .. m0 + BM - 1 + (W+1) — one window of BM + 2W + 2 rows instead of nine BM-row tiles. The
// gather kernel above stages 9 x (BM + BN) rows per 64-channel chunk and is bound by exactly that L2 -> LDS staging rate
// (DESIGN.md section 5); here a chunk stages the window once plus nine BN-row weight tiles (0.57x the rows at 14x14 / 128x128).
//   LDS: [window of HRI x 1 KiB][1 KiB with a zero row][2 weight stages of BN x 128 B]; same 128-byte swizzled rows.
//   A fragment of tap (dy, dx) = halo rows shifted by dy*W + dx (the swizzle key follows the shifted row); a lane whose pixel
//   has no (y+dy, x+dx) inside the image reads the zero row instead -> the border arithmetic of the gather kernel (zero
//   contributions) without per-tap staging. Rows >= M read zeros for every tap (BatchNorm partials rely on that).
//   Weight tiles: ring of 2, one tile per (chunk, tap) step. ONE window buffer, reloaded between chunks: a second buffer (next
//   window arriving under the current chunk's taps) measured slower than the third block per CU the smaller footprint allows
//   (14x14 x 256: 0.372 vs 0.363 ms, 7x7 x 512: 0.304 vs 0.277 ms; the gather kernel: 0.440 / 0.369).
// =====================================================================================================
template <int BM, int BN, int WM, int WN, int EPI>
__global__ __launch_bounds__(256, BM / WM > 64 ? 2 : 1) void conv3x3_halo_bf16_kernel(const GatherGemmParams p, const int hri) {
  static_assert(WM * WN == 4 && BN / WN == 64 && (BM / WM == 64 || BM / WM == 128), "four waves, 64 or 128 rows x 64 columns each");
  constexpr int TM = BM / WM / 32, TN = 2;
  constexpr int BJ = BN / 32;                        // weight DMA instructions per wave per tile
  constexpr int WSTAGE = BN * 128;                   // bytes
  extern __shared__ __attribute__((aligned(128))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int gridN = (p.Nc + BN - 1) / BN;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = lid / gridN, nt = lid % gridN;
  const int m0 = mt * BM, n0 = nt * BN;
  const char* Ab = reinterpret_cast<const char*>(p.A);
  const char* Bb = reinterpret_cast<const char*>(p.B);
  const int W = p.Wi, HW = p.Hi * p.Wi;
  const int halo_bytes = hri * 1024;
  unsigned char* zrow = smem + halo_bytes;                            // 128 zero bytes (1 KiB reserved)
  unsigned char* wring = zrow + 1024;
  if (tid < 16) *reinterpret_cast<uint4*>(zrow + tid * 16) = make_uint4(0u, 0u, 0u, 0u);   // 256 zero bytes: see the fragment addressing below

  const int srow = lane >> 3, pslot = lane & 7;
  const long long hb = (long long)m0 - (W + 1);                        // pixel staged in halo row 0
  // Round 3: buffer descriptors (see gather_gemm_bf16_kernel). Window rows: offsets relative to the first in-tensor pixel of the
  // window, rows before the tensor get an out-of-range offset, rows past it fall off the descriptor; the 64-channel chunk is the
  // scalar offset. Weights: constant per-lane offset, (tap, chunk) in the scalar offset.
  const long long hb0 = hb > 0 ? hb : 0;
  const char* a_base = Ab + hb0 * p.Ci * 2;
  int a_bytes;
  {
    const long long rest = ((long long)p.M - hb0) * p.Ci * 2;
    a_bytes = rest <= 0 ? 0 : (rest < (long long)BUF_OOB ? (int)rest : (int)BUF_OOB);
  }
  const unsigned hcol = (unsigned)pslot;                               // physical slot; the logical one depends on the row
  // DMA instruction i of the window of chunk c: halo rows 8i .. 8i+7
  auto issue_halo = [&](int c, int i) __attribute__((always_inline)) {
    const int hr = 8 * i + srow;
    const long long px = hb + hr;
    const unsigned voff = px >= hb0 ? (unsigned)((int)(px - hb0) * p.Ci * 2) + ((hcol ^ (unsigned)((hr >> 1) & 7)) * 16u) : BUF_OOB;
    buf_dma16(a_base, a_bytes, smem + i * 1024, voff, c * 128);
  };
  unsigned bvoff[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int r = wave * (BN / 4) + j * 8 + srow;
    const int n = min(n0 + r, p.Nc - 1);
    bvoff[j] = (unsigned)(n * p.T * p.Ci * 2) + (unsigned)((pslot ^ ((r >> 1) & 7)) * 16);
  }
  const int b_bytes = p.Nc * p.T * p.Ci * 2;
  auto issue_w = [&](int c, int pack, int stage) __attribute__((always_inline)) {
    const int wt = pack >> 16;
    unsigned char* lb = wring + stage * WSTAGE + wave * (BN / 4) * 128;
#pragma unroll
    for (int j = 0; j < BJ; ++j) buf_dma16(Bb, b_bytes, lb + j * 1024, bvoff[j], wt * p.Ci * 2 + c * 128);
  };

  // per-lane rows of the two A row tiles: halo row of the centre tap and a 9-bit validity mask (bit = tap position in p.tap[])
  const int lrow = lane & 31, lh = lane >> 5;
  int crow[TM];
  unsigned vmask[TM];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int r = wm * (BM / WM) + t * 32 + lrow;
    crow[t] = r + W + 1;
    const int m = m0 + r;
    unsigned v = 0;
    if (m < p.M) {
      const int rem = m % HW;
      const int y = rem / W, x = rem - y * W;
      for (int k = 0; k < 9; ++k) {
        const int pk = p.tap[k];
        const int dy = (pk << 24) >> 24, dx = (pk << 16) >> 24;
        if ((unsigned)(y + dy) < (unsigned)p.Hi && (unsigned)(x + dx) < (unsigned)W) v |= 1u << k;
      }
    }
    vmask[t] = v;
  }
  const int zoff = (int)(zrow - smem);
  int goffb[4];
  const int xrb = (lrow >> 1) & 7;
#pragma unroll
  for (int g = 0; g < 4; ++g) goffb[g] = ((2 * g + lh) ^ xrb) * 16;
  const unsigned char* fragB0 = wring + (wn * 64 + lrow) * 128;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int nc = p.Ci >> 6;
  // prologue: window of chunk 0, weight tile (0, tap 0)
  for (int i = wave; i < hri; i += 4) issue_halo(0, i);
  issue_w(0, p.tap[0], 0);
  int stage = 0;
  for (int c = 0; c < nc; ++c) {
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const bool last_tap = k == 8;     // next weight tile
      if (!last_tap) issue_w(c, p.tap[k + 1], stage ^ 1);
      else if (c + 1 < nc) issue_w(c + 1, p.tap[0], stage ^ 1);
      const int pk = p.tap[k];
      const int shift = ((pk << 24) >> 24) * W + ((pk << 16) >> 24);
      int abase[TM], akey[TM];
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const bool ok = (vmask[t] >> k) & 1u;
        const int rv = crow[t] + shift;
        // Round 5: a masked lane reads its zeros at the SAME position of the 256-byte bank window its real row would have used
        // (row parity picks the 128-byte half, the swizzled slot the 16 bytes): the 16 lanes of a ds_read_b128 group then still hit
        // 16 distinct positions. With ONE zero row at a fixed position a masked lane collided with whichever lane owned that slot:
        // PMC showed 25 % of this kernel's LDS cycles as bank conflicts at 14 x 14 (profiles/r05_pw16_pmc_v5_halo.csv).
        abase[t] = ok ? rv * 128 : zoff + (rv & 1) * 128;
        akey[t] = (rv >> 1) & 7;
      }
      const unsigned char* fb = fragB0 + stage * WSTAGE;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x8 a[TM], b[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) a[t] = *reinterpret_cast<const bf16x8*>(smem + abase[t] + (((2 * g + lh) ^ akey[t]) * 16));
#pragma unroll
        for (int t = 0; t < TN; ++t) b[t] = *reinterpret_cast<const bf16x8*>(fb + t * 32 * 128 + goffb[g]);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
      }
      stage ^= 1;
    }
    if (c + 1 < nc) {
      __syncthreads();                                 // every wave is done with this chunk's window
      for (int i = wave; i < hri; i += 4) issue_halo(c + 1, i);
    }
  }
  __syncthreads();   // all fragment reads done before the epilogue reuses the LDS
  // a 256 x 128 tile writes one partial row per 128-row half (the partial geometry of the 128-row tiles)
  if (EPI & EPI_STATS) gg_stats<BM, BN, WM, WN, (BM == 256 && BN == 128)>(p, acc, reinterpret_cast<float*>(smem), n0, mt);
  gg_store_bf16<BM, BN, WM, WN, EPI, 40960 / 4>(p, acc, reinterpret_cast<float*>(smem), m0, n0);
}

// LDS bytes of the halo kernel for a tile of BM pixels at image width W
static inline int halo_lds_bytes(int BM, int BN, int W) {
  const int hri = ceil_div(BM + 2 * W + 2, 8);
  const int b = hri * 1024 + 1024 + 2 * BN * 128;
  return b < 40960 ? 40960 : b;
}

template <int BM, int BN, int WM, int WN, int EPI>
static int halo_launch_one(const GatherGemmParams& p, hipStream_t s) {
  const int hri = ceil_div(BM + 2 * p.Wi + 2, 8);
  const int lds = halo_lds_bytes(BM, BN, p.Wi);
  auto kern = conv3x3_halo_bf16_kernel<BM, BN, WM, WN, EPI>;
  static DynLdsOptIn optin;
  if (int e = ensure_dyn_lds(optin, reinterpret_cast<const void*>(kern), lds, "conv3x3_halo(bf16)")) return e;
  const int grid = ceil_div(p.M, BM) * ceil_div(p.Nc, BN);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, p, hri);
  return 0;
}

template <int BM, int BN, int WM, int WN>
static int halo_launch(const GatherGemmParams& p, hipStream_t s) {
  const int rc = gg16_epi_switch<false>(p.flags, [&](auto e) { return halo_launch_one<BM, BN, WM, WN, decltype(e)::value>(p, s); });
  if (rc < 0) { set_last_error("conv3x3_halo(bf16): unsupported epilogue flag combination %d", p.flags); return 1; }
  return rc;
}

// 3x3 stride-1 launches go through the halo kernel; wide launches with enough rows use the 256 x 128 tile (0.55x the staged rows
// of the 128 x 128 halo tile again: 14x14 x 256 at 1280 frames 0.317 ms against 0.380, the gather kernel 0.450).
// R3M_BF16_HALO=0: gather kernel; =2: 128-row tiles only; =4: 256-row tile whatever M (tests)
static int gg16_halo() {
  const int v = R3M_ENV_INT("R3M_BF16_HALO", 1);
  return v;
}

static bool halo_eligible(const GatherGemmParams& p) {
  if (p.ntaps != 9 || p.simple_rows || p.is != 1 || p.os != 1 || p.ooy != 0 || p.oox != 0) return false;
  if (p.Hg != p.Hi || p.Wg != p.Wi || p.Ho != p.Hi || p.Wo != p.Wi || (p.Ci & 63) || (p.Nc & 7)) return false;
  if (!(p.Nc % 128 == 0 || p.Nc == 64)) return false;
  if (!gg16_epilogue_built(p.flags, false)) return false;
  for (int k = 0; k < 9; ++k)
    if (p.dy[k] < -1 || p.dy[k] > 1 || p.dx[k] < -1 || p.dx[k] > 1) return false;
  return true;
}

// tile rows of the halo launch (0: the window does not fit the LDS -> gather kernel)
static int halo_tile_rows(const GatherGemmParams& p) {
  if (p.Nc == 64) return halo_lds_bytes(256, 64, p.Wi) <= 160 * 1024 ? 256 : 0;
  const int h = gg16_halo();
  const int min_m = h == 4 ? 0 : 65536;      // 7x7 x 512 at 1280 frames (M = 62720) measured the same either way
  if (h != 2 && p.M >= min_m && halo_lds_bytes(256, 128, p.Wi) <= 80 * 1024) return 256;
  return halo_lds_bytes(128, 128, p.Wi) <= 160 * 1024 ? 128 : 0;
}

static int launch_halo(const GatherGemmParams& p, int rows, hipStream_t s) {
  if (p.Nc == 64) return halo_launch<256, 64, 4, 1>(p, s);
  return rows == 256 ? halo_launch<256, 128, 2, 2>(p, s) : halo_launch<128, 128, 2, 2>(p, s);
}

static inline bool gg_wide(int Nc) { return (Nc % 128) == 0; }

template <int BM, int BN, int WM, int WN, int EPI, int NST, int BK>
static int gg16_launch_one(const GatherGemmParams& p, int grid, hipStream_t s) {
  constexpr int slab = WM * WN * (BM / WM > 64 ? 64 : BM / WM) * (BN / WN + 8) * 2;   // bf16 epilogue slabs (64 rows per wave and pass)
  constexpr int slab32 = WM * WN * 32 * (BN / WN + 4) * 4;                  // fp32 slabs of the read-modify-write epilogues
  constexpr int tiles = NST * (BM + BN) * BK * 2;
  constexpr int lds = tiles > slab ? (tiles > slab32 ? tiles : slab32) : (slab > slab32 ? slab : slab32);
  auto kern = gather_gemm_bf16_kernel<BM, BN, WM, WN, EPI, NST, BK>;
  static DynLdsOptIn optin;         // > 64 KiB of dynamic LDS needs the opt-in once per kernel (and device)
  if (int e = ensure_dyn_lds(optin, reinterpret_cast<const void*>(kern), lds, "gather_gemm(bf16)")) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(WM * WN * 64), lds, s, p);
  return 0;
}

template <int BM, int BN, int WM, int WN, int NST, int BK = 64>
static int gg16_launch(const GatherGemmParams& p, int grid, hipStream_t s) {
  const int rc = gg16_epi_switch<true>(p.flags, [&](auto e) { return gg16_launch_one<BM, BN, WM, WN, decltype(e)::value, NST, BK>(p, grid, s); });
  if (rc < 0) { set_last_error("gather_gemm(bf16): unsupported epilogue flag combination %d", p.flags); return 1; }
  return rc;
}

// R3M_BF16_RING=n: use the 8-wave / 3-stage configuration for launches with >= n K tiles. Default 0 = never: measured on
// ResNet-50 shapes it LOSES 20-30 % to two co-resident 4-wave blocks (one block per CU leaves its prologue and epilogue
// uncovered, and the 2 x 4 wave layout reads 1.5x the LDS bytes per tile). Kept for experiments.
static int gg16_ring_min() {
  const int v = R3M_ENV_INT("R3M_BF16_RING", 0);
  return v;
}

// R3M_BF16_SINGLE=0 disables the single-stage configuration of one-K-tile launches
static bool gg16_single() {
  const int v = R3M_ENV_INT("R3M_BF16_SINGLE", 1);
  return v != 0;
}

// K tile width of a multi-tile launch. 32 (16 KB stages, THREE blocks per CU instead of two) wins where the epilogue is a large
// part of a block's life — the expanding 1x1 convs and everything with a read-modify-write epilogue: -10..-33 % per launch on
// ResNet-50 — because a third resident block covers it; 64 (half the barriers per K) wins by 3..16 % where the main loop
// dominates: K >= 4 N, i.e. the 3x3 convs and the contracting 1x1 convs (per-shape table measured in round 2: profiles/r02_*).
// The 256x64 tile's 3x3 launches are the exception (measured -4 % with 32). R3M_BF16_BK=32 / 64 forces one width.
static bool gg16_bk32(const GatherGemmParams& p, bool wide) {
  const int v = R3M_ENV_INT("R3M_BF16_BK", 0);
  if (v == 32) return true;
  if (v == 64) return false;
  const long long ktot = (long long)p.ntaps * p.Ci;
  const bool mainloop_bound = ktot >= 4LL * p.Nc && (wide || p.ntaps == 1);
  return !mainloop_bound;
}

// 256 x 128 block tile (waves 2 x 2, 128 x 64 per wave) for the main-loop-bound wide launches: a 64 x 64 wave tile reads
// (64 + 64) x 32 B of fragments per 4 MFMAs — with 8 waves per CU that is exactly the LDS's 128 B/clk, so those launches sat at
// ~35 % of the MFMA peak; 128 x 64 per wave needs 0.75x the fragment bytes per flop. R3M_BF16_BIG=0 disables, =64 uses 64-wide
// K tiles (96 KB ring, one block per CU) instead of 32-wide (48 KB, two blocks).
static int gg16_big() {
  const int v = R3M_ENV_INT("R3M_BF16_BIG", 0);
  return v;
}

// Which kernel family launch_gather_gemm_bf16 runs: a pure function of the launch parameters, the ONLY place the conditions are
// written (the launcher switches on it, r3m_debug_conv_route reports it without a GPU). The numbers are public.
enum : int { GG16_ROUTE_GATHER = 30, GG16_ROUTE_HALO = 31, GG16_ROUTE_ROW = 32, GG16_ROUTE_PW = 33 };
int gg16_route(const GatherGemmParams& p) {
  if (row16_eligible(p)) return GG16_ROUTE_ROW;     // round 6: 3x3 / stride-1 launches -> persistent kernel-row kernel (conv_row16.hip)
  if (gg16_halo() && halo_eligible(p) && pw16_form(p) != 3 && halo_tile_rows(p)) return GG16_ROUTE_HALO;   // (3: the persistent window form takes it)
  if (pw16_form(p)) return GG16_ROUTE_PW;           // dense / parity-strided output rows: the persistent warp-specialised kernel (conv_pw16.hip)
  return GG16_ROUTE_GATHER;
}

// Which epilogue flag combinations each bf16 route builds (conv_dev.h gg16_epi_switch; the probe-build persistent kernel
// conv_pw16.hip has no inference epilogue). What gather_gemm_fuses_affine answers from, as the fp32 branch from gg_route.
bool gg16_route_builds(int route, int flags) {
  if (route == GG16_ROUTE_GATHER) return gg16_epilogue_built(flags, true);
  return (route == GG16_ROUTE_HALO || route == GG16_ROUTE_ROW) && gg16_epilogue_built(flags, false);
}

// The gather route's choice of tile, ring depth and K tile width per shape (the table above gather_gemm_bf16_kernel): outputs that
// are a multiple of 128 wide run 128 x 128 tiles (experiments: 256 x 128, 8 waves), ...
static int gg16_launch_wide(const GatherGemmParams& p, hipStream_t s) {
  const int nk = p.ntaps * (p.Ci / 64);
  const int grid = ceil_div(p.M, 128) * ceil_div(p.Nc, 128);
  // R3M_BF16_BIG < 0: every multi-tile wide launch (tests)
  const bool big = gg16_big() < 0 ? nk >= 2 : gg16_big() != 0 && !gg16_bk32(p, true) && nk >= 4 && p.M >= 256 * 256;
  if (big) {
    const int gridb = ceil_div(p.M, 256) * ceil_div(p.Nc, 128);
    return gg16_big() == 64 ? gg16_launch<256, 128, 2, 2, 2, 64>(p, gridb, s) : gg16_launch<256, 128, 2, 2, 2, 32>(p, gridb, s);
  }
  if (gg16_ring_min() > 0 && nk >= gg16_ring_min()) return gg16_launch<128, 128, 2, 4, 3>(p, grid, s);
  if (gg16_ring_min() < 0) return gg16_launch<128, 128, 2, 4, 2>(p, grid, s);   // experiment: 8 waves, 2 stages (2 blocks/CU = 16 waves/CU)
  if (nk == 1 && gg16_single()) return gg16_launch<128, 128, 2, 2, 1>(p, grid, s);
#ifdef R3M_PROBES
  if (gg16_bk32(p, true) && R3M_ENV_INT("R3M_BF16_NST3", 0)) return gg16_launch<128, 128, 2, 2, 3, 32>(p, grid, s);   // 3-stage ring, 48 KB: 3 blocks/CU
#endif
  return gg16_bk32(p, true) ? gg16_launch<128, 128, 2, 2, 2, 32>(p, grid, s) : gg16_launch<128, 128, 2, 2, 2>(p, grid, s);
}

// ... every other width 256 x 64 tiles
static int gg16_launch_narrow(const GatherGemmParams& p, hipStream_t s) {
  const int nk = p.ntaps * (p.Ci / 64);
  const int grid = ceil_div(p.M, 256) * ceil_div(p.Nc, 64);
  if (gg16_ring_min() > 0 && nk >= gg16_ring_min()) return gg16_launch<256, 64, 4, 2, 3>(p, grid, s);
  if (gg16_ring_min() < 0) return gg16_launch<256, 64, 4, 2, 2>(p, grid, s);
  if (nk == 1 && gg16_single()) return gg16_launch<256, 64, 4, 1, 1>(p, grid, s);
  return gg16_bk32(p, false) ? gg16_launch<256, 64, 4, 1, 2, 32>(p, grid, s) : gg16_launch<256, 64, 4, 1, 2>(p, grid, s);
}

int launch_gather_gemm_bf16(const GatherGemmParams& p, hipStream_t s) {
  R3M_REQUIRE(p.Ci % 64 == 0, "gather_gemm(bf16): Ci=%d must be a multiple of 64", p.Ci);
  R3M_REQUIRE(p.Nc % 4 == 0, "gather_gemm(bf16): Nc=%d must be a multiple of 4", p.Nc);
  // every loader here addresses the weights (and a frame's worth of activations) through 32-bit buffer offsets
  R3M_REQUIRE((long long)p.Nc * p.T * p.Ci * 2 < (long long)BUF_OOB, "gather_gemm(bf16): weight tensor of %lld bytes exceeds the 32-bit buffer range",
              (long long)p.Nc * p.T * p.Ci * 2);
  R3M_REQUIRE(p.simple_rows || (long long)p.Hi * p.Wi * p.Ci * 2 < (long long)BUF_OOB, "gather_gemm(bf16): one frame of %lld bytes exceeds the 32-bit buffer range",
              (long long)p.Hi * p.Wi * p.Ci * 2);
  const int route = gg16_route(p);
  const bool wide = gg_wide(p.Nc);
  const double flops = 2.0 * (double)p.M * (double)p.Nc * (double)p.ntaps * p.Ci;
  // profiler class by tile width; the kernel-row route has always reported KC_GEMM_WIDE, also for Nc == 64: kept (launch CSVs stay comparable)
  prof_begin(wide || route == GG16_ROUTE_ROW ? KC_GEMM_WIDE : KC_GEMM_NARROW, flops, p.M, p.Nc, p.Ci, p.ntaps, s);
  int rc;
  const char* what;
  switch (route) {
    case GG16_ROUTE_ROW: rc = launch_conv3x3_row_bf16(p, s); what = "conv3x3_row_bf16"; break;
    case GG16_ROUTE_HALO: rc = launch_halo(p, halo_tile_rows(p), s); what = "conv3x3_halo_bf16"; break;
    case GG16_ROUTE_PW: rc = launch_pw16(p, s); what = "pw16_gemm"; break;
    default: rc = wide ? gg16_launch_wide(p, s) : gg16_launch_narrow(p, s); what = "gather_gemm_bf16"; break;   // GG16_ROUTE_GATHER
  }
  if (rc) { prof_abandon(); return rc; }      // a launcher that returned an error: no launch is counted
  if (prof_open()) prof_bytes(gather_gemm_alg_bytes(p, 2));
  prof_end(s);
  return check_launch(what);
}

// ---- weight images: fp32 master [Co][T][Ci] -> bf16 copy (forward) / bf16 [Ci][T][Co] (dgrad) ----
__global__ __launch_bounds__(256) void convert_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long long n4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) st4t(dst + i * 4, ld4t(src + i * 4));
}

int launch_convert_bf16(const float* src, void* dst, long long n, hipStream_t s) {
  R3M_REQUIRE(n % 4 == 0, "convert_bf16: n=%lld must be a multiple of 4", n);
  hipLaunchKernelGGL(convert_bf16_kernel, dim3(ceil_div(n / 4, 256)), dim3(256), 0, s, src, reinterpret_cast<bf16_t*>(dst), n / 4);
  return check_launch("convert_bf16");
}

__global__ __launch_bounds__(256) void transpose_w_bf16_kernel(const float* __restrict__ W, bf16_t* __restrict__ Wt, int Co, int T, int Ci) {
  // Wt[ci][t][co] = W[co][t][ci]; a 32 x 32 (co, ci) tile per block through LDS, both sides coalesced
  __shared__ float tile[32][33];
  const int t = blockIdx.z;
  const int co0 = blockIdx.y * 32, ci0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    tile[r][tx] = (co < Co && ci < Ci) ? W[((long long)co * T + t) * Ci + ci] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < Ci && co < Co) Wt[((long long)ci * T + t) * Co + co] = (bf16_t)tile[tx][r];
  }
}

int launch_transpose_w_bf16(const float* W, void* Wt, int Co, int T, int Ci, hipStream_t s) {
  hipLaunchKernelGGL(transpose_w_bf16_kernel, dim3(ceil_div(Ci, 32), ceil_div(Co, 32), T), dim3(256), 0, s, W,
                     reinterpret_cast<bf16_t*>(Wt), Co, T, Ci);
  return check_launch("transpose_w_bf16");
}

}  // namespace r3m
