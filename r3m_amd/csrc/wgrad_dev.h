// r3m_amd — device code shared by the weight-gradient kernels (wgrad.hip, wgrad_win.hip, wgrad_bf16.hip): what every kernel of the
// family does around its K loop. The K loops themselves (fp32: scalar cursor walk; bf16: per-lane additive walk; window kernel:
// padding masks; all-taps kernel: register masks) are the kernels and stay in their files.
// A piece lives here only where each kernel keeps its registers, LDS, occupancy, scratch 0 and instruction counts with it
// (profiles/wgrad_unify_isa.txt).
#pragma once
#include "common.h"
#include "conv_dev.h"

namespace r3m {

// the 128 x 128 tile (else 64 x 64): both channel counts are multiples of 128
static inline bool wg_wide(int Co, int Ci) { return (Co % 128 == 0) && (Ci % 128 == 0); }

// What a block works on. The launch is 1-D, p.gx blocks per split: tile-major, the `groups` tap groups of one (co, ci) tile are
// neighbours (they re-read the same dY rows); by = split index, so consecutive logical blocks read the same rows.
struct WgBlock {
  int by, grp;       // split, tap group of the tile
  int co0, ci0;      // first channels of the tile
  int ms, me;        // GEMM rows [ms, me) of the split
};
// PIN: the block coordinates are uniform, but the divisions are expanded on the vector unit; wgrad_rowwin_kernel says so
// (readfirstlane), or everything it derives from them — descriptors, the padding-mask walk — stays in vector registers. The other
// kernels keep what the compiler picks.
template <int BMt, int BNt, bool PIN>
__device__ __forceinline__ WgBlock wg_block(const WgradParams& p, int groups) {
  auto pin = [](int v) __attribute__((always_inline)) { return PIN ? __builtin_amdgcn_readfirstlane(v) : v; };
  const int lid = p.xcd ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int bx = lid % p.gx;
  WgBlock b;
  b.by = lid / p.gx;
  b.grp = pin(bx % groups);
  const int tile = bx / groups;
  const int tn_ = tile % p.tilesN, tm_ = tile / p.tilesN;
  b.co0 = pin(tm_ * BMt);
  b.ci0 = pin(tn_ * BNt);
  b.ms = pin(b.by * p.rows_per_split);
  b.me = min(p.M, b.ms + p.rows_per_split);
  return b;
}

// accumulator clear
template <int NT, int TM, int TN>
__device__ __forceinline__ void wg_clear(f32x16 (&acc)[NT][TM][TN]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][a][b][r] = 0.f;
}

// Buffer descriptor of operand rows that are linear in m (dY; X of 1x1 / stride-1 layers and of the shared window): rows
// [r0 + BK step, r1) of a [rows][ld] tensor of ESZ-byte elements, seen from column col0. Per-lane offsets are constants; a K step
// moves the base by BK rows and shrinks the byte count on the scalar unit — rows past r1 fall off the descriptor and read zeros.
struct WgRows {
  const char* base;
  int left, stepb;     // bytes to the end of the rows, bytes per K step
  __device__ __forceinline__ void advance() {
    base += stepb;
    left = left > stepb ? left - stepb : 0;
  }
};
template <int ESZ>
__device__ __forceinline__ WgRows wg_rows(const void* t, int r0, int r1, int ld, int col0, int bk) {
  WgRows d;
  d.base = reinterpret_cast<const char*>(t) + ((long long)r0 * ld + col0) * ESZ;
  d.left = (int)(((long long)(r1 - r0) * ld - col0) * ESZ);      // (host: a split spans < 2 GiB)
  d.stepb = bk * ld * ESZ;
  return d;
}

// A block's result into its split's partial slab [Co][T][Ci]: taps tap0 .. tap0 + NT - 1. Wave layouts of the 32 x 32 MFMA tiles
// acc[.][TM][TN] (lane -> lrow = lane & 31, lh = lane >> 5):
//   INTERLEAVED (fp32 128 x 128, TM = 4, TN = 1): waves 1 x 4, MFMA tile tm owns channels co0 + 4 i + tm;
//   else waves 2 x 2 of (32 TM) x (32 TN): 32 x 32 (64-wide tiles) or 64 x 64 (bf16 128 x 128).
// CHECK: ragged tiles (fp32 per-tap / kernel-row forms); the others only run on whole tiles.
// (One call for all taps, lrow / lh from the caller: a per-tap helper, or one that derives them from the lane, cost the 128-wide
// kernel-row kernels up to 41 registers and wgrad_glds_kernel<128, 128, 16, 3> 52 bytes of scratch.)
template <bool INTERLEAVED, bool CHECK, int NT, int TM, int TN>
__device__ __forceinline__ void wg_store(const WgradParams& p, const WgBlock& b, int T, int tap0, int wm, int wn, int lrow, int lh,
                                         const f32x16 (&acc)[NT][TM][TN]) {
  float* out = p.out + (long long)b.by * p.Co * T * p.Ci;
#pragma unroll
  for (int tp = 0; tp < NT; ++tp)
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rho = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int co = INTERLEAVED ? b.co0 + 4 * rho + tm : b.co0 + (wm * TM + tm) * 32 + rho;
        if (CHECK && co >= p.Co) continue;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          const int ci = b.ci0 + (wn * TN + tn) * 32 + lrow;
          if (!CHECK || ci < p.Ci) out[((long long)co * T + tap0 + tp) * p.Ci + ci] = acc[tp][tm][tn][r];
        }
      }
}

}  // namespace r3m
