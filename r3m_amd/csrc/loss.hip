// r3m_amd — the R3M objective on embeddings alle[B,5,D] (frame roles e0, eg, es0, es1, es2), forward + backward fused:
// LP norms, time-contrastive InfoNCE with permuted cross-clip negatives, and the language-alignment InfoNCE on the
// reward-head scores. Restates /root/reference/r3m/trainer.py:39-152 and R3M.sim (/root/reference/r3m/models/models_r3m.py:102-107):
//   * permutations are INPUTS (the reference draws them with torch.randperm on the CPU generator, trainer.py:87-91,136-137);
//     negatives are gathered through the permutation, their gradient returns through the inverse permutation (a gather,
//     so no atomics and a fixed summation order);
//   * InfoNCE keeps the reference's literal form -log(eps + e^{s+} / (eps + sum e^{s})), eps = 1e-8, no max-subtraction;
//   * ||a-b||_2 has sub-gradient 0 at a == b (as torch.linalg.norm does).
// The reference runs ~60 tiny latency-bound kernels plus ~10 .item() syncs here; this is 3 launches and one metrics array.
//
// The number of cross-clip negatives N is the reference's model.num_negatives (trainer.py:66,86-92 and :124,135-139), a launch
// argument here: 0 <= N <= LOSS_MAX_NEG. The cap is this file's (it sizes the shared tables below), the reference has none.
//   * TCN: 3 + 2N pairs per clip. Pair ids 0..2 = s02, s12, s01; 3 + k = neg0_k (es0 against es0[perm[2k]]); 3 + N + k = neg2_k
//     (es2 against es2[perm[2k+1]]). perm / iperm are [2N][B]. N = 0 with tcnweight > 0 is refused on the host: the reference
//     fails there (torch.stack of an empty list, trainer.py:140).
//   * language InfoNCE: 6 + 3N score rows, q = 6 + 3k + j the k-th permuted negative of head j.
//   * sums over negatives run left to right, k = 0..N-1, after the fixed terms; every per-pair reduction is the same fmaf chain and
//     block_sum whatever N is, so a result does not depend on how the negatives are grouped into passes.
#include "common.h"

namespace r3m {

constexpr float LOSS_EPS = 1e-8f;
constexpr int LOSS_MAX_NEG = 16;                    // = R3M_MAX_NEGATIVES (include/r3m_hip.h)
constexpr int NEG_PASS = 3;                         // negatives of es0 and of es2 reduced per pass of tcn_pairs_kernel
constexpr int MAX_PAIR = 3 + 2 * LOSS_MAX_NEG;      // 35
constexpr int MAX_TERM = 2 + 2 * LOSS_MAX_NEG;      // 34: similarity terms that touch one es0 / es2 row
constexpr int NCLIPM = 8;    // per-clip metric partials: sum||.||2, sum||.||1, sum||.||0, tcn_i, aligned_i, (3 spare)
static_assert(LOSS_MAX_NEG == 16, "include/r3m_hip.h states the cap as R3M_MAX_NEGATIVES 16");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* smem /* >= 4*NV floats */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) smem[wave * NV + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = smem[k] + smem[NV + k] + smem[2 * NV + k] + smem[3 * NV + k];
  __syncthreads();
}

struct TcnArgs {
  const float* alle;   // [B,5,D]
  const int* perm;     // [2N][B]: order of trainer.py:136-137 -> (es0-perm, es2-perm) for k = 0..N-1
  const int* iperm;    // [2N][B]: inverse permutations
  float* pair_stat;    // [B][3+2N][4]: l2dist: {dist,-,-,-}; cosine: {dot, na, nb, -}
  float* coef;         // [B][3+2N]: d full_loss / d sim
  float* rownorm;      // [B][5]
  float* clipm;        // [B][NCLIPM]
  float* dalle;        // [B,5,D]
  int B, D, N;
  int l2dist;
  float l2weight, l1weight, tcnweight;
};

// One reduction pass of pass A over row i: the NFIX fixed pairs (3 in the first pass, 0 after it), then negatives k0 .. k0 + NEG_PASS - 1
// of es0 and of es2. A pass whose last negatives lie past N - 1 reads the last real one again and drops the result. Thread 0 leaves
// every live pair's statistics in pair_stat and its similarity in sim_s[pair id].
template <int NFIX>
__device__ __forceinline__ void tcn_pair_pass(const TcnArgs& a, int i, int k0, const float* es0, const float* es1, const float* es2,
                                              float* smem, float* sim_s) {
  constexpr int NQ = NFIX + 2 * NEG_PASS;
  const int D = a.D, N = a.N;
  const float* n0p[NEG_PASS];
  const float* n2p[NEG_PASS];
#pragma unroll
  for (int k = 0; k < NEG_PASS; ++k) {
    const int kr = k0 + k < N ? k0 + k : N - 1;
    n0p[k] = a.alle + ((long long)a.perm[(2 * kr + 0) * a.B + i] * 5 + 2) * D;
    n2p[k] = a.alle + ((long long)a.perm[(2 * kr + 1) * a.B + i] * 5 + 4) * D;
  }
  float pv[NQ * 3];
#pragma unroll
  for (int k = 0; k < NQ * 3; ++k) pv[k] = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
    const float x0 = es0[d], x2 = es2[d];
    float pa[NQ], pb[NQ];
    if (NFIX) {
      const float x1 = es1[d];
      pa[0] = x2; pb[0] = x0;
      pa[1] = x2; pb[1] = x1;
      pa[2] = x1; pb[2] = x0;
    }
#pragma unroll
    for (int k = 0; k < NEG_PASS; ++k) {
      pa[NFIX + k] = x0; pb[NFIX + k] = n0p[k][d];
      pa[NFIX + NEG_PASS + k] = x2; pb[NFIX + NEG_PASS + k] = n2p[k][d];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (a.l2dist) {
        const float df = pa[q] - pb[q];
        pv[q * 3] = fmaf(df, df, pv[q * 3]);
      } else {
        pv[q * 3 + 0] = fmaf(pa[q], pb[q], pv[q * 3 + 0]);
        pv[q * 3 + 1] = fmaf(pa[q], pa[q], pv[q * 3 + 1]);
        pv[q * 3 + 2] = fmaf(pb[q], pb[q], pv[q * 3 + 2]);
      }
    }
  }
  block_sum<NQ * 3>(pv, smem);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int id = q;                                        // fixed pairs keep their ids
      if (q >= NFIX) {
        const int k = k0 + (q - NFIX) % NEG_PASS;
        if (k >= N) continue;
        id = 3 + ((q - NFIX) / NEG_PASS) * N + k;        // neg0_k, neg2_k
      }
      float* ps = a.pair_stat + ((long long)i * (3 + 2 * N) + id) * 4;
      if (a.l2dist) {
        const float dist = sqrtf(pv[q * 3]);
        ps[0] = dist; ps[1] = 0.f; ps[2] = 0.f; ps[3] = 0.f;
        sim_s[id] = -dist;
      } else {
        const float na = sqrtf(pv[q * 3 + 1]), nb = sqrtf(pv[q * 3 + 2]);
        ps[0] = pv[q * 3]; ps[1] = na; ps[2] = nb; ps[3] = 0.f;
        sim_s[id] = pv[q * 3] / (fmaxf(na, LOSS_EPS) * fmaxf(nb, LOSS_EPS));
      }
    }
  }
}

// ---- pass A: one block per clip: all row norms, the 3 + 2N pair similarities, per-clip loss terms and dL/dsim ----
__global__ __launch_bounds__(256) void tcn_pairs_kernel(const TcnArgs a) {
  __shared__ float smem[4 * (9 * 3)];
  __shared__ float sim_s[MAX_PAIR];        // thread 0's table: the similarities, then their exponentials
  const int i = blockIdx.x;
  const int D = a.D, N = a.N;
  const float* base = a.alle + (long long)i * 5 * D;
  const float* r[5] = {base, base + D, base + 2 * D, base + 3 * D, base + 4 * D};
  // --- row norms ---
  float nv[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) nv[k] = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const float e = r[f][d];
      nv[f * 3 + 0] = fmaf(e, e, nv[f * 3 + 0]);
      nv[f * 3 + 1] += fabsf(e);
      nv[f * 3 + 2] += (e != 0.f) ? 1.f : 0.f;
    }
  }
  block_sum<15>(nv, smem);
  // --- pair sums: the fixed pairs ride with negatives 0..2, then NEG_PASS negatives of each kind per pass ---
  if (a.tcnweight > 0.f) {
    tcn_pair_pass<3>(a, i, 0, r[2], r[3], r[4], smem, sim_s);
    for (int k0 = NEG_PASS; k0 < N; k0 += NEG_PASS) tcn_pair_pass<0>(a, i, k0, r[2], r[3], r[4], smem, sim_s);
  }
  if (threadIdx.x == 0) {
    float s2 = 0.f, s1 = 0.f, s0 = 0.f;
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const float n2 = sqrtf(nv[f * 3]);
      a.rownorm[i * 5 + f] = n2;
      s2 += n2; s1 += nv[f * 3 + 1]; s0 += nv[f * 3 + 2];
    }
    float* cm = a.clipm + (long long)i * NCLIPM;
    cm[0] = s2; cm[1] = s1; cm[2] = s0; cm[3] = 0.f; cm[4] = 0.f; cm[5] = 0.f; cm[6] = 0.f; cm[7] = 0.f;
    if (a.tcnweight > 0.f) {
      const float sim0 = sim_s[0], sim1 = sim_s[1], sim2 = sim_s[2];
      const float e02 = expf(sim0), e12 = expf(sim1), e01 = expf(sim2);
      // exponentials of the negatives, summed left to right: (en[0] + en[1]) + en[2] ...
      float En0 = 0.f, En2 = 0.f;
      for (int k = 0; k < N; ++k) {
        const float e0k = expf(sim_s[3 + k]), e2k = expf(sim_s[3 + N + k]);
        sim_s[3 + k] = e0k; sim_s[3 + N + k] = e2k;
        En0 = k ? En0 + e0k : e0k;
        En2 = k ? En2 + e2k : e2k;
      }
      const float den1 = ((LOSS_EPS + e02) + e12) + En2;
      const float den2 = ((LOSS_EPS + e01) + e02) + En0;
      const float p1 = e12 / den1, p2 = e01 / den2;
      const float L1 = -logf(LOSS_EPS + p1), L2 = -logf(LOSS_EPS + p2);
      cm[3] = (L1 + L2) / 2.0f;
      cm[4] = ((sim0 < sim1) && (sim2 > sim0)) ? 1.f : 0.f;
      const float w = a.tcnweight / (2.0f * (float)a.B);
      const float g1 = -w / (LOSS_EPS + p1), g2 = -w / (LOSS_EPS + p2);
      float* cf = a.coef + (long long)i * (3 + 2 * N);
      cf[0] = g1 * (-p1 * e02 / den1) + g2 * (-p2 * e02 / den2);
      cf[1] = g1 * (p1 - p1 * e12 / den1);
      cf[2] = g2 * (p2 - p2 * e01 / den2);
      for (int k = 0; k < N; ++k) {
        cf[3 + k] = g2 * (-p2 * sim_s[3 + k] / den2);
        cf[3 + N + k] = g1 * (-p1 * sim_s[3 + N + k] / den1);
      }
    }
  }
}

// d sim(a,b) / d(row) for the row playing `role` (0: a, 1: b); returns the two scalars (alpha, beta) such that
//   grad_row += c * (alpha * row + beta * partner)
__device__ __forceinline__ void sim_grad_coeffs(const float* ps, int l2dist, int role, float* alpha, float* beta) {
  if (l2dist) {
    const float dist = ps[0];
    const float k = dist > 0.f ? -1.0f / dist : 0.f;  // s = -dist ; ds/da = -(a-b)/dist ; ds/db = +(a-b)/dist
    *alpha = k;
    *beta = -k;
  } else {
    const float dot = ps[0];
    const float nr = role == 0 ? ps[1] : ps[2];   // this row's norm
    const float np = role == 0 ? ps[2] : ps[1];   // partner's norm
    const float nrc = fmaxf(nr, LOSS_EPS), npc = fmaxf(np, LOSS_EPS);
    *beta = 1.0f / (nrc * npc);
    *alpha = nr > LOSS_EPS ? -dot / (nrc * npc * nr * nr) : 0.f;
  }
}

// ---- pass B: one block per (clip, frame role): LP gradient + every similarity term that touches this row ----
// The term list of a row (owner clip of the pair, pair id, role of this row, partner row), in the order the terms are added:
//   es0: s02, s01, then for k = 0..N-1: neg0_k of this clip, neg0_k of the clip that drew this one (the inverse permutation)
//   es1: s12, s01            es2: s02, s12, then for k = 0..N-1: neg2_k of this clip, neg2_k of the clip that drew this one
// Thread t works out term t into shared tables; every thread then walks them in order, so an element's sum has one fixed order.
__global__ __launch_bounds__(256) void tcn_grad_kernel(const TcnArgs a) {
#pragma clang fp contract(off)     // g += ca * e + cb * p stays two products and two sums, whatever the loop around it looks like
  __shared__ const float* partner_s[MAX_TERM];
  __shared__ float calpha_s[MAX_TERM], cbeta_s[MAX_TERM];
  const int i = blockIdx.x, f = blockIdx.y;
  const int D = a.D, B = a.B, N = a.N;
  const float* row = a.alle + ((long long)i * 5 + f) * D;
  float* out = a.dalle + ((long long)i * 5 + f) * D;
  const float invF = 1.0f / (float)(5 * B);
  const float nrm = a.rownorm[i * 5 + f];
  const float k2 = nrm > 0.f ? a.l2weight * invF / nrm : 0.f;
  const float k1 = a.l1weight * invF;

  const int nt = a.tcnweight > 0.f ? (f == 3 ? 2 : (f == 2 || f == 4 ? 2 + 2 * N : 0)) : 0;
  const int t = threadIdx.x;
  if (t < nt) {
    int owner = i, q, role, pclip = i, pframe;
    if (t < 2) {
      if (f == 2) { q = t == 0 ? 0 : 2; role = 1; pframe = t == 0 ? 4 : 3; }
      else if (f == 3) { q = t == 0 ? 1 : 2; role = t == 0 ? 1 : 0; pframe = t == 0 ? 4 : 2; }
      else { q = t; role = 0; pframe = t == 0 ? 2 : 3; }
    } else {
      const int k = (t - 2) >> 1, prow = 2 * k + (f == 4 ? 1 : 0);
      q = (f == 4 ? 3 + N : 3) + k;
      pframe = f;
      if (((t - 2) & 1) == 0) { role = 0; pclip = a.perm[prow * B + i]; }
      else { role = 1; owner = pclip = a.iperm[prow * B + i]; }
    }
    float al, be;
    sim_grad_coeffs(a.pair_stat + ((long long)owner * (3 + 2 * N) + q) * 4, a.l2dist, role, &al, &be);
    const float c = a.coef[(long long)owner * (3 + 2 * N) + q];
    partner_s[t] = a.alle + ((long long)pclip * 5 + pframe) * D;
    calpha_s[t] = c * al;
    cbeta_s[t] = c * be;
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 256) {
    const float e = row[d];
    float g = k2 * e + k1 * ((e > 0.f) ? 1.f : ((e < 0.f) ? -1.f : 0.f));
    for (int u = 0; u < nt; ++u) g += calpha_s[u] * e + cbeta_s[u] * partner_s[u][d];
    out[d] = g;
  }
}

// ---- language InfoNCE on the 6 + 3N score vectors (trainer.py:72-117) ----
// scores [6+3N][B]: q0..2 = pos1..3 ; q3..5 = in-clip negatives (e0e0, e0es0, e0es1) ; q6+3k+j = k-th permuted negative of
// head j (call order of the reference loop). Writes dscore [6+3N][B] and per-clip partials {rew_i, acc1, acc2, acc3}.
// Head j's negatives are the in-clip one, then k = 0..N-1: summed in that order, and the positive is compared with the max of all.
__global__ __launch_bounds__(256) void lang_infonce_kernel(const float* __restrict__ scores, const float* __restrict__ mask,
                                                            float* __restrict__ dscore, float* __restrict__ clipl, int B, int N,
                                                            float langweight) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const float mk = mask[i];
  const float w = langweight * mk / (3.0f * (float)B);
  float rew = 0.f;
  for (int j = 0; j < 3; ++j) {
    const float pos = scores[(long long)j * B + i];
    float mx = -INFINITY, sum = 0.f;
    for (int k = 0; k <= N; ++k) {                       // k = 0: the in-clip negative, row 3 + j; then rows 6 + 3 (k - 1) + j
      const float sn = scores[(long long)(3 * k + 3 + j) * B + i];
      const float en = expf(sn);
      sum = k ? sum + en : en;
      mx = fmaxf(mx, sn);
    }
    const float ep = expf(pos);
    const float den = (LOSS_EPS + ep) + sum;
    const float p = ep / den;
    rew += -logf(LOSS_EPS + p);
    const float g = -w / (LOSS_EPS + p);
    dscore[(long long)j * B + i] = g * (p - p * ep / den);
    for (int k = 0; k <= N; ++k) {
      const long long at = (long long)(3 * k + 3 + j) * B + i;
      dscore[at] = g * (-p * expf(scores[at]) / den);
    }
    clipl[(long long)i * 4 + 1 + j] = (mx < pos) ? 1.f : 0.f;
  }
  clipl[(long long)i * 4 + 0] = mk * (rew / 3.0f);
}

// ---- finalize: fixed-order sums over clips -> metrics[16] ----
// metrics: 0 l2loss, 1 l1loss, 2 l0loss, 3 tcnloss, 4 aligned, 5 rewloss, 6 rewacc1, 7 rewacc2, 8 rewacc3, 9 full_loss
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ clipm, const float* __restrict__ clipl,
                                                             float* __restrict__ metrics, int B, float l2w, float l1w,
                                                             float tcnw, float langw) {
  __shared__ float smem[4 * 9];
  float v[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) {
    const float* cm = clipm + (long long)i * NCLIPM;
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] += cm[k];
    if (clipl) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[5 + k] += clipl[(long long)i * 4 + k];
    }
  }
  block_sum<9>(v, smem);
  if (threadIdx.x == 0) {
    const float invF = 1.0f / (float)(5 * B), invB = 1.0f / (float)B;
    const float l2 = v[0] * invF, l1 = v[1] * invF, l0 = v[2] * invF;
    const float tcn = v[3] * invB, al = v[4] * invB;
    const float rew = v[5] * invB;
    metrics[0] = l2; metrics[1] = l1; metrics[2] = l0; metrics[3] = tcn; metrics[4] = al;
    metrics[5] = rew; metrics[6] = v[6] * invB; metrics[7] = v[7] * invB; metrics[8] = v[8] * invB;
    float full = l2w * l2;
    full += l1w * l1;
    if (langw > 0.f) full += langw * rew;
    if (tcnw > 0.f) full += tcnw * tcn;
    metrics[9] = full;
  }
}

// Workspace (floats): clipm [B][8], clipl [B][4], rownorm [B][5] -- what r3m_loss_finalize reads comes first, at offsets that do not
// depend on N -- then pair_stat [B][3+2N][4] and coef [B][3+2N], and 64 floats to spare.
size_t loss_workspace_floats(int B, int N) { return (size_t)B * (NCLIPM + 4 + 5 + (size_t)(3 + 2 * N) * 5) + 64; }
size_t loss_finalize_floats(int B) { return (size_t)B * (NCLIPM + 4); }
static float* loss_ws_clipm(float* ws) { return ws; }
static float* loss_ws_clipl(float* ws, int B) { return ws + (size_t)B * NCLIPM; }

// the one place that refuses a shape or a number of negatives (the C ABI calls it before it sizes or launches anything)
int loss_refused(const char* what, int B, int D, int N, float tcnw) {
  R3M_REQUIRE(B >= 1 && D >= 1, "%s: B=%d D=%d", what, B, D);
  R3M_REQUIRE(N >= 0 && N <= LOSS_MAX_NEG, "%s: num_negatives=%d is outside 0..16 (R3M_MAX_NEGATIVES)", what, N);
  R3M_REQUIRE(N > 0 || !(tcnw > 0.f), "%s: num_negatives=%d with tcnweight > 0: the reference fails there (torch.stack of an empty list, "
              "r3m/trainer.py:140)", what, N);
  return 0;
}

int launch_tcn_lp_loss(const float* alle, const int* perm, const int* iperm, float* dalle, float* ws, int B, int D, int N, int l2dist,
                       float l2w, float l1w, float tcnw, hipStream_t s) {
  TcnArgs a;
  a.alle = alle; a.perm = perm; a.iperm = iperm; a.dalle = dalle;
  a.clipm = loss_ws_clipm(ws);
  a.rownorm = loss_ws_clipl(ws, B) + (size_t)B * 4;
  a.pair_stat = a.rownorm + (size_t)B * 5;
  a.coef = a.pair_stat + (size_t)B * (3 + 2 * N) * 4;
  a.B = B; a.D = D; a.N = N; a.l2dist = l2dist; a.l2weight = l2w; a.l1weight = l1w; a.tcnweight = tcnw;
  hipLaunchKernelGGL(tcn_pairs_kernel, dim3(B), dim3(256), 0, s, a);
  if (int e = check_launch("tcn_pairs")) return e;
  if (dalle) {
    hipLaunchKernelGGL(tcn_grad_kernel, dim3(B, 5), dim3(256), 0, s, a);
    if (int e = check_launch("tcn_grad")) return e;
  }
  return 0;
}

int launch_lang_infonce(const float* scores, const float* mask, float* dscore, float* ws, int B, int N, float langw, hipStream_t s) {
  hipLaunchKernelGGL(lang_infonce_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, s, scores, mask, dscore, loss_ws_clipl(ws, B), B, N, langw);
  return check_launch("lang_infonce");
}

int launch_loss_finalize(float* ws, int B, int have_lang, float* metrics, float l2w, float l1w, float tcnw, float langw,
                         hipStream_t s) {
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, loss_ws_clipm(ws),
                     have_lang ? loss_ws_clipl(ws, B) : (const float*)nullptr, metrics, B, l2w, l1w, tcnw, langw);
  return check_launch("loss_finalize");
}

}  // namespace r3m
