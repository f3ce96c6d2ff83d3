"""-m gpu: the objective (csrc/loss.hip) through the C ABI, one entry point at a time, against oracle/r3m_ref.r3m_loss_ref evaluated in
float64 on the CPU on the same fp32 values, at the edges of the launch geometry that the golden tests (B = 8, D = 512) and the
comfortable sizes of tests/test_gpu_encoder.py / tests/test_gpu_lang.py do not reach:

  * tcn_pairs_kernel / tcn_grad_kernel: the strided `d += 256` loops with a tail (D = 1, 255, 257; D = 33 and 8 leave three of the four
    waves of block_sum carrying only zeros) and with many trips (D = 2048);
  * loss_finalize_kernel: the second and third trip of its `i += 256` loop (B = 257, 513);
  * lang_infonce_kernel: a second and third block (B = 257, 513), and `dscore` element by element.

Every output buffer enters filled with NaN, the workspace is the size r3m_loss_workspace_bytes reports, filled with NaN, plus a
256-byte guard that must come back intact. Ceilings: the project's own for these quantities (tests/test_gpu_encoder.py
test_tcn_lp_loss_matches_reference_golden): metrics 1e-5 * max(1, |ref|), gradients max-rel < 1e-4. Counts (aligned, rewacc1..3) must
match exactly; the input builders keep every compared pair of similarities / scores more than 1e-4 apart in float64.

Witness rule (as tests/test_gpu_bn.py): a figure over its ceiling may pass only if it is listed in WITNESSED below with its measured
value and is within 4 x the error of the same oracle evaluated in float32 on the CPU. Measured figures: profiles/objective_edges.txt.
One case needed the rule:
  * (B, D) = (2, 1), cosine, tcnweight 1, dalle of the non-zero rows: MI355X 2.235e-02, float32 oracle on the CPU 2.980e-02, ceiling
    1e-4. The cosine of two one-element rows is +-1 whatever their values, so its gradient is exactly 0 in float64 and the scale of
    the reference is the LP gradient alone (2e-6); in fp32 the two halves of the cosine gradient (each ~0.1 / x) cancel to their
    rounding residue, on the kernel as in torch. The metrics and the zero rows of the same case are inside their ceilings."""
import functools

import numpy as np
import pytest
import torch

from util import DEV, _st, assert_edge_figures, assert_guard_intact, guarded_bytes, rel_err, rnd

pytestmark = pytest.mark.gpu

# (B, D): what the case reaches
CASES = [(1, 32),      # one clip, every permutation a fixed point
         (2, 1),       # one element per row
         (3, 255),     # tail just under the 256-thread stride
         (3, 257),     # tail just over it: a second trip with one live lane
         (2, 2048),    # many trips of the stride loop
         (257, 8),     # second trip of the finalize loop
         (513, 33)]    # third trip, second (and third) InfoNCE block, odd D
L2W, L1W = 1e-5, 1e-5              # as the goldens have
SLOTS = dict(l2loss=0, l1loss=1, l0loss=2, tcnloss=3, aligned=4, rewloss=5, rewacc1=6, rewacc2=7, rewacc3=8, full_loss=9)
COUNTS = ("aligned", "rewacc1", "rewacc2", "rewacc3")
WITNESSED = (("tcn_lp B=2 D=1 cosine tcnweight=1", "dalle rows"),)         # (what, figure) pairs that needed the witness rule


class _Objective:
    """what r3m_loss_ref asks of its model: the weights, R3M.sim, and a reward head -- here one that hands out the rows of a given
    score table in the reference's call order (pos1-3, in-clip negatives, then k-major permuted negatives: the table's own order)"""
    num_negatives = 3

    def __init__(self, l2dist, tcnweight, langweight=0.0, score_rows=None):
        from oracle import r3m_ref
        self.l2weight, self.l1weight, self.tcnweight, self.langweight, self.l2dist = L2W, L1W, tcnweight, langweight, l2dist
        self.cs = torch.nn.CosineSimilarity(1)
        self._sim = r3m_ref.R3MRef.sim
        self._rows = iter(score_rows) if score_rows is not None else None

    def sim(self, a, b):
        return self._sim(self, a, b)

    def lang_rew(self, a, b, feats):
        return next(self._rows)


def oracle(alle, perm, l2dist, tcnweight, dtype, scores=None, mask=None, langweight=0.0):
    """r3m_loss_ref in `dtype` on the CPU -> (metrics dict, d full_loss / d alle, d full_loss / d scores or None)"""
    from oracle import r3m_ref
    a = alle.to(dtype).clone().requires_grad_(True)
    rows = None if scores is None else [scores[q].to(dtype).clone().requires_grad_(True) for q in range(15)]
    model = _Objective(l2dist, tcnweight, langweight if scores is not None else 0.0, rows)
    full, met, _ = r3m_ref.r3m_loss_ref(model, a, tcn_perm=perm, lang_mask=None if mask is None else mask.to(dtype),
                                        lang_perm=torch.arange(a.shape[0]).repeat(9, 1))      # the head above ignores its inputs
    full.backward()
    ds = None if rows is None else torch.stack([r.grad for r in rows]).double().numpy()
    return met, a.grad.double().numpy(), ds


@functools.lru_cache(maxsize=None)
def embeddings(B, D, l2dist):
    """alle [B,5,D] = relu(uniform(-0.5, 1.0)): non-negative with many exact zeros, like the encoder's output, so the L0 count and the L1
    sign at zero are exercised. B >= 2: clip 1's es1 row is all zero (cosine: its gradient is the 1/eps clamp term) and permutation
    row 2 is the identity (every negative is the row itself: distance 0 with sub-gradient 0, or cosine 1). B >= 3: clip 2 has
    es2 == es0. Redrawn with the next seed until s02 / s12 and s01 / s02 of every clip differ by more than 1e-4 in float64."""
    for seed in range(1000):
        alle = torch.relu(rnd((B, 5, D), 100 + seed, -0.5, 1.0))
        if B >= 2:
            alle[1, 3] = 0.0
        if B >= 3:
            alle[2, 4] = alle[2, 2]
        g = torch.Generator().manual_seed(200 + seed)
        perm = torch.stack([torch.randperm(B, generator=g) for _ in range(6)])
        perm[2] = torch.arange(B)
        a = alle.double()
        sim = _Objective(l2dist, 1.0).sim
        s02, s12, s01 = sim(a[:, 4], a[:, 2]), sim(a[:, 4], a[:, 3]), sim(a[:, 3], a[:, 2])
        if float((s02 - s12).abs().min()) > 1e-4 and float((s01 - s02).abs().min()) > 1e-4:
            return alle, perm
    raise AssertionError(f"no draw of B={B} D={D} keeps the compared similarities apart")


@functools.lru_cache(maxsize=None)
def reference(B, D, l2dist, tcnweight):
    """(float64 result, float32 witness) of the TCN + LP objective, computed once per case"""
    alle, perm = embeddings(B, D, l2dist)
    return oracle(alle, perm, l2dist, tcnweight, torch.float64), oracle(alle, perm, l2dist, tcnweight, torch.float32)


class Device:
    """one case's buffers: NaN-filled outputs, NaN-filled workspace of the reported size + guard"""

    def __init__(self, hip, alle, perm):
        from r3m_amd.ops import inverse_permutations
        self.hip, self.B, self.D = hip, alle.shape[0], alle.shape[2]
        self.alle = alle.to(DEV)
        self.perm = perm.to(torch.int32).to(DEV).contiguous()
        self.iperm = inverse_permutations(self.perm).contiguous()
        self.wsb = hip.r3m_loss_workspace_bytes(self.B)
        self.ws = guarded_bytes(self.wsb)
        self.ws[:self.wsb] = 0xFF                                    # every float of the workspace a NaN

    def tcn_lp(self, l2dist, tcnweight, want_dalle=True):
        dalle = torch.full((self.B, 5, self.D), float("nan"), device=DEV) if want_dalle else None
        rc = self.hip.r3m_loss_tcn_lp(self.alle.data_ptr(), self.perm.data_ptr(), self.iperm.data_ptr(), None if dalle is None else dalle.data_ptr(),
                                      self.ws.data_ptr(), self.wsb, self.B, self.D, 1 if l2dist else 0, L2W, L1W, tcnweight, _st())
        assert rc == 0, self.hip.r3m_last_error()
        return dalle

    def infonce(self, scores, mask, langweight):
        sd, md = scores.to(DEV).contiguous(), mask.to(DEV).contiguous()
        ds = torch.full((15, self.B), float("nan"), device=DEV)
        rc = self.hip.r3m_loss_lang_infonce(sd.data_ptr(), md.data_ptr(), ds.data_ptr(), self.ws.data_ptr(), self.wsb, self.B, langweight, _st())
        assert rc == 0, self.hip.r3m_last_error()
        return ds

    def finalize(self, have_lang, tcnweight, langweight):
        met = torch.full((16,), float("nan"), device=DEV)
        rc = self.hip.r3m_loss_finalize(self.ws.data_ptr(), self.wsb, self.B, have_lang, met.data_ptr(), L2W, L1W, tcnweight, langweight, _st())
        assert rc == 0, self.hip.r3m_last_error()
        torch.cuda.synchronize()
        assert_guard_intact(self.ws, self.wsb, f"loss workspace B={self.B}")
        return met.cpu().double().numpy()


def metric_figures(got, ref, names, B, counts=True):
    """{name: |got - ref| / max(1, |ref|)}; counts: the ranking metrics must also be the same whole number of clips"""
    out = {}
    for k in names:
        r = ref.get(k, 0.0)
        out[k] = abs(float(got[SLOTS[k]]) - r) / max(1.0, abs(r))
        if counts and k in COUNTS:
            assert round(float(got[SLOTS[k]]) * B) == round(r * B), (k, float(got[SLOTS[k]]) * B, r * B)
    return out


def dalle_figures(got, ref, alle, per_clip):
    """max-rel of dalle in separate parts: the rows that are not all zero; the all-zero rows on their own scale (under cosine their
    gradient is the 1/eps clamp term, ~1e7: it must not set the scale for the others); each clip on its own scale (B >= 257)"""
    zero = (alle.numpy() == 0).all(-1)                               # [B,5]
    out = {"dalle rows": rel_err(got[~zero], ref[~zero])[0]}
    if zero.any():
        out["dalle zero rows"] = rel_err(got[zero], ref[zero])[0]
    if per_clip:
        keep = (~zero)[:, :, None]
        d = np.abs((got - ref) * keep).max((1, 2))
        s = np.abs(ref * keep).max((1, 2))
        assert (s > 0).all()
        out["dalle worst clip on its own scale"] = float((d / s).max())
    return out


def ceilings(figs):
    return {k: (1e-4 if k.startswith("d") else 1e-5) for k in figs}


@pytest.mark.parametrize("l2dist", [1, 0], ids=["l2dist", "cosine"])
@pytest.mark.parametrize("B,D", CASES, ids=[f"B{b}_D{d}" for b, d in CASES])
def test_tcn_lp_and_finalize_against_float64(hip, B, D, l2dist):
    """r3m_loss_tcn_lp + r3m_loss_finalize (have_lang 0): metrics 0-4 and 9 and dalle in three parts, at tcnweight 1; then with
    tcnweight 0 (dalle must be the LP gradient alone, metrics 3 and 4 exactly 0) and with dalle = NULL (metrics bit-identical).
    Paths first reached here: tcn_pairs_kernel / tcn_grad_kernel with a tail of the `d += 256` loop and block_sum waves that carry only
    zeros -- (2, 1), (3, 255), (3, 257), (513, 33); loss_finalize_kernel's second / third trip of `i += 256` -- (257, 8), (513, 33)."""
    alle, perm = embeddings(B, D, l2dist)
    assert bool((alle == 0).any()) and (B < 2 or (bool((alle[1, 3] == 0).all()) and bool((perm[2] == torch.arange(B)).all())))
    assert B < 3 or torch.equal(alle[2, 4], alle[2, 2])
    dev = Device(hip, alle, perm)
    names = ("l2loss", "l1loss", "l0loss", "tcnloss", "aligned", "full_loss")
    kept = None
    for tcnw in (1.0, 0.0):
        (m64, d64, _), (m32, d32, _) = reference(B, D, l2dist, tcnw)
        dalle = dev.tcn_lp(l2dist, tcnw)
        met = dev.finalize(0, tcnw, 0.0)
        assert (met[5:9] == 0).all(), met[5:9]                       # have_lang = 0
        got = dalle.cpu().double().numpy()
        wit_met = np.zeros(16)
        for k in names:
            wit_met[SLOTS[k]] = m32.get(k, 0.0)
        figs = {**metric_figures(met, m64, names, B), **dalle_figures(got, d64, alle, B >= 257)}
        wit = {**metric_figures(wit_met, m64, names, B, counts=False), **dalle_figures(d32, d64, alle, B >= 257)}
        what = f"tcn_lp B={B} D={D} {'l2dist' if l2dist else 'cosine'} tcnweight={tcnw:g}"
        assert_edge_figures(what, figs, wit, ceilings(figs), WITNESSED)
        if tcnw == 0.0:
            assert met[3] == 0 and met[4] == 0
        else:
            kept = met
    # dalle = NULL: metrics only, the same ones
    assert dev.tcn_lp(l2dist, 1.0, want_dalle=False) is None
    met = dev.finalize(0, 1.0, 0.0)
    assert np.array_equal(met[:10], kept[:10]), (met[:10], kept[:10])


@functools.lru_cache(maxsize=None)
def score_table(B, rng, tie=False):
    """scores [15,B] uniform in [-rng, rng], mask [B] of 0 / 1 with zeros (B >= 2), every positive more than 1e-4 away from its largest
    negative in float64 (redrawn with the next seed otherwise). tie: head 0 of clip B // 2 gets a positive bit-equal to its largest
    negative -- `<` is strict, so that clip counts 0."""
    for seed in range(1000):
        s = rnd((15, B), 300 + seed, -float(rng), float(rng))
        mask = (rnd((B,), 400 + seed) > -0.4).float()
        mask[0] = 1.0
        if B >= 2:
            mask[B - 1] = 0.0
        d = s.double()
        ok = True
        for j in range(3):
            mx = torch.stack([d[3 + j]] + [d[6 + 3 * k + j] for k in range(3)]).max(0)[0]
            ok = ok and float((d[j] - mx).abs().min()) > 1e-4
        if ok:
            if tie:
                i = B // 2
                s[0, i] = torch.stack([s[3, i], s[6, i], s[9, i], s[12, i]]).max()
                mask[i] = 1.0
            return s, mask
    raise AssertionError(f"no draw of B={B} keeps the positives apart from their negatives")


def _infonce_case(hip, B, D, scores, mask, what):
    alle, perm = embeddings(B, D, 1)
    dev = Device(hip, alle, perm)
    dev.tcn_lp(1, 1.0)
    ds = dev.infonce(scores, mask, 1.0)
    met = dev.finalize(1, 1.0, 1.0)
    m64, _, ds64 = oracle(alle, perm, 1, 1.0, torch.float64, scores, mask, 1.0)
    m32, _, ds32 = oracle(alle, perm, 1, 1.0, torch.float32, scores, mask, 1.0)
    names = ("rewloss", "rewacc1", "rewacc2", "rewacc3", "full_loss")
    wit_met = np.zeros(16)
    for k in names:
        wit_met[SLOTS[k]] = m32[k]
    got = ds.cpu().double().numpy()
    assert got.shape == (15, B) and np.isfinite(got).all()
    figs = {**metric_figures(met, m64, names, B), "dscore": rel_err(got, ds64)[0]}
    wit = {**metric_figures(wit_met, m64, names, B, counts=False), "dscore": rel_err(ds32, ds64)[0]}
    assert_edge_figures(what, figs, wit, ceilings(figs), WITNESSED)
    # have_lang = 0 on the same workspace: the language slots read 0, full_loss drops the term
    met0 = dev.finalize(0, 1.0, 0.0)
    assert (met0[5:9] == 0).all(), met0[5:9]
    return met, got, m64


INFONCE_B = [(1, 32), (2, 1), (257, 8), (513, 33)]


@pytest.mark.parametrize("rng", [3, 15])
@pytest.mark.parametrize("B,D", INFONCE_B, ids=[f"B{b}" for b, _ in INFONCE_B])
def test_lang_infonce_against_float64(hip, B, D, rng):
    """r3m_loss_lang_infonce + r3m_loss_finalize (have_lang 1): all 15 B entries of dscore, metrics 5-8 and full_loss; scores uniform in
    [-3, 3] and [-15, 15] (the literal form of the reference overflows only above 88: not under test), mask with zeros. Paths first
    reached here: lang_infonce_kernel's second and third block and loss_finalize_kernel's further trips with the language partials
    -- B = 257, 513; dscore compared element by element at every B."""
    scores, mask = score_table(B, rng)
    assert B < 2 or (float(mask.min()) == 0 and float(mask.max()) == 1)
    _infonce_case(hip, B, D, scores, mask, f"infonce B={B} scores in [-{rng}, {rng}]")


def test_lang_infonce_all_zero_mask_is_exactly_zero(hip):
    """an all-zero mask (no clip of the batch has language): rewloss and every dscore exactly 0, at B = 257 (two blocks)"""
    B, D = 257, 8
    scores, _ = score_table(B, 3)
    met, ds, _ = _infonce_case(hip, B, D, scores, torch.zeros(B), "infonce B=257 all-zero mask")
    assert met[SLOTS["rewloss"]] == 0 and (ds == 0).all()


def test_lang_infonce_tie_counts_zero(hip):
    """a positive score bit-equal to its largest negative: `max(neg) < pos` is strict, so that clip counts 0 for rewacc1 (B = 257: the
    clip sits in the first block, the counts are summed over both)"""
    B, D = 257, 8
    scores, mask = score_table(B, 3, tie=True)
    i = B // 2
    assert float(scores[0, i]) == float(torch.stack([scores[3, i], scores[6, i], scores[9, i], scores[12, i]]).max())
    met, _, m64 = _infonce_case(hip, B, D, scores, mask, "infonce B=257 tie")
    # with the positive a hair above, the same clip counts 1: the tie is what decides
    up = scores.clone()
    up[0, i] = torch.nextafter(scores[0, i], torch.tensor(float("inf")))
    met_up, _, m64_up = _infonce_case(hip, B, D, up, mask, "infonce B=257 tie + 1 ulp")
    assert round(m64_up["rewacc1"] * B) == round(m64["rewacc1"] * B) + 1
    assert round(met_up[SLOTS["rewacc1"]] * B) == round(met[SLOTS["rewacc1"]] * B) + 1
