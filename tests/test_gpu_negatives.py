"""-m gpu: num_negatives = N through every layer -- the `_n` entry points of the objective (csrc/loss.hip) and of the batched reward head
(csrc/lang.hip), ops.r3m_loss, LanguageReward.batched_scores, R3M(num_negatives=) and Trainer.update.

The objective is checked the way tests/test_gpu_objective.py checks N = 3 (its helpers are imported, the file is not edited): NaN-filled
outputs, a NaN-filled workspace of exactly r3m_loss_workspace_bytes_n(B, N) bytes with a 256-byte guard behind it, float64
oracle/r3m_ref.r3m_loss_ref on the same fp32 values, that file's ceilings (metrics 1e-5 * max(1, |ref|), gradients max-rel 1e-4, counts
exact) and its witness rule, with nothing witnessed here. On top of its three dalle figures every non-zero row of dalle is compared on
its own scale (ceiling 1e-4, the file's per-clip ceiling applied to a row): a term missing from the list of an es0 / es2 row moves
that row by a share of its own size, which the whole-tensor figure could hide.

Shapes: (1, 32) every permutation a fixed point (negative = own row: distance 0 with sub-gradient 0, cosine 1); (2, 3) and (3, 257) the
stride loops' tails; (5, 2048) many trips; (257, 8), at N = 16 only, the finalize and InfoNCE loops' second trip. N: 1, 2 (one partly
filled pass of tcn_pairs_kernel), 3 (one full pass), 4 and 7 (a second and third pass, partly filled), 16 (the cap: six passes, 34
terms per row), and 0 for the language kernel. The permutation sets hold the identity (row 0), a self-inverse permutation (row 1, the
reversal) and, from N = 2 on, the same permutation for two different k.

Every test reaches the `_n` symbols or R3M(num_negatives=) before any launch, so on a tree without the feature it fails in Python
(AttributeError / TypeError) and launches nothing."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_objective as obj
from util import DEV, _st, assert_edge_figures, assert_guard_intact, guarded_bytes, rel_err, rnd

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 4, 7, 16)
SHAPES = ((1, 32), (2, 3), (3, 257), (5, 2048))
TCN_CASES = [(N, B, D) for N in NS for (B, D) in SHAPES] + [(16, 257, 8)]
LANG_CASES = [(N, B, D) for N in (0,) + NS for (B, D) in SHAPES] + [(16, 257, 8)]
L2W, L1W, SLOTS = obj.L2W, obj.L1W, obj.SLOTS


def _ids(cases):
    return [f"N{n}_B{b}_D{d}" for n, b, d in cases]


class _Objective(obj._Objective):
    def __init__(self, N, *a, **k):
        super().__init__(*a, **k)
        self.num_negatives = N


def oracle(N, alle, perm, l2dist, tcnweight, dtype, scores=None, mask=None, langweight=0.0):
    """r3m_loss_ref with num_negatives = N in `dtype` on the CPU -> (metrics, d full_loss / d alle, d full_loss / d scores or None)"""
    from oracle import r3m_ref
    a = alle.to(dtype).clone().requires_grad_(True)
    rows = None if scores is None else [scores[q].to(dtype).clone().requires_grad_(True) for q in range(6 + 3 * N)]
    model = _Objective(N, l2dist, tcnweight, langweight if scores is not None else 0.0, rows)
    full, met, _ = r3m_ref.r3m_loss_ref(model, a, tcn_perm=perm, lang_mask=None if mask is None else mask.to(dtype),
                                        lang_perm=torch.arange(a.shape[0]).repeat(max(3 * N, 1), 1))   # the head ignores its inputs
    full.backward()
    ds = None if rows is None else torch.stack([r.grad for r in rows]).double().numpy()
    return met, a.grad.double().numpy(), ds


@functools.lru_cache(maxsize=None)
def permutations(N, B):
    """[2N, B]: row 0 the identity, row 1 the reversal (its own inverse); N = 2: rows 1 and 3 equal (es2, k = 0 and 1); N >= 3: rows 2
    and 4 equal (es0, k = 1 and 2); the rest drawn"""
    g = torch.Generator().manual_seed(500 + 17 * N + B)
    perm = torch.stack([torch.randperm(B, generator=g) for _ in range(2 * N)])
    perm[0] = torch.arange(B)
    perm[1] = torch.arange(B - 1, -1, -1)
    if N == 2:
        perm[3] = perm[1]
    if N >= 3:
        perm[4] = perm[2]
    assert torch.equal(perm[1][perm[1]], torch.arange(B))
    return perm


@functools.lru_cache(maxsize=None)
def reference(N, B, D, l2dist, tcnweight):
    alle, _ = obj.embeddings(B, D, l2dist)          # non-negative with exact zeros, a zero row, es2 == es0, compared similarities apart
    perm = permutations(N, B)
    return oracle(N, alle, perm, l2dist, tcnweight, torch.float64), oracle(N, alle, perm, l2dist, tcnweight, torch.float32)


class Device:
    """one case's buffers: NaN-filled outputs, NaN-filled workspace of the reported size + guard; every call is an `_n` entry point"""

    def __init__(self, hip, N, alle, perm):
        from r3m_amd.ops import inverse_permutations
        self.hip, self.N, self.B, self.D = hip, N, alle.shape[0], alle.shape[2]
        self.wsb = hip.r3m_loss_workspace_bytes_n(self.B, N)       # first: a library without the entry point fails here
        assert self.wsb > 0, hip.r3m_last_error()
        self.alle = alle.to(DEV)
        self.perm = perm.to(torch.int32).to(DEV).contiguous()
        self.iperm = inverse_permutations(self.perm).contiguous()
        self.ws = guarded_bytes(self.wsb)
        self.ws[:self.wsb] = 0xFF

    def tcn_lp(self, l2dist, tcnweight, want_dalle=True):
        dalle = torch.full((self.B, 5, self.D), float("nan"), device=DEV) if want_dalle else None
        rc = self.hip.r3m_loss_tcn_lp_n(self.alle.data_ptr(), self.perm.data_ptr(), self.iperm.data_ptr(),
                                        None if dalle is None else dalle.data_ptr(), self.ws.data_ptr(), self.wsb, self.B, self.D, self.N,
                                        1 if l2dist else 0, L2W, L1W, tcnweight, _st())
        assert rc == 0, self.hip.r3m_last_error()
        return dalle

    def infonce(self, scores, mask, langweight):
        sd, md = scores.to(DEV).contiguous(), mask.to(DEV).contiguous()
        ds = torch.full((6 + 3 * self.N, self.B), float("nan"), device=DEV)
        rc = self.hip.r3m_loss_lang_infonce_n(sd.data_ptr(), md.data_ptr(), ds.data_ptr(), self.ws.data_ptr(), self.wsb, self.B, self.N,
                                              langweight, _st())
        assert rc == 0, self.hip.r3m_last_error()
        return ds

    def finalize(self, have_lang, tcnweight, langweight):
        met = torch.full((16,), float("nan"), device=DEV)
        rc = self.hip.r3m_loss_finalize(self.ws.data_ptr(), self.wsb, self.B, have_lang, met.data_ptr(), L2W, L1W, tcnweight, langweight, _st())
        assert rc == 0, self.hip.r3m_last_error()
        torch.cuda.synchronize()
        assert_guard_intact(self.ws, self.wsb, f"loss workspace B={self.B} N={self.N}")
        return met.cpu().double().numpy()


def row_figure(got, ref, alle):
    """the worst non-zero row of dalle on its own scale"""
    keep = ~(alle.numpy() == 0).all(-1)
    d = np.abs(got - ref).max(-1)[keep]
    s = np.abs(ref).max(-1)[keep]
    assert (s > 0).all()
    return float((d / s).max())


@pytest.mark.parametrize("l2dist", [1, 0], ids=["l2dist", "cosine"])
@pytest.mark.parametrize("N,B,D", TCN_CASES, ids=_ids(TCN_CASES))
def test_tcn_lp_n_against_float64(hip, N, B, D, l2dist):
    """r3m_loss_tcn_lp_n + r3m_loss_finalize: metrics 0-4 and 9 and dalle (whole, zero rows, per clip, per row) at tcnweight 1; the
    LP gradient alone at tcnweight 0; dalle = NULL gives the same metrics bit for bit"""
    alle = obj.embeddings(B, D, l2dist)[0]
    dev = Device(hip, N, alle, permutations(N, B))
    names = ("l2loss", "l1loss", "l0loss", "tcnloss", "aligned", "full_loss")
    kept = None
    for tcnw in (1.0, 0.0):
        (m64, d64, _), (m32, d32, _) = reference(N, B, D, l2dist, tcnw)
        dalle = dev.tcn_lp(l2dist, tcnw)
        met = dev.finalize(0, tcnw, 0.0)
        assert (met[5:9] == 0).all(), met[5:9]
        got = dalle.cpu().double().numpy()
        assert np.isfinite(got).all()
        wit_met = np.zeros(16)
        for k in names:
            wit_met[SLOTS[k]] = m32.get(k, 0.0)
        figs = {**obj.metric_figures(met, m64, names, B), **obj.dalle_figures(got, d64, alle, True), "dalle worst row on its own scale": row_figure(got, d64, alle)}
        wit = {**obj.metric_figures(wit_met, m64, names, B, counts=False), **obj.dalle_figures(d32, d64, alle, True),
               "dalle worst row on its own scale": row_figure(d32, d64, alle)}
        what = f"tcn_lp_n N={N} B={B} D={D} {'l2dist' if l2dist else 'cosine'} tcnweight={tcnw:g}"
        assert_edge_figures(what, figs, wit, obj.ceilings(figs), ())
        if tcnw == 0.0:
            assert met[3] == 0 and met[4] == 0
        else:
            kept = met
    assert dev.tcn_lp(l2dist, 1.0, want_dalle=False) is None
    met = dev.finalize(0, 1.0, 0.0)
    assert np.array_equal(met[:10], kept[:10]), (met[:10], kept[:10])


@functools.lru_cache(maxsize=None)
def score_table(N, B, rng):
    """scores [6+3N, B] uniform in [-rng, rng], mask [B] of 0 / 1 with a zero (B >= 2), every positive more than 1e-4 from the largest of
    its 1 + N negatives in float64 (redrawn with the next seed otherwise)"""
    for seed in range(1000):
        s = rnd((6 + 3 * N, B), 600 + 31 * N + seed, -float(rng), float(rng))
        mask = (rnd((B,), 700 + seed) > -0.4).float()
        mask[0] = 1.0
        if B >= 2:
            mask[B - 1] = 0.0
        d = s.double()
        if all(float((d[j] - torch.stack([d[3 + j]] + [d[6 + 3 * k + j] for k in range(N)]).max(0)[0]).abs().min()) > 1e-4 for j in range(3)):
            return s, mask
    raise AssertionError(f"no draw of N={N} B={B} keeps the positives apart from their negatives")


@pytest.mark.parametrize("N,B,D", LANG_CASES, ids=_ids(LANG_CASES))
def test_lang_infonce_n_against_float64(hip, N, B, D):
    """r3m_loss_lang_infonce_n + r3m_loss_finalize (have_lang 1): all (6 + 3N) B entries of dscore, metrics 5-8 and full_loss, behind an
    LP-only r3m_loss_tcn_lp_n (tcnweight 0, which N = 0 needs); scores in [-3, 3]"""
    alle = obj.embeddings(B, D, 1)[0]
    perm = permutations(N, B) if N else torch.zeros((0, B), dtype=torch.int64)
    scores, mask = score_table(N, B, 3)
    dev = Device(hip, N, alle, perm)
    dev.tcn_lp(1, 0.0)
    ds = dev.infonce(scores, mask, 1.0)
    met = dev.finalize(1, 0.0, 1.0)
    m64, _, ds64 = oracle(N, alle, perm, 1, 0.0, torch.float64, scores, mask, 1.0)
    m32, _, ds32 = oracle(N, alle, perm, 1, 0.0, torch.float32, scores, mask, 1.0)
    names = ("rewloss", "rewacc1", "rewacc2", "rewacc3", "full_loss")
    wit_met = np.zeros(16)
    for k in names:
        wit_met[SLOTS[k]] = m32[k]
    got = ds.cpu().double().numpy()
    assert got.shape == (6 + 3 * N, B) and np.isfinite(got).all()
    figs = {**obj.metric_figures(met, m64, names, B), "dscore": rel_err(got, ds64)[0],
            "dscore worst row": max(rel_err(got[q], ds64[q])[0] for q in range(6 + 3 * N))}
    wit = {**obj.metric_figures(wit_met, m64, names, B, counts=False), "dscore": rel_err(ds32, ds64)[0],
           "dscore worst row": max(rel_err(ds32[q], ds64[q])[0] for q in range(6 + 3 * N))}
    assert_edge_figures(f"infonce_n N={N} B={B}", figs, wit, obj.ceilings(figs), ())
    assert met[3] == 0 and met[4] == 0


@pytest.mark.parametrize("l2dist", [1, 0], ids=["l2dist", "cosine"])
@pytest.mark.parametrize("B,D", [(3, 257), (5, 2048), (257, 8)])
def test_n_entries_at_three_equal_the_old_entries_bit_for_bit(hip, B, D, l2dist):
    """the same inputs through r3m_loss_tcn_lp / _lang_infonce and through the `_n` calls with N = 3: dalle, dscore and the metrics"""
    assert hip.r3m_loss_workspace_bytes_n(B, 3) == hip.r3m_loss_workspace_bytes(B)
    alle, perm = obj.embeddings(B, D, l2dist)
    scores, mask = obj.score_table(B, 3)
    old, new = obj.Device(hip, alle, perm), Device(hip, 3, alle, perm)
    out = []
    for dev in (old, new):
        dalle = dev.tcn_lp(l2dist, 1.0)
        ds = dev.infonce(scores, mask, 1.0)
        met = dev.finalize(1, 1.0, 1.0)
        out.append((dalle, ds, met))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert np.isfinite(out[1][2][:10]).all() and np.array_equal(out[0][2][:10], out[1][2][:10])      # slots 10-15 are not written


# ---- the batched head ---------------------------------------------------------------------------------------------------------------
def _lang_state(module):
    from oracle import detgen
    sd, full = {}, module.state_dict()
    for k, v in full.items():
        fan_in = v.shape[1] if v.dim() == 2 else full[k.replace("bias", "weight")].shape[1]
        a = 1.0 / np.sqrt(fan_in)
        sd[k] = torch.from_numpy(detgen.uniform("lr" + k, tuple(v.shape), -a, a))
    return sd


def _head_inputs(N, B, D, LD):
    g = torch.Generator().manual_seed(800 + 13 * N + B)
    perm = torch.stack([torch.randperm(B, generator=g) for _ in range(3 * N)]) if N else torch.zeros((0, B), dtype=torch.int64)
    if B >= 2:                                       # clip 0 is mapped to itself by no permutation: its rows are reached through iperm only
        for r in range(3 * N):
            if int(perm[r, 0]) == 0:
                perm[r, [0, 1]] = perm[r, [1, 0]]
        assert not bool((perm[:, 0] == 0).any())
    alle0 = torch.relu(rnd((B, 5, D), 810 + N, -0.5, 1.0))
    feats = rnd((B, LD), 820 + N, -0.6, 0.6)
    wts = rnd((6 + 3 * N, B), 830 + N, -1.0, 1.0)
    return perm, alle0, feats, wts


def _rounding_model_loop(rew, alle0, feats, perm, wts, N):
    """the 6 + 3N calls one by one in float64 with the bf16 head's roundings (input rows, weights, the GEMM result, every hidden
    activation; straight-through in the backward pass) -> (scores [6+3N, B], d/d alle, flat parameter gradients) of sum(scores * wts)"""
    def r16(t):
        return t + (t.to(torch.bfloat16).to(torch.float64) - t).detach()
    sd = rew.state_dict()
    wb = [tuple(sd[f"pred.{li}.{pn}"].double().cpu().clone().requires_grad_(True) for pn in ("weight", "bias")) for li in (0, 2, 4, 6, 8)]
    B = alle0.shape[0]
    a64 = alle0.double().clone().requires_grad_(True)
    f64 = feats.double()
    rows = []
    for q in range(6 + 3 * N):
        src = torch.arange(B) if q < 6 else perm[q - 6].long()
        bframe = (1, 3, 4, 0, 2, 3)[q] if q < 6 else (1, 3, 4)[(q - 6) % 3]
        x = r16(torch.cat([a64[src, 0], a64[src, bframe], f64], dim=1))
        for (w, b) in wb[:4]:
            x = r16(torch.relu(r16(x @ r16(w).T) + b))
        rows.append((x @ wb[4][0].T + wb[4][1]).reshape(B))
    s = torch.stack(rows)
    (s * wts.double()).sum().backward()
    return s.detach(), a64.grad, torch.cat([t.grad.reshape(-1) for (w, b) in wb for t in (w, b)])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("N", [0, 1, 5, 16])
def test_reference_style_call_loop_equals_batched_n(hip, N, B, prec):
    """the reference's loop of 6 + 3N get_reward calls with autograd (trainer.py:72-92, restated call for call through the differentiable
    single-call head, which is fp32) against ONE batched_scores pass: scores, d/d alle and every parameter gradient under the loss
    sum(scores * weights). fp32: the gates of tests/test_gpu_lang.py::test_reference_style_15_call_loop_equals_batched (scores 1e-6,
    dalle and each parameter tensor max-rel 1e-4). bf16: the single-call head has no bf16 form, so the loop that the bf16 pass must
    reproduce is the same 6 + 3N calls evaluated one by one in float64 with a bf16 rounding wherever the kernels store bf16
    (_rounding_model_loop: util.langrew_bf16_model's roundings, any N), at the gates tests/test_gpu_lang.py's bf16 test applies to that
    model (scores 2e-3 * max(1, |s|), cosine of dalle and of the parameter gradients >= 0.999). Against the fp32 HIP loop itself the
    gates are those of that bf16 test against the fp32 head: scores 2e-2 * max(1, |s|), cosine of dalle and of the parameter gradients
    >= 0.99. That floor was set for 1024 hidden units; with 64 hidden units and as few as 6 rows, a handful of ReLU units whose
    pre-activation bf16 rounds across zero carry a visible share of the gradient, in any evaluation that stores bf16. So a cosine under
    0.99 passes only by the witness rule of tests/test_gpu_objective.py, with the float64 rounding model as the witness: 1 - cos of the
    GPU result against the fp32 loop may be at most 4 x (1 - cos of the rounding model against the same fp32 loop), a figure the CPU
    computes from the number format alone, per case."""
    from r3m_amd.models_language import LanguageReward
    assert hip.r3m_langrew_workspace_bytes_n(B, 512, 64, 768, N) > 0          # a library without the entry point fails here
    D, H, LD = 512, 64, 768
    perm, alle0, feats, wts = _head_inputs(N, B, D, LD)
    feats, wts = feats.to(DEV), wts.to(DEV)
    loop = LanguageReward(None, D, H, LD)
    loop.load_state_dict(_lang_state(loop))
    loop = loop.to(DEV)
    alle = alle0.clone().to(DEV).requires_grad_(True)
    e0, eg, es0, es1, es2 = (alle[:, i] for i in range(5))
    G = lambda a, b: loop(a, b, feats)[0].reshape(B)
    rows = [G(e0, eg), G(e0, es1), G(e0, es2), G(e0, e0), G(e0, es0), G(e0, es1)]
    for k in range(N):
        for j, other in enumerate((eg, es1, es2)):
            pi = perm[3 * k + j].to(DEV)
            rows.append(G(e0[pi], other[pi]))
    loop_scores = torch.stack(rows)
    loop.mark_grads_stale()
    (loop_scores * wts).sum().backward()
    dalle_loop, grads_loop = alle.grad.clone(), loop.flat_grads().clone()

    rew = LanguageReward(None, D, H, LD, precision=prec)
    rew.load_state_dict(_lang_state(rew))
    rew = rew.to(DEV)
    alle2 = alle0.clone().to(DEV).requires_grad_(True)
    scores = rew.batched_scores(alle2, feats, perm.to(torch.int32).to(DEV))
    assert scores.shape == (6 + 3 * N, B)
    rew.mark_grads_stale()
    (scores * wts).sum().backward()
    gb = rew.flat_grads()
    s_l, s_b = loop_scores.detach().double().cpu(), scores.detach().double().cpu()
    assert bool((alle2.grad.abs().amax(-1) > 0).all()), "a row of dalle got no gradient"
    if prec == "fp32":
        assert rel_err(s_l.numpy(), s_b.numpy())[0] < 1e-6
        e_max, _ = rel_err(dalle_loop.cpu().numpy(), alle2.grad.cpu().numpy())
        print(f"N={N} B={B}: {6 + 3 * N}-call loop vs batched: dalle max-rel {e_max:.3e}")
        assert e_max < 1e-4
        for name, off, shape in rew._layout:
            n = int(np.prod(shape))
            e = rel_err(grads_loop[off:off + n].cpu().numpy(), gb[off:off + n].cpu().numpy())[0]
            assert e < 1e-4, (name, e)
    else:
        def cos(a, b):
            a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
            return float((a * b).sum() / (a.norm() * b.norm()))
        print(f"N={N} B={B} bf16: scores max|d| {float((s_b - s_l).abs().max()):.3e}; cos dalle {cos(alle2.grad, dalle_loop):.6f}, "
              f"cos param grads {cos(gb, grads_loop):.6f}")
        assert float((s_b - s_l).abs().max()) <= 2e-2 * max(1.0, float(s_l.abs().max()))
        s_m, da_m, g_m = _rounding_model_loop(rew, alle0, feats.cpu(), perm, wts.cpu(), N)
        for name, got, loop_v, model in (("dalle", alle2.grad, dalle_loop, da_m), ("param grads", gb[:g_m.numel()], grads_loop[:g_m.numel()], g_m)):
            miss, witness = 1.0 - cos(got, loop_v), 1.0 - cos(model, loop_v)
            print(f"N={N} B={B} bf16 {name}: 1 - cos against the fp32 loop {miss:.3e}; the rounding model against the same loop {witness:.3e}")
            assert miss <= max(0.01, 4.0 * witness), (name, miss, witness)
        err = float((s_b - s_m).abs().max())
        print(f"N={N} B={B} bf16 vs the rounding-model loop: scores max|d| {err:.3e}; cos dalle {cos(alle2.grad, da_m):.6f}, cos param grads "
              f"{cos(gb[:g_m.numel()], g_m):.6f}")
        assert err <= 2e-3 * max(1.0, float(s_m.abs().max()))
        assert cos(alle2.grad, da_m) >= 0.999 and cos(gb[:g_m.numel()], g_m) >= 0.999


def test_head_n_entries_at_three_equal_the_old_entries_bit_for_bit(hip):
    """r3m_langrew_forward_dt / _backward_dt and the `_n` calls with N = 3 on the same inputs, fp32 and bf16: scores, dalle, gradients"""
    from r3m_amd.ops import inverse_permutations
    from util import langrew_layers
    B, D, H, LD = 5, 512, 64, 768
    wsb = hip.r3m_langrew_workspace_bytes_n(B, D, H, LD, 3)
    assert wsb == hip.r3m_langrew_workspace_bytes(B, D, H, LD)
    perm, alle0, feats, wts = _head_inputs(3, B, D, LD)
    layers = langrew_layers(D, H, LD, seed=0)
    flat = torch.cat([t.detach().reshape(-1) for l in layers for t in (l.weight, l.bias)])
    flat = torch.cat([flat, torch.zeros((-flat.numel()) % 4)]).to(DEV)
    alled, featsd, wtsd = alle0.to(DEV), feats.to(DEV), wts.to(DEV).contiguous()
    permd = perm.to(torch.int32).to(DEV).contiguous()
    ipermd = inverse_permutations(permd).contiguous()
    for dt in (0, 1):
        res = []
        for new in (False, True):
            ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
            scores = torch.full((15, B), float("nan"), device=DEV)
            grads = torch.zeros_like(flat)                       # the padding behind the last parameter is not written
            dalle = torch.zeros((B, 5, D), device=DEV)
            a = (alled.data_ptr(), featsd.data_ptr(), permd.data_ptr(), flat.data_ptr(), scores.data_ptr(), ws.data_ptr(), wsb, B, D, H, LD)
            b = (wtsd.data_ptr(), ipermd.data_ptr(), flat.data_ptr(), grads.data_ptr(), dalle.data_ptr(), ws.data_ptr(), wsb, B, D, H, LD)
            if new:
                assert hip.r3m_langrew_forward_n(*a, 3, dt, _st()) == 0, hip.r3m_last_error()
                assert hip.r3m_langrew_backward_n(*b, 3, 0, dt, _st()) == 0, hip.r3m_last_error()
            else:
                assert hip.r3m_langrew_forward_dt(*a, dt, _st()) == 0, hip.r3m_last_error()
                assert hip.r3m_langrew_backward_dt(*b, 0, dt, _st()) == 0, hip.r3m_last_error()
            torch.cuda.synchronize()
            res.append((scores, grads, dalle))
        for x, y in zip(*res):
            assert bool(torch.isfinite(x).all()) and torch.equal(x, y), dt


# ---- the reference's own runs with num_negatives 1 and 5 through the HIP path ----------------------------------------------------------
@pytest.mark.parametrize("l2dist", [True, False], ids=["l2dist", "cosine"])
@pytest.mark.parametrize("N", [1, 5])
def test_reference_goldens_with_num_negatives(hip, golden_dir, N, l2dist):
    """tests/golden/loss_neg{N}_*.npz (the reference's Trainer.update with model.module.num_negatives = N): first the TCN + LP part at the
    gates of tests/test_gpu_encoder.py::test_tcn_lp_loss_matches_reference_golden, then the whole objective with the language head at the
    gates of tests/test_gpu_lang.py::test_full_loss_with_language_matches_reference_golden"""
    from oracle import detgen, r3m_ref
    from r3m_amd import ops
    from r3m_amd.models_language import LanguageReward
    assert hip.r3m_loss_workspace_bytes_n(8, N) > 0                           # a library without the entry point fails here
    sys.path.insert(0, golden_dir)
    from make_golden import make_alle
    g = np.load(os.path.join(golden_dir, f"loss_neg{N}_{'l2' if l2dist else 'cos'}.npz"))
    B, D = 8, 512
    perms = torch.from_numpy(g["perms"])
    lang_perm, tcn_perm = perms[:3 * N], perms[3 * N:5 * N]
    ref = dict(zip([str(n) for n in g["metric_names"]], g["metric_values"]))
    # TCN + LP
    alle = torch.from_numpy(make_alle(B, D, "alle")).to(DEV).requires_grad_(True)
    full, m = ops.r3m_loss(alle, tcn_perm.to(torch.int32).to(DEV), 1e-5, 1e-5, 1.0, l2dist=l2dist, num_negatives=N)
    got = m.cpu().numpy()
    for k in ("l2loss", "l1loss", "l0loss", "tcnloss", "aligned"):
        assert abs(got[ops.METRIC_SLOTS[k]] - ref[k]) <= 1e-5 * max(1.0, abs(ref[k])), (k, got[ops.METRIC_SLOTS[k]], ref[k])
    mref = r3m_ref.R3MRef(size=18, l2weight=1e-5, l1weight=1e-5, langweight=0.0, tcnweight=1.0, l2dist=l2dist)
    mref.num_negatives = N
    a2 = alle.detach().cpu().requires_grad_(True)
    fl, met, _ = r3m_ref.r3m_loss_ref(mref, a2, tcn_perm=tcn_perm)
    fl.backward()
    assert abs(float(full) - met["full_loss"]) <= 1e-5 * abs(met["full_loss"])
    full.backward()
    assert rel_err(alle.grad.cpu().numpy(), a2.grad.numpy())[0] < 1e-4
    # the whole objective
    rew = LanguageReward(None, D, 1024, 768)
    rew.load_state_dict(_lang_state(rew))
    rew = rew.to(DEV)
    alle = torch.from_numpy(make_alle(B, D, "alle")).to(DEV).requires_grad_(True)
    feats = torch.from_numpy(detgen.uniform("langfeat", (B, 768), -0.6, 0.6)).to(DEV)
    mask = torch.ones(B)
    mask[5] = 0.0
    scores = rew.batched_scores(alle, feats, lang_perm.to(torch.int32).to(DEV))
    assert rel_err(scores.detach().cpu().numpy(), g["scores"])[0] < 1e-5
    full, m = ops.r3m_loss(alle, tcn_perm.to(torch.int32).to(DEV), 1e-5, 1e-5, 1.0, l2dist=l2dist, scores=scores, mask=mask.to(DEV),
                           langweight=1.0, num_negatives=N)
    got = m.cpu().numpy()
    for k, v in ref.items():
        assert abs(got[ops.METRIC_SLOTS[k]] - v) <= 1e-5 * max(1.0, abs(v)), (k, got[ops.METRIC_SLOTS[k]], v)
    rew.mark_grads_stale()
    full.backward()
    assert rel_err(alle.grad.cpu().numpy(), g["dalle"])[0] < 1e-4
    P = dict(rew.named_parameters())
    for k, p in P.items():
        ref_n = float(g["gradnorm_" + k])
        if k == "pred.8.bias":       # the sum of d loss / d score over all scores: each clip's InfoNCE gradients sum to 0, so the reference's
            # own value is its rounding residue (1.5e-8 / 6.0e-8 in these files). No relative gate applies to that; the absolute one of
            # tests/test_gpu_lang.py::test_reference_style_15_call_loop_equals_batched for this tensor does.
            assert ref_n < 1e-6 and abs(float(p.grad.double().norm()) - ref_n) < 1e-6, k
            continue
        assert abs(float(p.grad.double().norm()) - ref_n) <= 1e-4 * max(ref_n, 1e-12), k
    assert rel_err(P["pred.8.weight"].grad.cpu().numpy(), g["grad_pred.8.weight"])[0] < 1e-4
    assert rel_err(P["pred.0.bias"].grad.cpu().numpy(), g["grad_pred.0.bias"])[0] < 1e-4


# ---- whole steps ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5])
def test_whole_steps_with_num_negatives_vs_oracle(hip, N):
    """R3M(size=18, num_negatives=N), B = 2 clips, language and time-contrastive loss on: an eval step, a training step, then
    model.num_negatives = 2 and another training step, each against oracle.r3m_ref.train_step_ref with the same attribute and the
    permutations the update is about to draw. Gates of the G5 step test (tests/test_gpu_encoder.py): 2e-4 * max(1, |ref|) while the
    weights are identical, 5e-3 after an Adam step. The torch CPU generator must end where the oracle side's draws end: 3N language
    permutations, then 2N."""
    from oracle import detgen, r3m_ref
    from r3m_amd import R3M
    from r3m_amd.parallel import SingleDevice
    from r3m_amd.trainer import Trainer
    B = 2
    m = R3M("cuda", 1e-4, 1024, size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=1.0, num_negatives=N)   # TypeError without the keyword
    assert m.num_negatives == N
    shapes = [(k, tuple(v.shape)) for k, v in m.convnet.state_dict().items()]
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes).items()}
    m.convnet.load_state_dict(sd)
    lsd = _lang_state(m.lang_rew)
    m.lang_rew.load_state_dict(lsd)
    ref = r3m_ref.R3MRef(size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=1.0)
    ref.num_negatives = N
    ref.convnet.load_state_dict(sd)
    ref.lang_rew.load_state_dict(lsd)
    model = SingleDevice(m).to(DEV)
    frames = torch.from_numpy(detgen.frames("negstep", (B, 5, 3, 224, 224)))
    feats = torch.from_numpy(detgen.uniform("langfeat", (B, 768), -0.6, 0.6))
    mask = torch.tensor([1.0, 0.0])
    T = Trainer(1)
    for step, (n, ev, tol) in enumerate(((N, True, 2e-4), (N, False, 2e-4), (2, False, 5e-3))):
        m.num_negatives = ref.num_negatives = n
        torch.manual_seed(40 + step)
        lang_perm = torch.stack([torch.randperm(B) for _ in range(3 * n)])
        tcn_perm = torch.stack([torch.randperm(B) for _ in range(2 * n)])
        state_after = torch.get_rng_state()
        torch.manual_seed(40 + step)
        metrics, _ = T.update(model, (frames.to(DEV), (feats.to(DEV), mask)), step, eval=ev)
        assert torch.equal(torch.get_rng_state(), state_after), "the update drew a different number of permutations"
        mref = r3m_ref.train_step_ref(ref, frames, tcn_perm=tcn_perm, lang_feats=feats, lang_mask=mask, lang_perm=lang_perm, eval=ev)
        assert set(metrics.keys()) == set(mref.keys())
        print(f"N={n} eval={ev}: " + ", ".join(f"{k} {metrics[k]:.6g} (ref {v:.6g})" for k, v in mref.items()))
        for k, v in mref.items():
            assert abs(metrics[k] - v) <= tol * max(1.0, abs(v)), (step, n, k, metrics[k], v)


def test_whole_step_without_cross_clip_negatives(hip):
    """num_negatives = 0 with the time-contrastive loss off: Trainer.update draws nothing, builds an empty [0, B] language permutation
    and runs the language loss with its in-clip negative alone -- an eval step and a training step against train_step_ref with the same
    attribute, at the 2e-4 gate of the step tests (identical weights)."""
    from oracle import detgen, r3m_ref
    from r3m_amd import R3M
    from r3m_amd.parallel import SingleDevice
    from r3m_amd.trainer import Trainer
    B = 2
    m = R3M("cuda", 1e-4, 1024, size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=0.0, num_negatives=0)
    shapes = [(k, tuple(v.shape)) for k, v in m.convnet.state_dict().items()]
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes).items()}
    m.convnet.load_state_dict(sd)
    lsd = _lang_state(m.lang_rew)
    m.lang_rew.load_state_dict(lsd)
    ref = r3m_ref.R3MRef(size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=0.0)
    ref.convnet.load_state_dict(sd)
    ref.lang_rew.load_state_dict(lsd)
    model = SingleDevice(m).to(DEV)
    frames = torch.from_numpy(detgen.frames("negstep", (B, 5, 3, 224, 224)))
    feats = torch.from_numpy(detgen.uniform("langfeat", (B, 768), -0.6, 0.6))
    mask = torch.tensor([1.0, 1.0])
    T = Trainer(1)
    for step, (n, ev) in enumerate(((0, True), (0, False))):
        m.num_negatives = ref.num_negatives = n
        torch.manual_seed(50 + step)
        before = torch.get_rng_state()
        metrics, _ = T.update(model, (frames.to(DEV), (feats.to(DEV), mask)), step, eval=ev)
        assert torch.equal(torch.get_rng_state(), before), "a step without negatives drew a permutation"
        mref = r3m_ref.train_step_ref(ref, frames, lang_feats=feats, lang_mask=mask, lang_perm=torch.zeros((0, B), dtype=torch.int64), eval=ev)
        assert set(metrics.keys()) == set(mref.keys()) and "tcnloss" not in metrics
        for k, v in mref.items():
            assert abs(metrics[k] - v) <= 2e-4 * max(1.0, abs(v)), (step, k, metrics[k], v)
