"""-m gpu: the language-reward head (csrc/lang.hip) through the C ABI against a float64 torch MLP evaluated call by call on the CPU, at the
row counts the workload runs (256 / 512 clips = 3840 / 7680 rows) stand for -- tests/test_gpu_lang.py stops at 16 clips, 240 rows:

  * colsum_partial_kernel / colsum_final_kernel (all five bias gradients and the last layer's weight gradient): R = 15 x 275 = 4125 and
    R = 4097 rows are past 4096, where colsum_slices caps at 64 slices, rows_per_slice becomes 65 and the last slice is short (30 rows of
    65 at R = 4125, 2 at R = 4097); R = 1035 and 65 stay under the cap with a ragged last slice; R = 1 and 15 are a single slice;
  * the head's Linear layers on the conv GEMMs as R one-pixel images, with the epilogues nothing else asks: bias + ReLU (flags 24)
    forward, ReLU mask on the stored input gradient (flags 32), many row tiles with a partial last one at R = 4125; K1 = 96 / 128 / 192
    and 64- / 128-wide outputs (tests/test_dispatch.py checks on the CPU that these cases hold every dispatch signature of the workload's
    head: (1, 32, 128, 32) is here for route 22 with 128-wide outputs);
  * lang_scatter_kernel ADDS into dalle: dalle enters holding a known non-zero pattern and must come out as pattern + reference;
  * accumulate = 1 of r3m_langrew_backward / _call_backward on pre-filled grads, otherwise reached only through the module.

Ceilings: those of test_langrew_c_abi_vs_torch (scores 2e-5, dalle and each of the ten parameter gradients 1e-4, max-rel against
float64); bf16: the checks and ceilings of test_bf16_head_follows_fp32_head_and_its_own_rounding_model. Outputs enter NaN-filled
(accumulated ones hold the pattern), the workspace is the reported size, NaN-filled, plus a 256-byte guard that must come back intact.

Kink rule: no hidden pre-activation of the float64 MLP may lie within 1e-5 of zero relative to its layer's largest -- a float32 ReLU may
decide such an element the other way, and a flipped mask is a gradient error of a whole term, not of rounding size. A plain redraw cannot
reach that at these sizes (R = 4125 rows x 128 units x 4 layers is 2.1 M pre-activations: about 40 of any draw are that close), so the
builder first moves the fp32 bias of every offending unit, layer by layer, by the smallest multiple of 2e-5 of the layer's range that
clears all rows, then checks the rule on the result in float64 and only then falls back to the next seed."""
import copy
import functools

import numpy as np
import pytest
import torch

from util import (DEV, LANG_BFRAME, _st, assert_edge_figures, assert_guard_intact, guarded_bytes, langrew_bf16_model, langrew_layers,
                  langrew_scores_call_by_call, rel_err, rnd)

pytestmark = pytest.mark.gpu

# (B, D, H, LD): what the case reaches
FP32_CASES = [(1, 32, 64, 32),        # R = 15 rows, K1 = 96
              (1, 32, 128, 64),       # K1 = 128, outputs a multiple of 128 wide
              (1, 32, 128, 32),       # K1 = 96 with 128-wide outputs: the forward GEMM without LDS-direct loads (route 22) on the 128-wide tile
              (69, 64, 64, 64),       # R = 1035
              (275, 32, 64, 32),      # R = 4125 > 4096: capped slices, rows_per_slice = 65, short last slice, many row tiles + a partial one
              (275, 32, 128, 64)]     # the same, K1 = 128, 128-wide outputs
BF16_CASES = [(1, 32, 64, 64), (275, 32, 128, 64)]          # dt = 1 needs LD % 64 == 0
CALL_ROWS = [1, 65, 4097]
CALL_DIMS = (32, 64, 32)                                     # (D, H, LD) of the single-call cases
KINK = 1e-5
WITNESSED = ()                                               # no figure here may use the witness rule


def mlp_preacts(layers, X):
    """float64 hidden pre-activations [R,H] x 4 of the rows X"""
    out, x = [], X
    for l in layers[:4]:
        z = x @ l.weight.double().T + l.bias.double()
        out.append(z)
        x = torch.relu(z)
    return out


def settle_kinks(layers, X):
    """move fp32 biases until no pre-activation is within 2 x KINK of zero relative to its layer's largest (module docstring)"""
    with torch.no_grad():
        for li in range(4):
            Z = mlp_preacts(layers, X)[li]
            tau = 2 * KINK * float(Z.abs().max())
            for u in torch.nonzero((Z.abs() < tau).any(0)).flatten().tolist():
                z, b0 = Z[:, u], layers[li].bias[u].clone()
                for k in range(1, 2000):
                    done = False
                    for sgn in (1.0, -1.0):
                        b1 = (b0.double() + sgn * k * tau).float()
                        if float((z + (b1.double() - b0.double())).abs().min()) >= tau:
                            layers[li].bias[u] = b1
                            done = True
                            break
                    if done:
                        break
        return all(float(Z.abs().min()) > KINK * float(Z.abs().max()) for Z in mlp_preacts(layers, X))


def gathered_rows(alle, feats, perm):
    """X [15 B, 2 D + LD] of the batched pass (csrc/lang.hip lang_gather_kernel), float64"""
    B = alle.shape[0]
    rows = []
    for q in range(15):
        src = torch.arange(B) if q < 6 else perm[q - 6]
        rows.append(torch.cat([alle[src, 0], alle[src, LANG_BFRAME[q]], feats], dim=1))
    return torch.cat(rows, dim=0).double()


def flat_of(layers, grad=False):
    return torch.cat([(t.grad if grad else t.detach()).reshape(-1) for l in layers for t in (l.weight, l.bias)])


@functools.lru_cache(maxsize=None)
def batched_case(B, D, H, LD):
    """inputs (CPU fp32) and the float64 / float32 results of sum(scores * dscore): relu(uniform) embeddings, permutation row 4 the
    identity, kink rule enforced"""
    for seed in range(20):
        layers = langrew_layers(D, H, LD, seed=seed)
        alle = torch.relu(rnd((B, 5, D), 601 + 10 * seed, -0.5, 1.0))
        feats = rnd((B, LD), 602 + 10 * seed, -0.6, 0.6)
        g = torch.Generator().manual_seed(603 + 10 * seed)
        perm = torch.stack([torch.randperm(B, generator=g) for _ in range(9)])
        perm[4] = torch.arange(B)
        if settle_kinks(layers, gathered_rows(alle, feats, perm)):
            break
    else:
        raise AssertionError(f"no draw of {(B, D, H, LD)} satisfies the kink rule")
    dscore = rnd((15, B), 604, -1.0, 1.0)
    res = {}
    for dt in (torch.float64, torch.float32):
        ls = [copy.deepcopy(l).to(dt) for l in layers]
        a = alle.to(dt).clone().requires_grad_(True)
        sc = langrew_scores_call_by_call(ls, a, feats.to(dt), perm)
        (sc * dscore.to(dt)).sum().backward()
        res[dt] = (sc.detach().double().numpy(), a.grad.double().numpy(), flat_of(ls, grad=True).double().numpy())
    return layers, alle, feats, perm, dscore, res[torch.float64], res[torch.float32]


def tensor_slices(D, H, LD):
    """[(name, offset, count)] of the ten tensors in the flat layout pred.{0,2,4,6,8}.{weight,bias}"""
    K1, out, off = 2 * D + LD, [], 0
    for li, (i, o) in enumerate([(K1, H), (H, H), (H, H), (H, H), (H, 1)]):
        for name, k in (("weight", i * o), ("bias", o)):
            out.append((f"pred.{2 * li}.{name}", off, k))
            off += k
    return out


def pattern_like(ref, seed):
    """a known non-zero pattern on the scale of `ref` (numpy float64): +-uniform(0.5, 1.5) x max|ref|, as fp32"""
    t = rnd(ref.shape, seed, 0.5, 1.5) * torch.where(rnd(ref.shape, seed + 1) > 0, 1.0, -1.0) * float(np.abs(ref).max())
    assert bool((t != 0).all())
    return t


def grads_pattern(ref_flat, D, H, LD, seed):
    """pattern_like per tensor: each of the ten on its own gradient's scale"""
    return torch.cat([pattern_like(ref_flat[off:off + k], seed + 2 * i) for i, (_, off, k) in enumerate(tensor_slices(D, H, LD))])


def grad_figures(got_flat, ref_flat, D, H, LD, minus=None):
    """{tensor name: max-rel} of the ten parameter gradients; minus: the pattern the buffer held before an accumulating call"""
    got = got_flat if minus is None else got_flat - minus
    return {name: rel_err(got[off:off + k], ref_flat[off:off + k])[0] for (name, off, k) in tensor_slices(D, H, LD)}


def colsum_fixed_order(A):
    """the column sums of A [R,C] (numpy float32) in the order csrc/lang.hip documents as fixed, restated add for add: colsum_slices =
    min(ceil(R / 64), 64) slices of ceil(R / slices) rows; inside a slice four row lanes (rows r0 + lane, + 4, ...) each add their rows in
    order, combined as (l0 + l1) + (l2 + l3); the slices are then added in order. Every operation is one fp32 addition, so numpy float32
    reproduces the kernels bit for bit. A launcher that cuts the rows differently (63 slices at the cap, say) still sums correctly -- no
    tolerance can see it -- but gives other bits here; whoever changes the geometry on purpose restates it here."""
    R, C = A.shape
    S = min(max(-(-R // 64), 1), 64)
    rps = -(-R // S)
    out = np.zeros(C, dtype=np.float32)
    for sl in range(S):
        r0, r1 = sl * rps, min(sl * rps + rps, R)
        lanes = []
        for ty in range(4):
            acc = np.zeros(C, dtype=np.float32)
            for r in range(r0 + ty, r1, 4):
                acc = acc + A[r]
            lanes.append(acc)
        out = out + ((lanes[0] + lanes[1]) + (lanes[2] + lanes[3]))
    assert out.dtype == np.float32
    return out, S, rps


class Head:
    """device buffers of one case: parameters padded to a multiple of 4 floats, NaN-filled workspace of the reported size + guard"""

    def __init__(self, hip, layers, D, H, LD, wsb):
        self.hip, self.dims = hip, (D, H, LD)
        flat = flat_of(layers)
        self.n = hip.r3m_langrew_num_params(D, H, LD)
        assert self.n == flat.numel()
        self.pad = (-self.n) % 4
        self.params = torch.cat([flat, torch.zeros(self.pad)]).to(DEV)
        self.wsb = wsb
        self.ws = guarded_bytes(wsb)
        self.ws[:wsb] = 0xFF

    def grads_buffer(self, pattern=None):
        g = torch.full((self.n + self.pad,), float("nan"), device=DEV)
        if pattern is not None:
            g[:self.n] = pattern.to(DEV)
        return g

    def done(self, what):
        torch.cuda.synchronize()
        assert_guard_intact(self.ws, self.wsb, what)


def run_batched(hip, case, dt):
    """forward, backward (accumulate 0, dalle holding a pattern), backward again (accumulate 1 on pre-filled grads, dalle holding a
    second pattern) -> scores, dalle - pattern, grads, dalle2 - pattern2, grads2 - pattern (numpy float64)"""
    B, D, H, LD = case
    layers, alle, feats, perm, dscore, r64, _ = batched_case(*case)
    from r3m_amd.ops import inverse_permutations
    head = Head(hip, layers, D, H, LD, hip.r3m_langrew_workspace_bytes(B, D, H, LD))
    alled, featsd, dsd = alle.to(DEV), feats.to(DEV), dscore.to(DEV)
    permd = perm.to(torch.int32).to(DEV).contiguous()
    ipermd = inverse_permutations(permd).contiguous()
    scores = torch.full((15, B), float("nan"), device=DEV)
    rc = hip.r3m_langrew_forward_dt(alled.data_ptr(), featsd.data_ptr(), permd.data_ptr(), head.params.data_ptr(), scores.data_ptr(),
                                    head.ws.data_ptr(), head.wsb, B, D, H, LD, dt, _st())
    assert rc == 0, hip.r3m_last_error()
    out = [scores.cpu().double().numpy()]
    gpat = grads_pattern(r64[2], D, H, LD, 620)
    for acc, seed in ((0, 610), (1, 612)):
        pat = pattern_like(r64[1], seed)
        dalle = pat.to(DEV)
        grads = head.grads_buffer(gpat if acc else None)
        rc = hip.r3m_langrew_backward_dt(dsd.data_ptr(), ipermd.data_ptr(), head.params.data_ptr(), grads.data_ptr(), dalle.data_ptr(),
                                         head.ws.data_ptr(), head.wsb, B, D, H, LD, acc, dt, _st())
        assert rc == 0, hip.r3m_last_error()
        head.done(f"langrew workspace {case} dt={dt} accumulate={acc}")
        out.append(dalle.cpu().double().numpy() - pat.double().numpy())
        g = grads[:head.n].cpu().double().numpy()
        out.append(g - gpat.double().numpy() if acc else g)
    if dt == 0:          # the plain entry points are the same pass: r3m_langrew_forward == r3m_langrew_forward_dt(R3M_DT_F32)
        s2 = torch.full((15, B), float("nan"), device=DEV)
        rc = hip.r3m_langrew_forward(alled.data_ptr(), featsd.data_ptr(), permd.data_ptr(), head.params.data_ptr(), s2.data_ptr(), head.ws.data_ptr(),
                                     head.wsb, B, D, H, LD, _st())
        assert rc == 0, hip.r3m_last_error()
        g2 = head.grads_buffer()
        rc = hip.r3m_langrew_backward(dsd.data_ptr(), ipermd.data_ptr(), head.params.data_ptr(), g2.data_ptr(), None, head.ws.data_ptr(), head.wsb,
                                      B, D, H, LD, 0, _st())
        assert rc == 0, hip.r3m_last_error()
        head.done(f"langrew workspace {case} plain entry points")
        assert torch.equal(s2, scores) and np.array_equal(g2[:head.n].cpu().double().numpy(), out[2])      # dalle = NULL changes nothing else
    return out


@pytest.mark.parametrize("B,D,H,LD", FP32_CASES, ids=["x".join(map(str, c)) for c in FP32_CASES])
def test_batched_head_fp32_against_float64(hip, B, D, H, LD):
    """r3m_langrew_forward[_dt] / _backward[_dt], fp32: scores at 2e-5; dalle (pattern + reference) and each of the ten parameter
    gradients at 1e-4, with accumulate 0 and 1. Paths first reached here: colsum_partial_kernel / colsum_final_kernel past the 64-slice
    cap with rows_per_slice = 65 and a short last slice -- (275, ...); lang_scatter_kernel adding into a non-zero dalle and
    accumulate = 1 -- every case; the conv GEMMs' epilogues 24 and 32 with many row tiles and a partial one -- (275, ...)."""
    case = (B, D, H, LD)
    _, _, _, perm, _, r64, r32 = batched_case(*case)
    assert bool((perm[4] == torch.arange(B)).all())
    scores, dalle, grads, dalle_acc, grads_acc = run_batched(hip, case, 0)
    what = f"langrew fp32 B={B} D={D} H={H} LD={LD}"
    figs = {"scores": rel_err(scores, r64[0])[0], "dalle": rel_err(dalle, r64[1])[0], "dalle (accumulate run)": rel_err(dalle_acc, r64[1])[0]}
    wit = {"scores": rel_err(r32[0], r64[0])[0], "dalle": rel_err(r32[1], r64[1])[0], "dalle (accumulate run)": rel_err(r32[1], r64[1])[0]}
    for tag, g in (("", grads), (" += ", grads_acc)):
        for k, e in grad_figures(g, r64[2], D, H, LD).items():
            figs[f"grad{tag} {k}"] = e
        for k, e in grad_figures(r32[2], r64[2], D, H, LD).items():
            wit[f"grad{tag} {k}"] = e
    ceil = {k: (2e-5 if k == "scores" else 1e-4) for k in figs}
    assert_edge_figures(what, figs, wit, ceil, WITNESSED)


@pytest.mark.parametrize("B,D,H,LD", BF16_CASES, ids=["x".join(map(str, c)) for c in BF16_CASES])
def test_batched_head_bf16_follows_fp32_head_and_its_rounding_model(hip, B, D, H, LD):
    """r3m_langrew_forward_dt / _backward_dt with R3M_DT_BF16 at R = 15 and R = 4125, by the two checkers and the ceilings of
    tests/test_gpu_lang.py::test_bf16_head_follows_fp32_head_and_its_own_rounding_model: the fp32 head on the same inputs (scores
    2e-2 of their range, cosines >= 0.99) and the float64 MLP with a bf16 rounding where the kernel stores bf16 (scores 2e-3, cosines
    >= 0.999). Paths first reached here: colsum_partial_kernel<bf16> past the slice cap, the bf16 scatter into a non-zero dalle,
    accumulate = 1 of the bf16 backward."""
    case = (B, D, H, LD)
    layers, alle, feats, perm, dscore, _, _ = batched_case(*case)
    s32, da32, g32, _, _ = run_batched(hip, case, 0)
    s16, da16, g16, da16_acc, g16_acc = run_batched(hip, case, 1)
    wb = [(l.weight.detach().double().clone().requires_grad_(True), l.bias.detach().double().clone().requires_grad_(True)) for l in layers]
    s_model, da_model, g_model = langrew_bf16_model(wb, alle, feats, perm, dscore)
    s_model, da_model, g_model = s_model.numpy(), da_model.numpy(), g_model.numpy()

    def cos(a, b):
        return float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)))
    d32, dm = float(np.abs(s16 - s32).max()), float(np.abs(s16 - s_model).max())
    print(f"EDGE langrew bf16 B={B} D={D} H={H} LD={LD} | scores max|d| vs fp32 head {d32:.3e} (max|s| {float(np.abs(s32).max()):.3f}), vs rounding "
          f"model {dm:.3e}; cos dalle {cos(da16, da32):.6f} / {cos(da16, da_model):.6f}, cos grads {cos(g16, g32):.6f} / {cos(g16, g_model):.6f}; "
          f"accumulate run: cos dalle {cos(da16_acc, da_model):.6f}, cos grads {cos(g16_acc, g_model):.6f}", flush=True)
    assert d32 <= 2e-2 * max(1.0, float(np.abs(s32).max()))
    assert cos(da16, da32) >= 0.99 and cos(g16, g32) >= 0.99
    assert dm <= 2e-3 * max(1.0, float(np.abs(s_model).max()))
    assert cos(da16, da_model) >= 0.999 and cos(g16, g_model) >= 0.999
    assert cos(da16_acc, da_model) >= 0.999 and cos(g16_acc, g_model) >= 0.999


@functools.lru_cache(maxsize=None)
def call_case(R):
    D, H, LD = CALL_DIMS
    for seed in range(20):
        layers = langrew_layers(D, H, LD, seed=100 + seed)
        e0 = torch.relu(rnd((R, D), 701 + 10 * seed, -0.5, 1.0))
        eg = torch.relu(rnd((R, D), 702 + 10 * seed, -0.5, 1.0))
        le = rnd((R, LD), 703 + 10 * seed, -0.6, 0.6)
        if settle_kinks(layers, torch.cat([e0, eg, le], 1).double()):
            break
    else:
        raise AssertionError(f"no draw of R={R} satisfies the kink rule")
    ds = rnd((R,), 704, -1.0, 1.0)
    res = {}
    for dt in (torch.float64, torch.float32):
        ls = [copy.deepcopy(l).to(dt) for l in layers]
        x = [t.to(dt).clone().requires_grad_(True) for t in (e0, eg, le)]
        h = torch.cat(x, -1)
        for l in ls[:-1]:
            h = torch.relu(l(h))
        sc = ls[-1](h).squeeze(-1)
        (sc * ds.to(dt)).sum().backward()
        res[dt] = (sc.detach().double().numpy(), [t.grad.double().numpy() for t in x], flat_of(ls, grad=True).double().numpy())
    return layers, e0, eg, le, ds, res[torch.float64], res[torch.float32]


@pytest.mark.parametrize("R", CALL_ROWS)
def test_single_call_head_against_float64(hip, R):
    """r3m_langrew_call_forward / _call_backward at R = 1, 65, 4097 rows: score at 2e-5; de0, deg, dle (WRITTEN: they enter NaN-filled)
    and each of the ten parameter gradients at 1e-4, with accumulate 0 and 1. Paths first reached here: the column sums past the slice
    cap with a last slice of 2 rows (R = 4097), one row over a single slice (R = 65: two slices of 33 and 32 rows), R = 1. The
    bias gradient of the last hidden layer is also compared BIT FOR BIT with the documented fixed-order sum (colsum_fixed_order): the
    slice count and rows_per_slice of launch_colsum are pinned, which no tolerance can do."""
    D, H, LD = CALL_DIMS
    layers, e0, eg, le, ds, r64, r32 = call_case(R)
    head = Head(hip, layers, D, H, LD, hip.r3m_langrew_call_workspace_bytes(R, D, H, LD))
    e0d, egd, led, dsd = (t.to(DEV) for t in (e0, eg, le, ds))
    score = torch.full((R,), float("nan"), device=DEV)
    rc = hip.r3m_langrew_call_forward(e0d.data_ptr(), egd.data_ptr(), led.data_ptr(), head.params.data_ptr(), score.data_ptr(), head.ws.data_ptr(),
                                      head.wsb, R, D, H, LD, _st())
    assert rc == 0, hip.r3m_last_error()
    figs = {"score": rel_err(score.cpu().double().numpy(), r64[0])[0]}
    wit = {"score": rel_err(r32[0], r64[0])[0]}
    gpat = grads_pattern(r64[2], D, H, LD, 720)
    for acc in (0, 1):
        outs = [torch.full(t.shape, float("nan"), device=DEV) for t in (e0, eg, le)]
        grads = head.grads_buffer(gpat if acc else None)
        rc = hip.r3m_langrew_call_backward(dsd.data_ptr(), head.params.data_ptr(), grads.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                           outs[2].data_ptr(), head.ws.data_ptr(), head.wsb, R, D, H, LD, acc, _st())
        assert rc == 0, hip.r3m_last_error()
        head.done(f"langrew call workspace R={R} accumulate={acc}")
        tag = " += " if acc else ""
        for name, o, ref, w in zip(("de0", "deg", "dle"), outs, r64[1], r32[1]):
            figs[f"{name}{tag}"] = rel_err(o.cpu().double().numpy(), ref)[0]
            wit[f"{name}{tag}"] = rel_err(w, ref)[0]
        g = grads[:head.n].cpu().double().numpy()
        if not acc:
            # pred.6.bias = column sums of dZ4[r, k] = H4[r, k] > 0 ? dscore[r] * w5[k] : 0 (one fp32 product each, the mask decided by
            # pre-activations the kink rule keeps clear of zero): known to the bit, so the sum must be THE fixed-order sum
            with torch.no_grad():
                on = (mlp_preacts(layers, torch.cat([e0, eg, le], 1).double())[3] > 0).numpy()
            dz4 = np.where(on, ds.numpy()[:, None] * layers[4].weight.detach().numpy()[0][None, :], np.float32(0)).astype(np.float32)
            want, S, rps = colsum_fixed_order(dz4)
            name, off, k = tensor_slices(D, H, LD)[7]
            assert name == "pred.6.bias" and (R != 4097 or (S, rps, R - (S - 1) * rps) == (64, 65, 2)) and (R != 65 or (S, rps) == (2, 33))
            got_b = grads[off:off + k].cpu().numpy()
            assert np.array_equal(got_b, want), f"R={R}: pred.6.bias is not the fixed-order column sum ({S} slices of {rps} rows): " \
                                                 f"{int((got_b != want).sum())} of {k} columns differ, max |d| {float(np.abs(got_b - want).max()):.3e}"
        for k, e in grad_figures(g, r64[2], D, H, LD, minus=gpat.double().numpy() if acc else None).items():
            figs[f"grad{tag} {k}"] = e
        for k, e in grad_figures(r32[2], r64[2], D, H, LD).items():
            wit[f"grad{tag} {k}"] = e
    ceil = {k: (2e-5 if k == "score" else 1e-4) for k in figs}
    assert_edge_figures(f"langrew call R={R}", figs, wit, ceil, WITNESSED)
