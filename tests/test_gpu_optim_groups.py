"""-m gpu: parameter groups, weight decay and gradient clipping of the fused optimizers: r3m_adam_step_groups / r3m_sgd_step_groups /
r3m_grad_sqnorm_ranges / r3m_clip_coef (csrc/adam.hip) at the C ABI, then through FusedAdam / FusedAdamW / FusedSGD, the encoder and the
data-parallel wrapper.

1. Bit identity. With every weight decay 0, one learning rate and a NULL coefficient a block of the step kernels runs the plain element
   loop (adam_span_t<false, 0> / sgd_span_t<false>), which is all that r3m_adam_step_ranges / r3m_sgd_step_ranges ask of the same
   kernels, so the result must be torch.equal to theirs (the CASES of tests/optim_cases.py): a wrongly replicated learning rate shows.
   A coefficient buffer holding 1.0f must give the same bits too: here grad_scale = 0.5, so g * grad_scale is exact and the extra
   multiplication by 1 changes nothing (include/r3m_hip.h says when that holds).

2. One grouped Adam step against float64. The bounds extend the derivation of tests/test_gpu_optim_steps.py (its docstring; u = 2^-24,
   the float64 reference uses the very fp32 scalars the launcher passes, a fused multiply-add only removes roundings). What changes is the
   error E_g of the gradient gr that enters the moments, and one rounding on p:
     gr0 = g * grad_scale                      E_g = u |gr0|
     gr1 = gr0 * coef (coefficient given)      one more rounding: E_g = 2 u |gr1|
     gr  = gr1 + wd * p (L2 mode, wd != 0)     a product and a sum more: E_g = E_g(gr1) + u |wd p| + u |gr|
     p1  = p * f, f = (float)(1 - lr wd) (decoupled mode, wd != 0): one product, E_p = u |p1|; otherwise p1 = p, E_p = 0
   and with S_m = max(|m|, |gr|), S_v = max(v, gr^2), a = (float)(1 - beta1), c = (float)(1 - beta2):
     m' : the error of gr arrives as a E_g; subtraction, product and sum add u (0.2 + 0.2 + 1) S_m.          BOUND a E_g + 1.9 u S_m
          (with E_g = u |gr| that is within the 2 u S_m of test_gpu_optim_steps.py)
     v' : gr^2 carries 2 |gr| E_g + E_g^2, the two products 2 u gr^2, v * beta2 one, the sum one.
                                                                                         BOUND c (2 |gr| E_g + E_g^2) + (2 c + 2.5) u S_v
     denom = sqrtf(v') / bc2_sqrt + eps: half the relative error r_v of v', then root, quotient and sum.    RELATIVE r_d = r_v / 2 + 3 u
     U = (neg_step * m') / denom:                                              BOUND |neg_step| / denom * (bound on m') + (2 u + r_d) |U|
     p' = p1 + U:                                                                               BOUND u |p'| + E_p + the bound on U
   The halving of r_v is the first-order term of the root: the test asserts r_v < 2^-10 on the float64 side and widens every bound by
   (1 + 2^-9) for the second-order terms. No bound comes from a measurement of the kernel.

3. The squared norm against math.fsum of the (exact) float64 squares. All terms are non-negative, so the relative error is at most the
   number of roundings a term passes through, in units of 2^-53: per lane 4 adds per trip of its grid-stride loop; 6 for the shuffle tree
   of the wave, 3 for the four waves; in the second kernel ceil(blocks / 256) adds per lane, 6 + 3 again; 1 for every addition to the
   accumulator (a further launch past 64 ranges, accumulate = 1); 1 for the reference's own rounding. Two runs must give equal bits.
   r3m_clip_coef: coef = 1.0f exactly below max_norm; above, within one fp32 rounding (2^-24 relative, the double arithmetic before it is
   worth 2^-50) of min(1, max_norm / (norm + 1e-6)) formed in float64 from the same accumulator; norm likewise.

4., 5. Through the optimizers and the encoder against torch.optim.AdamW / Adam(weight_decay=) / SGD on float64 copies fed the same
   gradients, after torch.nn.utils.clip_grad_norm_ on those copies: the project's tolerances (tests/test_gpu_optim_steps.py: rtol 1e-6 and
   its atols). The gradients shrink tenfold per step, so step 1 clips and step 3 does not, and every element's gradient keeps the sign
   of its parameter, so no first moment is a difference of nearly equal terms (a relative tolerance means nothing there). In 5. the two
   encoder gradients are unrelated, so exp_avg after the second step is held to 4 u max(|g1|, |g2|) per element instead: 0.9 m1 + 0.1 g2
   carries 2 u S_m from each of the two steps, S_m <= max(|g1|, |g2|).

6. Under the data-parallel wrapper (a forced one-rank RCCL group, as tests/test_gpu_ddp.py runs one) with grad_scale = 0.5: the clipped
   step equals the plain step on gradients multiplied by 0.5 beforehand, and last_grad_norm is half the norm of the raw gradients.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from optim_cases import CASES, HYPER, N, SGD, SIZES, _dd, _ll, _state
from util import DEV, _st, rnd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
U64 = 2.0 ** -53
B1, B2, EPS = 0.9, 0.999, 1e-8


def f32(x):
    return float(np.float32(x))


# ---- 1. bit identity with the ranged steps ------------------------------------------------------------------------------------
def _inside(ranges):
    inside = torch.zeros(N, dtype=torch.bool, device=DEV)
    for off, cnt, _ in ranges:
        inside[off:off + cnt] = True
    return inside


@pytest.mark.parametrize("case", sorted(CASES))
def test_adam_groups_without_decay_and_coefficient_equal_adam_ranges(hip, case):
    ranges = CASES[case]
    off, cnt, step = ([r[k] for r in ranges] for k in range(3))
    n = len(ranges)
    p, g, m, v = _state(20)
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    assert hip.r3m_adam_step_ranges(pr.data_ptr(), g.data_ptr(), mr.data_ptr(), vr.data_ptr(), _ll(off), _ll(cnt), _ll(step), n, HYPER["lr"],
                                    HYPER["b1"], HYPER["b2"], HYPER["eps"], HYPER["gs"], _st()) == 0, hip.r3m_last_error()
    one = torch.ones(1, device=DEV)
    inside = _inside(ranges)
    for decoupled in (0, 1):
        for coef in (None, one.data_ptr()):
            pg, mg, vg = p0.clone(), m0.clone(), v0.clone()
            rc = hip.r3m_adam_step_groups(pg.data_ptr(), g.data_ptr(), mg.data_ptr(), vg.data_ptr(), _ll(off), _ll(cnt), _ll(step),
                                          _dd([HYPER["lr"]] * n), _dd([0.0] * n), n, HYPER["b1"], HYPER["b2"], HYPER["eps"], decoupled,
                                          HYPER["gs"], coef, _st())
            assert rc == 0, hip.r3m_last_error()
            torch.cuda.synchronize()
            what = f"{case} decoupled={decoupled} coef={'1.0f' if coef else 'NULL'}"
            for got, ref, before in ((pg, pr, p0), (mg, mr, m0), (vg, vr, v0)):
                assert torch.equal(got, ref), what
                assert torch.equal(got[~inside], before[~inside]), what
                assert not torch.equal(got[inside], before[inside]), what


@pytest.mark.parametrize("cfg", SGD, ids=["plain", "momentum", "damp+wd", "nesterov"])
@pytest.mark.parametrize("case", ["adjacent", "distinct_steps", "65_ranges", "ends_at_buffer_end", "empty_range_between"])
def test_sgd_groups_without_coefficient_equal_sgd_ranges(hip, case, cfg):
    """one learning rate and one weight decay (zero or not: r3m_sgd_step_ranges has a global one) in every range"""
    ranges = CASES[case]
    off, cnt, step = ([r[k] for r in ranges] for k in range(3))
    n = len(ranges)
    p, g, buf, _ = _state(30)
    p0, b0 = p.clone(), buf.clone()
    pr, br = p.clone(), buf.clone()
    lr, gs = 1e-2, 0.5
    bp = lambda t: t.data_ptr() if cfg["momentum"] else None
    assert hip.r3m_sgd_step_ranges(pr.data_ptr(), g.data_ptr(), bp(br), _ll(off), _ll(cnt), _ll(step), n, lr, cfg["momentum"], cfg["damp"],
                                   cfg["wd"], cfg["nesterov"], gs, _st()) == 0, hip.r3m_last_error()
    one = torch.ones(1, device=DEV)
    inside = _inside(ranges)
    for coef in (None, one.data_ptr()):
        pg, bg = p0.clone(), b0.clone()
        rc = hip.r3m_sgd_step_groups(pg.data_ptr(), g.data_ptr(), bp(bg), _ll(off), _ll(cnt), _ll(step), _dd([lr] * n), _dd([cfg["wd"]] * n), n,
                                     cfg["momentum"], cfg["damp"], cfg["nesterov"], gs, coef, _st())
        assert rc == 0, hip.r3m_last_error()
        torch.cuda.synchronize()
        assert torch.equal(pg, pr) and torch.equal(bg, br), (case, coef)
        assert torch.equal(pg[~inside], p0[~inside]) and torch.equal(bg[~inside], b0[~inside])
        assert not torch.equal(pg[inside], p0[inside])


# ---- 2. one grouped Adam step against float64 -----------------------------------------------------------------------------------
GAP = 8
R_SIZES = [SIZES[0], SIZES[2], SIZES[1]]                 # one f32x4 group; the capped grid's ragged second trip; one block plus one group
R_OFFS = [0, SIZES[0] + GAP, SIZES[0] + GAP + SIZES[2] + GAP]
N2 = R_OFFS[2] + SIZES[1] + GAP
R_LR = [1e-5, 1e-3, 1e-4]
R_WD = [0.0, 1e-2, 0.3]


@functools.lru_cache(maxsize=None)
def state(n):
    """the state of tests/test_gpu_optim_steps.py: gradients +-10^uniform(-6, 2), moments of matching size, every 7th element with
    g = m = v = 0"""
    sign = lambda seed: torch.where(rnd((n,), seed) > 0, 1.0, -1.0)
    p = rnd((n,), 501)
    g = sign(502) * 10.0 ** rnd((n,), 503, -6.0, 2.0)
    m = sign(504) * 10.0 ** rnd((n,), 505, -6.0, 2.0)
    v = (m.abs() * rnd((n,), 506, 0.5, 2.0)) ** 2
    dead = torch.arange(n) % 7 == 3
    for t in (g, m, v):
        t[dead] = 0.0
    assert bool((p != 0).all()) and bool(((v > 0) | dead).all()) and bool(dead.any())
    assert float(g.abs().max()) > 50 and float(g[~dead].abs().min()) < 1e-5
    return p, g, m, v, dead


@functools.lru_cache(maxsize=1)
def state64(n):
    return tuple(t.double().numpy() for t in state(n)[:4])


def adam_group_reference(p64, g64, m64, v64, lr, wd, step, scale, coef, decoupled):
    """float64 results and bounds of ONE range (module docstring), with the launcher's fp32 scalars (csrc/adam.hip launch_adam)"""
    a, beta2, c, eps = f32(1.0 - B1), f32(B2), f32(1.0 - B2), f32(EPS)
    neg_step = f32(-(lr / (1.0 - math.pow(B1, float(step)))))
    bc2s = f32(math.sqrt(1.0 - math.pow(B2, float(step))))
    gr = g64 * f32(scale)
    E_g = U * np.abs(gr)
    if coef is not None:
        gr = gr * f32(coef)
        E_g = 2 * U * np.abs(gr)
    p1, E_p = p64, 0.0
    if wd != 0 and not decoupled:
        w = f32(wd)
        E_g = E_g + U * np.abs(w * p64)
        gr = gr + w * p64
        E_g = E_g + U * np.abs(gr)
    elif wd != 0:
        p1 = p64 * f32(1.0 - lr * wd)
        E_p = U * np.abs(p1)
    m_ref = m64 + (gr - m64) * a
    v_ref = v64 * beta2 + (c * gr) * gr
    denom = np.sqrt(v_ref) / bc2s + eps
    upd = (neg_step * m_ref) / denom
    p_ref = p1 + upd
    S_m, S_v = np.maximum(np.abs(m64), np.abs(gr)), np.maximum(v64, gr * gr)
    b_m = a * E_g + 1.9 * U * S_m
    b_v = c * (2 * np.abs(gr) * E_g + E_g * E_g) + (2 * c + 2.5) * U * S_v
    r_v = np.where(v_ref > 0, b_v / np.maximum(v_ref, 1e-300), 0.0)
    assert float(r_v.max()) < 2.0 ** -10, f"input condition: exp_avg_sq known to {float(r_v.max()):.2e} relative only"
    r_d = r_v / 2 + 3 * U
    b_u = abs(neg_step) / denom * b_m + (2 * U + r_d) * np.abs(upd)
    b_p = U * np.abs(p_ref) + E_p + b_u
    k = 1.0 + 2.0 ** -9
    return (m_ref, v_ref, p_ref), (k * b_m, k * b_v, k * b_p)


def check(what, got, ref, bound):
    """|got - ref| <= bound elementwise; the worst ratio is printed before it is asserted"""
    got = got.cpu().double().numpy()
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    ratio = np.abs(got - ref) / np.maximum(bound, 1e-300)
    i = int(ratio.argmax())
    print(f"{what}: worst error / bound {float(ratio[i]):.3f} (bound in units of 2^-24 of the scale: see the module docstring)", flush=True)
    assert ratio[i] <= 1.0, f"{what}: element {i} of {got.size}: got {got[i]!r}, float64 {ref[i]!r}, bound {bound[i]:.3e}"


@pytest.mark.parametrize("coef", [None, 0.37], ids=["nocoef", "coef0.37"])
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("decoupled", [0, 1], ids=["l2", "decoupled"])
def test_adam_groups_single_step_against_float64(hip, decoupled, step, scale, coef):
    """three ranges of 4, 4 194 316 and 1028 elements with learning rates 1e-5, 1e-3, 1e-4 and weight decays 0, 1e-2, 0.3, eight
    untouched elements between and behind them"""
    p, g, m, v, dead = state(N2)
    p64, g64, m64, v64 = state64(N2)
    steps = [step, step, step + 1]
    pd, gd, md, vd = (t.to(DEV) for t in (p, g, m, v))
    cd = None if coef is None else torch.tensor([coef], dtype=torch.float32, device=DEV)
    rc = hip.r3m_adam_step_groups(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), _ll(R_OFFS), _ll(R_SIZES), _ll(steps), _dd(R_LR),
                                  _dd(R_WD), 3, B1, B2, EPS, decoupled, scale, None if cd is None else cd.data_ptr(), _st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gd.cpu(), g)
    inside = torch.zeros(N2, dtype=torch.bool)
    for r in range(3):
        sl = slice(R_OFFS[r], R_OFFS[r] + R_SIZES[r])
        inside[sl] = True
        refs, bounds = adam_group_reference(p64[sl], g64[sl], m64[sl], v64[sl], R_LR[r], R_WD[r], steps[r], scale, coef, decoupled)
        what = f"adam groups {'decoupled' if decoupled else 'l2'} step={steps[r]} grad_scale={scale:g} coef={coef} range {r} (lr {R_LR[r]:g} wd {R_WD[r]:g})"
        for name, got, ref, bound in zip(("exp_avg", "exp_avg_sq", "params"), (md, vd, pd), refs, bounds):
            check(f"{what} {name}", got[sl], ref, bound)
        moved = float((pd[sl].cpu() != p[sl])[~dead[sl]].double().mean())
        assert R_SIZES[r] < 1000 or moved > 0.9, f"{what}: only {moved:.2f} of the live elements moved"
        if R_WD[r] == 0:                                  # g = m = v = 0 and no decay: nothing to add
            d = dead[sl]
            assert torch.equal(pd[sl].cpu()[d], p[sl][d]) and not md[sl].cpu()[d].any() and not vd[sl].cpu()[d].any()
    for got, before in ((pd, p), (md, m), (vd, v)):
        assert torch.equal(got.cpu()[~inside], before[~inside]) and int((~inside).sum()) == 3 * GAP


# ---- 3. the squared norm and the clip coefficient -------------------------------------------------------------------------------
def _depth(ranges, accumulate):
    """roundings a term of the sum passes through (module docstring), over the launches of up to 64 non-empty ranges"""
    live = [(o, c) for o, c in ranges if c]
    worst, adds = 0, 1 if accumulate else 0
    for k in range(0, len(live), 64):
        grid, lane = 0, 0
        for _, c in live[k:k + 64]:
            n4 = c // 4
            blocks = min((n4 + 255) // 256, 4096)
            grid += blocks
            lane = max(lane, 4 * ((n4 + blocks * 256 - 1) // (blocks * 256)))
        worst = max(worst, lane + 9 + (grid + 255) // 256 + 9)
        adds += 1 if k else 0
    return worst + adds + 1


def _sqnorm(hip, g, ranges, acc, accumulate, ws):
    off, cnt = [r[0] for r in ranges], [r[1] for r in ranges]
    rc = hip.r3m_grad_sqnorm_ranges(g.data_ptr(), _ll(off), _ll(cnt), len(ranges), acc.data_ptr(), accumulate, ws.data_ptr(), ws.numel(), _st())
    assert rc == 0, hip.r3m_last_error()


def _fsum_sq(g, ranges):
    return math.fsum(x for o, c in ranges for x in (g[o:o + c].double() ** 2).tolist())


@pytest.fixture(scope="module")
def sq_ws(hip):
    return torch.empty(hip.r3m_grad_sqnorm_workspace_bytes(), dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("n", SIZES)
def test_sqnorm_against_fsum(hip, sq_ws, n):
    g = state(max(n, 1028))[1][:n].clone()
    gd = g.to(DEV)
    ranges = [(0, n)]
    ref = _fsum_sq(g, ranges)
    acc = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    _sqnorm(hip, gd, ranges, acc, 0, sq_ws)
    first = acc.clone()
    d = _depth(ranges, False)
    err = abs(float(first) - ref) / ref
    print(f"sqnorm n={n}: relative error {err:.3e}, bound {d} x 2^-53 = {d * U64:.3e}", flush=True)
    assert err <= d * U64
    acc.fill_(float("nan"))
    _sqnorm(hip, gd, ranges, acc, 0, sq_ws)
    assert torch.equal(acc.view(torch.int64), first.view(torch.int64)), "two runs over the same gradients differ in their bits"


def test_sqnorm_65_ranges_accumulate_and_no_ranges(hip, sq_ws):
    g1, g2 = state(N2)[1][:N].clone(), state(N2)[1][N:2 * N].clone()
    d1, d2 = g1.to(DEV), g2.to(DEV)
    r65 = [(o, c) for o, c, _ in CASES["65_ranges"]]
    acc = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    _sqnorm(hip, d1, r65, acc, 0, sq_ws)                                   # two launches: the second adds to the first
    ref = _fsum_sq(g1, r65)
    d = _depth(r65, False)
    err = abs(float(acc) - ref) / ref
    print(f"sqnorm 65 ranges: relative error {err:.3e}, bound {d} x 2^-53", flush=True)
    assert err <= d * U64
    # chained over two buffers: the first call writes, the second adds; elements outside the ranges do not count
    r2 = [(o, c) for o, c, _ in CASES["distinct_steps"]]
    _sqnorm(hip, d2, r2, acc, 1, sq_ws)
    ref2 = _fsum_sq(g1, r65) + _fsum_sq(g2, r2)
    d = max(_depth(r65, False), _depth(r2, True)) + 1
    err = abs(float(acc) - ref2) / ref2
    print(f"sqnorm chained: relative error {err:.3e}, bound {d} x 2^-53", flush=True)
    assert err <= d * U64
    bits = acc.clone()
    _sqnorm(hip, d1, r65, acc, 0, sq_ws)
    _sqnorm(hip, d2, r2, acc, 1, sq_ws)
    assert torch.equal(acc.view(torch.int64), bits.view(torch.int64))
    # no ranges (or only empty ones): accumulate leaves the accumulator alone, otherwise it becomes 0
    for none in ([], [(8, 0), (16, 0)]):
        acc.fill_(3.5)
        _sqnorm(hip, d1, none, acc, 1, sq_ws)
        assert float(acc) == 3.5
        _sqnorm(hip, d1, none, acc, 0, sq_ws)
        assert float(acc) == 0.0


def test_clip_coef(hip):
    sq = torch.zeros(1, dtype=torch.float64, device=DEV)
    out = torch.full((2,), float("nan"), device=DEV)

    def run(sqnorm, max_norm, scale):
        sq.fill_(sqnorm)
        out.fill_(float("nan"))
        assert hip.r3m_clip_coef(sq.data_ptr(), max_norm, scale, out.data_ptr(), _st()) == 0, hip.r3m_last_error()
        coef, norm = (float(x) for x in out.cpu())
        n64 = f32(scale) * math.sqrt(sqnorm)
        c64 = min(1.0, max_norm / (n64 + 1e-6))
        assert abs(norm - n64) <= U * n64 * (1 + 2.0 ** -20), (norm, n64)
        assert abs(coef - c64) <= U * c64 * (1 + 2.0 ** -20), (coef, c64)
        return coef, norm

    assert run(9.0, 5.0, 1.0) == (1.0, 3.0)                               # below max_norm: exactly 1
    assert run(0.0, 1.0, 1.0) == (1.0, 0.0)                               # a zero gradient
    coef, norm = run(123.456, 2.5, 1.0)
    assert coef < 1.0
    for scale in (0.125, 3.0):                                             # the norm is that of the scaled gradient
        c, n = run(123.456, 2.5, scale)
        assert abs(n - scale * math.sqrt(123.456)) <= U * n * (1 + 2.0 ** -20)
        assert (c == 1.0) == (scale * math.sqrt(123.456) + 1e-6 <= 2.5)
    sq.fill_(float("inf"))                                                 # error_if_nonfinite=False: the arithmetic takes its course
    assert hip.r3m_clip_coef(sq.data_ptr(), 1.0, 1.0, out.data_ptr(), _st()) == 0
    assert out.cpu().tolist() == [0.0, float("inf")]
    sq.fill_(float("nan"))
    assert hip.r3m_clip_coef(sq.data_ptr(), 1.0, 1.0, out.data_ptr(), _st()) == 0
    assert bool(torch.isnan(out).all())


# ---- 4. through the optimizers ---------------------------------------------------------------------------------------------------
class _Ranged(torch.nn.Module):
    """an owner with param_ranges(): 2-D and 1-D tensors, views into one flat GPU buffer"""
    SHAPES = [(64, 33 * 4), (132,), (40, 100), (100,), (260,)]

    def __init__(self, seed):
        super().__init__()
        sizes = [math.prod(s) for s in self.SHAPES]
        self.flat = rnd((sum(sizes),), seed).to(DEV)
        self.g = torch.zeros_like(self.flat)
        self._ranges, off = [], 0
        for k, (s, n) in enumerate(zip(self.SHAPES, sizes)):
            self.register_parameter(f"t{k}", torch.nn.Parameter(self.flat[off:off + n].view(s)))
            self._ranges.append((off, n))
            off += n
        self.written = [True] * len(sizes)

    def flat_params(self):
        return self.flat

    def flat_grads(self):
        return self.g

    def mark_grads_stale(self):
        pass

    def param_ranges(self):
        return self._ranges

    def grads_written(self):
        return self.written


class _Flat(torch.nn.Module):
    """an owner without param_ranges() (tests/test_gpu_optim_steps.py)"""

    def __init__(self, n, seed):
        super().__init__()
        self.p = torch.nn.Parameter(rnd((n,), seed).to(DEV))
        self.g = torch.zeros(n, device=DEV)

    def flat_params(self):
        return self.p.data

    def flat_grads(self):
        return self.g

    def mark_grads_stale(self):
        pass

    def has_grads(self):
        return True


@pytest.mark.parametrize("kind", ["adamw", "adam_l2", "sgd"])
def test_two_owners_two_groups_clipping_scheduler_and_snapshot_match_torch(hip, kind):
    from r3m_amd.optim import FusedAdam, FusedAdamW, FusedSGD
    A, B = _Ranged(81), _Flat(1028, 82)
    fused_params = list(A.parameters()) + list(B.parameters())
    ref_params = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in fused_params]
    pick = lambda ps: ([ps[0], ps[2]], [ps[1], ps[3], ps[4], ps[5]])       # the 2-D tensors of A | its 1-D tensors and all of B
    hyper = [dict(lr=1e-4, weight_decay=1e-2), dict(lr=3e-5, weight_decay=0.0)]
    groups = lambda ps: [dict(params=sel, **h) for sel, h in zip(pick(ps), hyper)]
    # every element keeps the sign of its parameter and shrinks tenfold per step (module docstring)
    sign = torch.cat([p.detach().reshape(-1) for p in fused_params]).cpu().sign()
    grads = [sign * rnd((A.flat.numel() + 1028,), 90 + i, 0.0, 1.0) * (10.0 ** -i) for i in range(3)]
    max_norm = 0.5 * float(grads[0].double().norm())
    if kind == "adamw":
        make = lambda: FusedAdamW([A, B], lr=1e-3, max_grad_norm=max_norm, param_groups=groups(fused_params))
        ref = torch.optim.AdamW(groups(ref_params), lr=1e-3)
    elif kind == "adam_l2":
        make = lambda: FusedAdam([A, B], lr=1e-3, max_grad_norm=max_norm, param_groups=groups(fused_params))
        ref = torch.optim.Adam(groups(ref_params), lr=1e-3)
    else:
        make = lambda: FusedSGD([A, B], lr=1e-3, momentum=0.9, max_grad_norm=max_norm, param_groups=groups(fused_params))
        ref = torch.optim.SGD(groups(ref_params), lr=1e-3, momentum=0.9)
    opt = make()
    assert len(opt.param_groups) == 2 and opt.last_grad_norm is None
    lambdas = [lambda e: 0.5 ** e, lambda e: 1.0 / (1 + e)]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambdas)
    ref_sched = torch.optim.lr_scheduler.LambdaLR(ref, lambdas)
    nA = A.flat.numel()
    state_cat = lambda key: torch.cat([ref.state[p][key].reshape(-1) for p in ref_params])

    def compare(o, what):
        for k, (pf, pr) in enumerate(zip(fused_params, ref_params)):
            torch.testing.assert_close(pf.detach().cpu().double(), pr.detach(), rtol=1e-6, atol=1e-9, msg=lambda s: f"{what}: tensor {k}: {s}")
        if kind == "sgd":
            rb = state_cat("momentum_buffer")
            got = torch.cat([o._buf[0], o._buf[1]]).cpu().double()
            torch.testing.assert_close(got, rb, rtol=1e-6, atol=2e-7 * float(rb.abs().max()), msg=lambda s: f"{what}: momentum: {s}")
        else:
            torch.testing.assert_close(torch.cat([o._m[0], o._m[1]]).cpu().double(), state_cat("exp_avg"), rtol=1e-6, atol=1e-12,
                                       msg=lambda s: f"{what}: exp_avg: {s}")
            torch.testing.assert_close(torch.cat([o._v[0], o._v[1]]).cpu().double(), state_cat("exp_avg_sq"), rtol=1e-6, atol=1e-14,
                                       msg=lambda s: f"{what}: exp_avg_sq: {s}")

    norms = []
    for it, g in enumerate(grads):
        off = 0
        for pr in ref_params:
            pr.grad = g[off:off + pr.numel()].double().view(pr.shape).clone()
            off += pr.numel()
        norms.append(float(torch.nn.utils.clip_grad_norm_(ref_params, max_norm)))
        ref.step()
        A.g.copy_(g[:nA].to(DEV))
        B.g.copy_(g[nA:].to(DEV))
        opt.step()
        compare(opt, f"{kind} step {it + 1}")
        assert abs(float(opt.last_grad_norm) - norms[-1]) <= 4 * U * norms[-1]      # fp32 store of an fp64 norm
        if it < 2:
            sched.step()
            ref_sched.step()
            assert [g_["lr"] for g_ in opt.param_groups] == [g_["lr"] for g_ in ref.param_groups]
        if it == 1:                                         # a snapshot mid-run, into a fresh optimizer that takes the third step
            sd = opt.state_dict()
            opt = make()
            opt.load_state_dict(sd)
            assert [g_["lr"] for g_ in opt.param_groups] == [g_["lr"] for g_ in ref.param_groups]
    assert norms[0] > max_norm and norms[2] < max_norm, f"step 1 must clip and step 3 must not: norms {norms}, max_norm {max_norm}"
    assert [g_["lr"] for g_ in opt.param_groups] == [1e-4 * 0.5 ** 2, 3e-5 * (1.0 / 3)]           # both groups followed their own schedule


# ---- 5. through the encoder -----------------------------------------------------------------------------------------------------
def test_encoder_groups_match_torch_adamw_with_frozen_layer1(hip):
    """HipResNet(18), 2 frames of 32 x 32, loss = h.sum(); FusedAdamW over no_decay_groups(layerwise_lr_groups(...)); layer1 frozen for
    the first step (its tensors keep bits and moments), trainable for the second (it steps with count 1 next to tensors at count 2)"""
    from r3m_amd.encoder import HipResNet
    from r3m_amd.optim import FusedAdamW, layerwise_lr_groups, no_decay_groups
    torch.manual_seed(5)
    net = HipResNet(18).to(DEV)
    net.train()
    named = dict(net.named_parameters())
    name_of = {id(p): n for n, p in named.items()}
    groups = no_decay_groups(layerwise_lr_groups(net, 1e-4, 0.5), 0.05)
    opt = FusedAdamW([net], lr=1e-4, param_groups=groups)
    assert len(opt.param_groups) == 10
    ref_p = {n: torch.nn.Parameter(p.detach().cpu().double().clone()) for n, p in named.items()}
    ref = torch.optim.AdamW([dict(params=[ref_p[name_of[id(p)]] for p in g["params"]], lr=g["lr"], weight_decay=g["weight_decay"])
                             for g in opt.param_groups], lr=1e-4)
    layer1 = [n for n in named if n.startswith("layer1.")]
    for n in layer1:
        named[n].requires_grad_(False)
    before = {n: named[n].detach().clone() for n in layer1}
    gen = torch.Generator().manual_seed(7)
    seen = {}
    for it in range(2):
        x = (torch.rand(2, 3, 32, 32, generator=gen) * 255).to(DEV)
        opt.zero_grad()
        net(x).sum().backward()
        torch.cuda.synchronize()
        net.flat_grads()
        for n, p in named.items():
            frozen = it == 0 and n in layer1
            assert (p.grad is None) == frozen, n
            ref_p[n].grad = None if p.grad is None else p.grad.detach().cpu().double().clone()
            if p.grad is not None:
                seen[n] = torch.maximum(seen[n], ref_p[n].grad.abs()) if n in seen else ref_p[n].grad.abs()
        ref.step()
        opt.step()
        torch.cuda.synchronize()
        for n, p in named.items():
            mom = opt.moments(p)
            if it == 0 and n in layer1:
                assert torch.equal(p.detach(), before[n]) and not mom[0].any() and not mom[1].any(), f"frozen {n} or its moments moved"
                continue
            what = f"step {it + 1} {n}"
            torch.testing.assert_close(p.detach().cpu().double(), ref_p[n].detach(), rtol=1e-6, atol=1e-9, msg=lambda s: f"{what}: {s}")
            st = ref.state[ref_p[n]]
            err = (mom[0].cpu().double() - st["exp_avg"]).abs()
            assert bool((err <= 4 * U * seen[n] + 1e-30).all()), f"{what}: exp_avg off by {float(err.max()):.3e}"
            torch.testing.assert_close(mom[1].cpu().double(), st["exp_avg_sq"], rtol=1e-6, atol=1e-14, msg=lambda s: f"{what}: exp_avg_sq: {s}")
        if it == 0:
            for n in layer1:
                named[n].requires_grad_(True)
    steps = opt.tensor_steps(0)
    assert steps is not None and set(steps) == {1, 2}
    assert [int(ref.state[ref_p[n]]["step"]) for n in named] == steps


# ---- 6. under the data-parallel wrapper -----------------------------------------------------------------------------------------
def _wrapper_worker(port, q):
    import torch.distributed as dist
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from oracle import detgen
        from r3m_amd import R3M
        from r3m_amd.parallel import DistributedR3M, SingleDevice, make_network_wrapper
        from r3m_amd.trainer import Trainer
        CLIP = 1e-3

        def build():
            m = R3M("cuda", 1e-4, 1024, size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=1.0, weight_decay=0.05, grad_clip=CLIP)
            shapes = [(k, tuple(v.shape)) for k, v in m.convnet.state_dict().items()]
            m.convnet.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes).items()})
            torch.manual_seed(11)
            m.lang_rew.reset_parameters()
            return m.to("cuda:0")

        B = 4
        frames = torch.from_numpy(detgen.frames("nccl1", (B, 5, 3, 224, 224))).to("cuda:0")
        feats = torch.from_numpy(detgen.uniform("langfeat", (B, 768), -0.6, 0.6)).to("cuda:0")
        out = {}
        for name in ("wrapped", "plain"):
            m = build()
            opt = m.encoder_opt
            assert opt.max_grad_norm == CLIP and len(opt.param_groups) == 3 and opt.param_groups[0]["decoupled_weight_decay"]
            if name == "wrapped":
                net = make_network_wrapper(m, force=True)
                assert isinstance(net, DistributedR3M) and net.sync.active
                opt.grad_scale = 0.5
            else:                                           # the same step on gradients multiplied by 0.5 beforehand
                net = SingleDevice(m)
                fused_step = opt.step

                def step():
                    for o in opt.owners:
                        o.flat_grads().mul_(0.5)
                    return fused_step()
                opt.step = step
            start = (m.convnet.flat_params().clone(), m.lang_rew.flat_params().clone())
            torch.manual_seed(5)
            Trainer(1).update(net, (frames, (feats, torch.ones(B))), 0)
            torch.cuda.synchronize()
            out[name] = (m.convnet.flat_params().clone(), m.lang_rew.flat_params().clone(), float(opt.last_grad_norm),
                         m.convnet.flat_grads().clone(), m.lang_rew.flat_grads().clone())
        w, p = out["wrapped"], out["plain"]
        raw = math.sqrt(float((w[3].double() ** 2).sum() + (w[4].double() ** 2).sum()))
        assert torch.equal(w[3] * 0.5, p[3]) and torch.equal(w[4] * 0.5, p[4])           # same backward, then the hand-made halving
        assert abs(w[2] - 0.5 * raw) <= 2.0 ** -23 * 0.5 * raw, (w[2], raw)
        assert w[2] > CLIP, "the step must clip"
        assert abs(p[2] - w[2]) <= 2.0 ** -23 * w[2]
        for a, b, what in ((w[0], p[0], "encoder"), (w[1], p[1], "language head")):
            torch.testing.assert_close(a, b, rtol=2.0 ** -23, atol=0.0, msg=lambda s: f"{what}: {s}")
        assert not torch.equal(start[0], w[0]) and not torch.equal(start[1], w[1])      # both owners stepped
        q.put("ok")
    except Exception:  # noqa: BLE001
        import traceback
        q.put("FAIL: " + traceback.format_exc())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_clipped_step_under_the_wrapper_uses_the_scaled_gradient(hip):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_wrapper_worker, args=(port, q))
    proc.start()
    import queue
    while True:
        try:
            res = q.get(timeout=5)
            break
        except queue.Empty:
            if not proc.is_alive():
                res = f"the worker ended with exit code {proc.exitcode} and no result"
                break
    proc.join(timeout=120)
    assert res == "ok", res
