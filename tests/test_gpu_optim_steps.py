"""-m gpu: ONE step of r3m_adam_step / r3m_sgd_step (csrc/adam.hip) from a random non-zero fp32 state against float64 on the CPU, at the
sizes where the launch changes shape and with the scalars the other optimizer tests never pass:

  * the whole-buffer calls: n = 4 (one f32x4 group), 1028 (one block plus one group), 4 x (4096 x 256) + 12 = 4 194 316 (opt_grid caps
    the grid at 4096 blocks: the grid-stride loop takes a second, ragged trip -- three groups). No other operator test passes 4 194 304;
  * grad_scale = 0.125 and 3.0 (never anything but 1.0 elsewhere), at the C ABI and through FusedAdam / FusedSGD;
  * step = 1, 2, 1000, 10^6 (bias corrections from 0.1 / 0.001 to 1).

A single step, so no error accumulates: the bounds below are derived from the count of fp32 roundings in adam_span_t / sgd_span_t, in units
of u = 2^-24 (the relative error of one correctly rounded fp32 operation; the library is built without fast-math, so `/` and sqrtf are
correctly rounded) of the quantity's own scale. The float64 reference uses the very fp32 scalars the launcher passes (the `(float)` casts
and adam_bias_corrections are restated here). A fused multiply-add only removes roundings. None is looser than 16 u.

Adam, per element, gr = g * grad_scale (error u |gr|):
  m' = m + (gr - m) * a, a = (float)(1 - beta1) ~ 0.1: the error of gr arrives as a u |gr|; the subtraction, the product and the sum add
       a u |gr - m|, u |a (gr - m)| and u |m'|: together <= u (0.1 + 0.4 + 1) S_m with S_m = max(|m|, |gr|) >= |m'|.        BOUND 2 u S_m
  v' = v * beta2 + (c * gr) * gr, c = (float)(1 - beta2) ~ 0.001: gr^2 carries 2 u, the two products 2 u more (4 u c gr^2), v * beta2 one
       (u beta2 v), the sum u v': <= u (0.004 + 1 + 1) S_v with S_v = max(v, gr^2) >= v'.                                    BOUND 3 u S_v
       Relative to v' itself (both summands are non-negative and <= v'): 4 u + u + u = 6 u.
  denom = sqrtf(v') / bc2_sqrt + eps: 3 u from v', u for the root, u for the quotient, u for the sum: 6 u relative.
  U = (neg_step * m') / denom: the error of m' arrives as |neg_step| / denom * 2 u S_m; the product, the quotient and denom add
       (1 + 1 + 6) u |U|.                                                                         BOUND |neg_step| / denom * 2 u S_m + 8 u |U|
  p' = p + U: one more rounding.                                                                            BOUND u |p'| + the bound on U

SGD, per element, gr = g * grad_scale [+ wd * p]: u |g s|, then u |wd p| and u |gr| <= 2 u S_g with S_g = |g s| + |wd p|.      BOUND 2 u S_g
  buf' = gr on the first step (BOUND 2 u S_g), else buf * mu + (1 - damp) * gr: u |mu buf|, (1 - damp)(2 u S_g + u S_g), u |buf'|
       <= 4 u S_b with S_b = |mu buf| + (1 - damp) S_g.                                                                      BOUND 4 u S_b
  d = buf' (4 u S_b), or gr without momentum (2 u S_g), or gr + mu * buf' with Nesterov: 2 u S_g + mu (4 u S_b + u S_b) + u |d|
       <= 6 u S_d with S_d = S_g + mu S_b.                                                                                   BOUND 6 u S_d
  p' = p - lr * d: the product adds u |lr d|.                                                    BOUND u |p'| + lr (bound on d + u S_d) <= 7 u lr S_d
"""
import functools
import math

import numpy as np
import pytest
import torch

from optim_cases import SGD_CFGS, SGD_IDS, SIZES
from util import DEV, _st, rnd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
STEPS = [1, 2, 1000, 10 ** 6]
SCALES = [1.0, 0.125, 3.0]
LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-8
SGD_LR = 1e-2


def f32(x):
    """the (float) cast of a double scalar, as a python float"""
    return float(np.float32(x))


@functools.lru_cache(maxsize=None)
def state(n):
    """CPU fp32 p, g, m, v / momentum buffer: gradients +-10^uniform(-6, 2), moments of matching size (v = (|m| x uniform(0.5, 2))^2, so the
    step stays a step), every 7th element with g = m = v = buf = 0"""
    sign = lambda seed: torch.where(rnd((n,), seed) > 0, 1.0, -1.0)
    p = rnd((n,), 501)
    g = sign(502) * 10.0 ** rnd((n,), 503, -6.0, 2.0)
    m = sign(504) * 10.0 ** rnd((n,), 505, -6.0, 2.0)
    v = (m.abs() * rnd((n,), 506, 0.5, 2.0)) ** 2
    buf = sign(507) * 10.0 ** rnd((n,), 508, -6.0, 2.0)
    dead = torch.arange(n) % 7 == 3
    for t in (g, m, v, buf):
        t[dead] = 0.0
    assert bool((p != 0).all()) and bool(((v > 0) | dead).all()) and bool(dead.any())
    assert n < 1000 or (float(g.abs().max()) > 50 and float(g[~dead].abs().min()) < 1e-5)          # the gradients span 1e-6 ... 1e2
    return p, g, m, v, buf, dead


@functools.lru_cache(maxsize=2)
def state64(n):
    return tuple(t.double().numpy() for t in state(n)[:5])


def check(what, got, ref, bound):
    """|got - ref| <= bound elementwise; the worst ratio is printed before it is asserted"""
    got = got.cpu().double().numpy()
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: worst error / bound {ratio:.3f} (bound in units of 2^-24 of the scale: see the module docstring)", flush=True)
    i = int((err / np.maximum(bound, 1e-300)).argmax())
    assert ratio <= 1.0, f"{what}: element {i} of {got.size}: got {got[i]!r}, float64 {ref[i]!r}, bound {bound[i]:.3e}"


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_adam_single_step_against_float64(hip, n, step, scale):
    """r3m_adam_step, one step: m', v', p' within the derived bounds; elements with g = m = v = 0 keep p bit for bit and m' = v' = 0.
    Paths first reached here: r3m_adam_step's grid-stride loop (n = 4 194 316: 1 048 579 groups over 4096 x 256 threads, a second trip of
    three groups) and grad_scale != 1."""
    p, g, m, v, _, dead = state(n)
    p64, g64, m64, v64, _ = state64(n)
    # the launcher's scalars (csrc/adam.hip launch_adam, adam_bias_corrections)
    a, beta2, c, eps = f32(1.0 - B1), f32(B2), f32(1.0 - B2), f32(EPS)
    neg_step = f32(-(LR / (1.0 - math.pow(B1, float(step)))))
    bc2s = f32(math.sqrt(1.0 - math.pow(B2, float(step))))
    s = f32(scale)
    gr = g64 * s
    m_ref = m64 + (gr - m64) * a
    v_ref = v64 * beta2 + (c * gr) * gr
    denom = np.sqrt(v_ref) / bc2s + eps
    upd = (neg_step * m_ref) / denom
    p_ref = p64 + upd
    S_m, S_v = np.maximum(np.abs(m64), np.abs(gr)), np.maximum(v64, gr * gr)
    b_m, b_v = 2 * U * S_m, 3 * U * S_v
    b_u = abs(neg_step) / denom * 2 * U * S_m + 8 * U * np.abs(upd)
    b_p = U * np.abs(p_ref) + b_u

    pd, gd, md, vd = (t.to(DEV) for t in (p, g, m, v))
    rc = hip.r3m_adam_step(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, LR, B1, B2, EPS, step, scale, _st())
    assert rc == 0, hip.r3m_last_error()
    what = f"adam n={n} step={step} grad_scale={scale:g}"
    check(what + " exp_avg", md, m_ref, b_m)
    check(what + " exp_avg_sq", vd, v_ref, b_v)
    check(what + " params", pd, p_ref, b_p)
    assert torch.equal(gd.cpu(), g)
    dd = dead.to(DEV)
    assert torch.equal(pd[dd].cpu(), p[dead]) and bool((md[dd] == 0).all()) and bool((vd[dd] == 0).all())
    moved = float((pd.cpu() != p)[~dead].double().mean())
    assert n < 1000 or moved > 0.9, f"{what}: only {moved:.2f} of the live elements moved"


@pytest.mark.parametrize("cfg", SGD_CFGS, ids=SGD_IDS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_sgd_single_step_against_float64(hip, n, step, scale, cfg):
    """r3m_sgd_step, one step in the four configurations of test_sgd_matches_torch: buf' and p' within the derived bounds. Step 1 gets a
    NaN-filled momentum buffer, which must be initialised and not read. Without weight decay, elements with g = buf = 0 keep p bit for
    bit. Paths first reached here: r3m_sgd_step's grid-stride loop (n = 4 194 316) and grad_scale != 1 (dropping it from sgd_span_t fails
    every case with scale 0.125 or 3)."""
    p, g, _, _, buf, dead = state(n)
    p64, g64, _, _, buf64 = state64(n)
    mom, damp, wd, nest = cfg.get("momentum", 0.0), cfg.get("dampening", 0.0), cfg.get("weight_decay", 0.0), bool(cfg.get("nesterov"))
    lr, mu, omd, wdf, s = f32(SGD_LR), f32(mom), f32(1.0 - damp), f32(wd), f32(scale)
    first = step == 1
    gs = g64 * s
    gr = gs + wdf * p64 if wd else gs
    S_g = np.abs(gs) + np.abs(wdf * p64)
    if mom:
        b_ref = gr if first else buf64 * mu + omd * gr
        S_b = S_g if first else np.abs(mu * buf64) + omd * S_g
        bound_b = (2 if first else 4) * U * S_b
        if nest:
            d, S_d = gr + mu * b_ref, S_g + mu * S_b
            bound_d = 6 * U * S_d
        else:
            d, S_d, bound_d = b_ref, S_b, bound_b
    else:
        d, S_d, bound_d = gr, S_g, 2 * U * S_g
    p_ref = p64 - lr * d
    bound_p = U * np.abs(p_ref) + lr * (bound_d + U * S_d)

    pd, gd = p.to(DEV), g.to(DEV)
    bd = (torch.full((n,), float("nan"), device=DEV) if first else buf.to(DEV)) if mom else None
    rc = hip.r3m_sgd_step(pd.data_ptr(), gd.data_ptr(), None if bd is None else bd.data_ptr(), n, SGD_LR, mom, damp, wd, 1 if nest else 0, step,
                          scale, _st())
    assert rc == 0, hip.r3m_last_error()
    what = f"sgd[{SGD_IDS[SGD_CFGS.index(cfg)]}] n={n} step={step} grad_scale={scale:g}"
    if mom:
        check(what + " momentum buffer", bd, b_ref, bound_b)
    check(what + " params", pd, p_ref, bound_p)
    if not wd:
        assert torch.equal(pd.cpu()[dead], p[dead])      # g = 0 and buf = 0 there: nothing to add
    moved = float((pd.cpu() != p)[~dead].double().mean())    # lr |d| under half an ulp of p leaves p alone: the smallest gradients do
    assert n < 1000 or moved > 0.3, f"{what}: only {moved:.2f} of the live elements moved"


class _Flat(torch.nn.Module):
    """the smallest owner the fused optimizers accept: one flat parameter buffer and one flat gradient buffer on the GPU"""

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


@pytest.mark.parametrize("kind", ["adam", "sgd_momentum", "sgd_nesterov_wd"])
def test_fused_optimizers_apply_grad_scale_and_keep_it_in_their_state(hip, kind):
    """FusedAdam / FusedSGD with grad_scale = 0.125 (a power of two: scaling commutes with fp32 rounding) equal torch's optimizer fed
    0.125 * g over three steps, to the tolerances of test_adam_matches_torch / test_sgd_matches_torch; and grad_scale survives a
    state_dict() / load_state_dict() round trip into a fresh optimizer, which then takes the same fourth step."""
    from r3m_amd.optim import FusedAdam, FusedSGD
    n = 4096 + 64
    own = _Flat(n, 71)
    pr = own.p.detach().cpu().clone().requires_grad_(True)
    cfg = {"adam": {}, "sgd_momentum": dict(momentum=0.9), "sgd_nesterov_wd": dict(momentum=0.9, nesterov=True, weight_decay=1e-3)}[kind]
    make = (lambda o: FusedAdam([o], lr=1e-4)) if kind == "adam" else (lambda o: FusedSGD([o], lr=1e-2, **cfg))
    opt = make(own)
    ref = torch.optim.Adam([pr], lr=1e-4) if kind == "adam" else torch.optim.SGD([pr], lr=1e-2, **cfg)
    assert opt.grad_scale == 1.0
    opt.grad_scale = 0.125
    grads = [rnd((n,), 72 + i, -0.01, 0.01) * (10.0 ** (i - 1)) for i in range(4)]

    def compare(o):
        torch.testing.assert_close(own.p.detach().cpu(), pr.detach(), rtol=1e-6, atol=1e-9)
        if kind == "adam":
            torch.testing.assert_close(o._m[0].cpu(), ref.state[pr]["exp_avg"], rtol=1e-6, atol=1e-12)
            torch.testing.assert_close(o._v[0].cpu(), ref.state[pr]["exp_avg_sq"], rtol=1e-6, atol=1e-14)
        else:
            rb = ref.state[pr]["momentum_buffer"]
            torch.testing.assert_close(o._buf[0].cpu(), rb, rtol=1e-6, atol=2e-7 * float(rb.abs().max()))

    for g in grads[:3]:
        pr.grad = 0.125 * g
        ref.step()
        own.g.copy_(g.to(DEV))
        opt.step()
        compare(opt)
    sd = opt.state_dict()
    assert sd["grad_scale"] == 0.125
    opt2 = make(own)
    assert opt2.grad_scale == 1.0
    opt2.load_state_dict(sd)
    assert opt2.grad_scale == 0.125
    pr.grad = 0.125 * grads[3]
    ref.step()
    own.g.copy_(grads[3].to(DEV))
    opt2.step()
    compare(opt2)
