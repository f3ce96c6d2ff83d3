"""-m gpu: every BatchNorm pass of csrc/bn.hip one by one against a float64 evaluation of the same formula, at the shapes the encoder
makes for frames of any size and at every boundary of the launch geometry (the case list: util.bn_cases, checked on the CPU by
tests/test_bn_geometry.py).

Passes that take coefficients are compared with float64 on the SAME fp32 coefficient values (the check isolates the pass);
r3m_bn_train_coeffs with the float64 sum of the very fp32 partials it is given (its contract). bf16 inputs are rounded first. Backward
references use the ReLU mask the HIP forward produced. Ceilings (tests/util.rel_err against float64), those of test_bn_train_fwd_bwd
and test_bn_bf16_fwd_bwd: fp32 forward 1e-5, dy 2e-4, dgamma / dbeta 1e-4; bf16 forward and dy 2^-8, dgamma / dbeta 2e-4.

Witness rule, rows 1..3 only: there dy = scale (g - mean(g) - yhat mean(g yhat)) is a difference of nearly equal numbers (one row: exactly
0; two rows: yhat^2 = var / (var + eps), the result is eps / (var + eps) ~ 1e-5 of its terms), so a case that misses the ceiling must stay
within 4 x the error of the same formula evaluated in fp32 on the CPU; the figures are in test_bn_backward's docstring."""
import numpy as np
import pytest
import torch

from test_gpu_ops import BNRED_CASES
from test_gpu_ops_hw import HW_BNRED_GROUPS
from util import (DEV, EPS_BF16, bn_bwd_ref, bn_case_id, bn_cases, bn_geometry, bn_inputs, bn_pair_cases, bn_pre_activation, nhwc, pack_bits, q_bf16,
                  rel_err, rnd, unpack_bits)

pytestmark = pytest.mark.gpu

CASES = [(r, c, d) for (r, c, d, _) in bn_cases()]
IDS = [bn_case_id(c) for c in bn_cases()]
TOL = {"fp32": dict(fwd=1e-5, dy=2e-4, dg=1e-4), "bf16": dict(fwd=EPS_BF16, dy=EPS_BF16, dg=2e-4)}
ULP = 2.0 ** -23
FILL_BITS = 0x2AAAAAAA          # what a mask word holds before the kernel writes it


def st():
    return torch.cuda.current_stream().cuda_stream


def tdt(dtype):
    return torch.float32 if dtype == "fp32" else torch.bfloat16


def dti(dtype):
    return 0 if dtype == "fp32" else 1


def dev(t, dtype):
    return t.to(DEV).to(tdt(dtype))


def ptr(t):
    return None if t is None else t.data_ptr()


def run_fwd(hip, inp, mode, relu, want_bits, dtype):
    """r3m_bn_act_fwd_dt on the case's inputs -> (z on the device, mask words int32 on the device or None)"""
    rows, Cc = inp["y"].shape
    yd, coefd = dev(inp["y"], dtype), inp["coef"].to(DEV)
    zd = torch.full((rows, Cc), float("nan"), dtype=tdt(dtype), device=DEV)
    bits = torch.full((rows * Cc // 32,), FILL_BITS, dtype=torch.int32, device=DEV) if want_bits else None
    rd = dev(inp["r"], dtype) if mode == "identity" else None
    y2d = dev(inp["y2"], dtype) if mode == "downsample" else None
    c2d = inp["coef2"].to(DEV) if mode == "downsample" else None
    rc = hip.r3m_bn_act_fwd_dt(yd.data_ptr(), coefd.data_ptr(), ptr(rd), ptr(y2d), ptr(c2d), zd.data_ptr(), rows, Cc, relu, ptr(bits),
                               dti(dtype), st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    return zd, bits


def mask_of(zd, bits):
    """the ReLU mask the HIP forward produced, bool [rows][C] on the CPU"""
    if bits is None:
        return (zd.float() > 0).cpu()
    return torch.from_numpy(unpack_bits(bits.cpu().numpy(), zd.numel()).reshape(tuple(zd.shape)))


def eval_coeffs(hip, inp, second=False):
    """r3m_bn_eval_coeffs on running statistics -> coef [4][C] (CPU fp32), checked against float64 to a few fp32 ulp"""
    Cc = inp["y"].shape[1]
    gamma, beta = (inp["gamma2"], inp["beta2"]) if second else (inp["gamma"], inp["beta"])
    rm, rv = rnd((Cc,), 34 + second, -0.2, 0.4), rnd((Cc,), 36 + second, 0.5, 1.5)
    coef = torch.full((4, Cc), float("nan"), device=DEV)
    gd, bd, rmd, rvd = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)
    assert hip.r3m_bn_eval_coeffs(gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), 1e-5, coef.data_ptr(), Cc, st()) == 0
    got = coef.cpu()
    inv = 1.0 / torch.sqrt(rv.double() + 1e-5)
    sc = gamma.double() * inv
    assert torch.equal(got[0], rm)
    assert float(((got[1].double() - inv).abs() / inv).max()) <= 4 * ULP
    assert float(((got[2].double() - sc).abs() / sc.abs()).max()) <= 6 * ULP
    mag = beta.double().abs() + (rm.double() * sc).abs()
    assert float(((got[3].double() - (beta.double() - rm.double() * sc)).abs() / mag).max()) <= 6 * ULP
    return got


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C_,dtype", CASES, ids=IDS)
def test_bn_forward(hip, rows, C_, dtype):
    """r3m_bn_act_fwd_dt: plain / identity / downsample x relu 1 / 0 (relu = 0: what no other test runs) x with / without mask bits.
    fp32: the bits equal [z_stored > 0] exactly; bf16: they equal the float64 sign wherever |t| > 1e-4 (nothing is left out: the inputs
    are built clear of the kink, at most 0.1 % may be)."""
    bits_ok = (rows * C_) % 32 == 0
    for mode in ("plain", "identity", "downsample"):
        inp = bn_inputs(rows, C_, dtype, mode)
        t = bn_pre_activation(inp, mode)
        for relu in (1, 0):
            z_ref = torch.relu(t) if relu else t
            z_first = None
            for want_bits in ((False, True) if bits_ok else (False,)):
                zd, bits = run_fwd(hip, inp, mode, relu, want_bits, dtype)
                e = rel_err(zd.float().cpu().numpy(), z_ref.numpy())[0]
                assert e < TOL[dtype]["fwd"], f"{mode} relu={relu} bits={want_bits}: forward max-rel {e}"
                if z_first is None:
                    z_first = zd
                else:
                    assert torch.equal(zd, z_first), "the stored activation depends on whether mask bits are asked for"
                if want_bits:
                    got = mask_of(zd, bits)
                    if dtype == "fp32":
                        assert torch.equal(got, (zd > 0).cpu()), f"{mode} relu={relu}: mask bits differ from z_stored > 0"
                    else:
                        far = t.abs() > 1e-4
                        assert float((~far).double().mean()) <= 1e-3
                        assert torch.equal(got[far], (t > 0)[far]), f"{mode} relu={relu}: mask bits differ from the float64 sign"


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def run_bwd(hip, inp, coef, source, zd, bits, ubs, acc, dg0, db0, dtype):
    rows, Cc = inp["y"].shape
    yd, dzd, coefd = dev(inp["y"], dtype), dev(inp["dz"], dtype), coef.to(DEV)
    wsb = hip.r3m_bn_workspace_bytes(rows, Cc)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dg = dg0.to(DEV) if acc else torch.full((Cc,), float("nan"), device=DEV)
    db = db0.to(DEV) if acc else torch.full((Cc,), float("nan"), device=DEV)
    dyd = torch.full((rows, Cc), float("nan"), dtype=tdt(dtype), device=DEV)
    rc = hip.r3m_bn_bwd_dt(dzd.data_ptr(), zd.data_ptr() if source == "zmask" else None, bits.data_ptr() if source == "bits" else None,
                           yd.data_ptr(), coefd.data_ptr(), dg.data_ptr(), db.data_ptr(), dyd.data_ptr(), ws.data_ptr(), wsb, rows, Cc,
                           ubs, acc, dti(dtype), st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    return dg, db, dyd


def check_bwd(tag, rows, dtype, got, ref, wit, base=(None, None)):
    """got = (dg, db, dy) device; ref / wit = (db, dg, dy) in float64 / fp32; base = (dg0, db0) the buffers accumulated onto"""
    dg, db, dyd = got
    db_ref, dg_ref, dy_ref = ref
    if base[0] is not None:
        dg_ref, db_ref = dg_ref + base[0].double(), db_ref + base[1].double()
    tol = TOL[dtype]
    q = q_bf16 if dtype == "bf16" else (lambda x: x)
    for name, a, b, w, ceil in (("dy", dyd.float().cpu(), dy_ref, q(wit[2]), tol["dy"]), ("dgamma", dg.cpu(), dg_ref, None, tol["dg"]),
                                ("dbeta", db.cpu(), db_ref, None, tol["dg"])):
        e = rel_err(a.numpy(), b.numpy())[0]
        if not e < ceil and rows <= 3 and w is not None:          # the witness rule (module docstring)
            e_w = rel_err(w.numpy(), b.numpy())[0]
            print(f"witness {tag} rows={rows} {name}: HIP {e:.3e} fp32-formula {e_w:.3e}")
            assert e <= 4 * e_w, f"{tag}: {name} max-rel {e} > 4 x the fp32 formula's {e_w}"
        else:
            assert e < ceil, f"{tag}: {name} max-rel {e}"


@pytest.mark.parametrize("rows,C_,dtype", CASES, ids=IDS)
def test_bn_backward(hip, rows, C_, dtype):
    """r3m_bn_bwd_dt: use_batch_stats 1 (given coefficients) and 0 (eval backward: coefficients from r3m_bn_eval_coeffs, c1 = c2 = 0) x
    accumulate 0 / 1 onto non-zero buffers (different ones for dgamma and dbeta) x every mask source: recompute, zmask tensor and bits
    in fp32, recompute and bits in bf16, the mask being that of a plain forward (all sources give dy bit for bit) and of an identity
    forward (zmask / bits only). Witness rule for rows <= 3: with one row dy is an exact zero on both sides; with two and three rows
    the fp32 formula on the CPU is 1.4e-7 / 1.1e-7 (fp32) and 2.0e-8 / 6.1e-8 (bf16, before the rounding of dy) from float64 at C = 64,
    far under the ceilings, because moving y off the ReLU kink after the coefficients are fixed removes the cancellation. A case that
    does need the rule prints its pair (HIP error, fp32-formula error) before it asserts."""
    bits_ok = (rows * C_) % 32 == 0
    dg0, db0 = rnd((C_,), 41, 1.0, 2.0), rnd((C_,), 42, -3.0, -2.0)
    for ubs in (1, 0):
        for mode in ("plain", "identity"):
            base = bn_inputs(rows, C_, dtype, mode)
            inp = base if ubs else bn_inputs(rows, C_, dtype, mode, coef=eval_coeffs(hip, base))
            coef = inp["coef"]
            zd, bits = run_fwd(hip, inp, mode, 1, bits_ok, dtype)
            mask = mask_of(zd, bits)
            if dtype == "fp32":
                sources = (["recompute"] if mode == "plain" else []) + ["zmask"] + (["bits"] if bits_ok else [])
            else:
                sources = (["recompute"] if mode == "plain" else []) + (["bits"] if bits_ok else [])
            ref = bn_bwd_ref(inp["dz"], mask, inp["y"], coef, ubs)
            wit = bn_bwd_ref(inp["dz"], mask, inp["y"], coef, ubs, torch.float32)
            for acc in (0, 1):
                first = None
                for source in sources:
                    got = run_bwd(hip, inp, coef, source, zd, bits, ubs, acc, dg0, db0, dtype)
                    tag = f"{mode} use_batch_stats={ubs} accumulate={acc} mask={source}"
                    if first is None:
                        first = got
                        check_bwd(tag, rows, dtype, got, ref, wit, (dg0, db0) if acc else (None, None))
                    else:
                        assert torch.equal(got[2], first[2]), f"{tag}: dy differs from mask={sources[0]}"
                        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), f"{tag}: dgamma / dbeta differ from mask={sources[0]}"


# ---- the paired tail kernels -----------------------------------------------------------------------------------------------------------
PAIR_CASES = bn_pair_cases()          # every tail kind of the paired second pass per (C, dtype): checked by tests/test_bn_geometry.py


@pytest.mark.parametrize("rows,C_,dtype", PAIR_CASES, ids=[f"{r}x{c}_{d}" for (r, c, d) in PAIR_CASES])
def test_bn_backward_pair(hip, rows, C_, dtype):
    """r3m_bn_bwd_pair_dt (bn_bwd_apply_kernel / bn_bwd_reduce_kernel with NB = 2) on out = relu(bn_a(y) + bn_b(y2)) against two r3m_bn_bwd_dt
    calls on the same inputs: dy bit for bit; dgamma / dbeta bit for bit in fp32 (first passes one after the other), within the
    ceilings in bf16 (joint first pass); both orders against float64. use_batch_stats 1 / 0 x accumulate 0 / 1."""
    inp = bn_inputs(rows, C_, dtype, "downsample")
    zd, bits = run_fwd(hip, inp, "downsample", 1, True, dtype)
    mask = mask_of(zd, bits)
    dg0, db0 = rnd((C_,), 41, 1.0, 2.0), rnd((C_,), 42, -3.0, -2.0)
    dg0b, db0b = rnd((C_,), 43, 3.0, 4.0), rnd((C_,), 44, -5.0, -4.0)
    ya, yb, dzd = dev(inp["y"], dtype), dev(inp["y2"], dtype), dev(inp["dz"], dtype)
    wsb = hip.r3m_bn_pair_workspace_bytes(rows, C_)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    for ubs in (1, 0):
        refa = bn_bwd_ref(inp["dz"], mask, inp["y"], inp["coef"], ubs)
        refb = bn_bwd_ref(inp["dz"], mask, inp["y2"], inp["coef2"], ubs)
        wita = bn_bwd_ref(inp["dz"], mask, inp["y"], inp["coef"], ubs, torch.float32)
        witb = bn_bwd_ref(inp["dz"], mask, inp["y2"], inp["coef2"], ubs, torch.float32)
        for acc in (0, 1):
            c6a = torch.cat([inp["coef"], torch.full((2, C_), float("nan"))]).to(DEV)
            c6b = torch.cat([inp["coef2"], torch.full((2, C_), float("nan"))]).to(DEV)
            start = lambda t: t.to(DEV) if acc else torch.full((C_,), float("nan"), device=DEV)
            dga, dba, dgb, dbb = start(dg0), start(db0), start(dg0b), start(db0b)
            dya = torch.full((rows, C_), float("nan"), dtype=tdt(dtype), device=DEV)
            dyb = torch.full((rows, C_), float("nan"), dtype=tdt(dtype), device=DEV)
            rc = hip.r3m_bn_bwd_pair_dt(dzd.data_ptr(), bits.data_ptr(), ya.data_ptr(), c6a.data_ptr(), yb.data_ptr(), c6b.data_ptr(),
                                        dga.data_ptr(), dba.data_ptr(), dya.data_ptr(), dgb.data_ptr(), dbb.data_ptr(), dyb.data_ptr(),
                                        ws.data_ptr(), wsb, rows, C_, ubs, acc, dti(dtype), st())
            assert rc == 0, hip.r3m_last_error()
            torch.cuda.synchronize()
            tag = f"pair use_batch_stats={ubs} accumulate={acc}"
            if not ubs:
                assert float(c6a[4:].abs().max()) == 0.0 and float(c6b[4:].abs().max()) == 0.0, "eval backward: c1 / c2 must be 0"
            for side, y_key, c_key, got, ref, wit, b0 in (("A", "y", "coef", (dga, dba, dya), refa, wita, (dg0, db0)),
                                                          ("B", "y2", "coef2", (dgb, dbb, dyb), refb, witb, (dg0b, db0b))):
                one = dict(inp, y=inp[y_key])
                alone = run_bwd(hip, one, inp[c_key], "bits", zd, bits, ubs, acc, b0[0], b0[1], dtype)
                assert torch.equal(got[2], alone[2]), f"{tag} {side}: dy differs from the stand-alone call"
                if dtype == "fp32":
                    assert torch.equal(got[0], alone[0]) and torch.equal(got[1], alone[1]), f"{tag} {side}: dgamma / dbeta differ"
                else:
                    assert rel_err(got[0].cpu().numpy(), alone[0].cpu().numpy())[0] < TOL[dtype]["dg"]
                    assert rel_err(got[1].cpu().numpy(), alone[1].cpu().numpy())[0] < TOL[dtype]["dg"]
                check_bwd(f"{tag} {side}", rows, dtype, got, ref, wit, b0 if acc else (None, None))
                check_bwd(f"{tag} {side} stand-alone", rows, dtype, alone, ref, wit, b0 if acc else (None, None))


# ---- the fused first pass: dgrad epilogue -> combine with the invstd scaling -> apply -----------------------------------------------------
_HW = {c: modes for g in HW_BNRED_GROUPS.values() for (c, modes) in g}
FUSED_CASES = [(N, H, H, Ci, Co, k, s, p) for (N, H, Ci, Co, k, s, p) in
               (BNRED_CASES[0], BNRED_CASES[2], BNRED_CASES[3], BNRED_CASES[5], BNRED_CASES[7], BNRED_CASES[9])] + \
              [c for c in ((2, 10, 24, 128, 128, 3, 1, 1), (2, 13, 10, 128, 128, 3, 2, 1), (3, 6, 10, 1024, 256, 1, 1, 0),
                           (3, 3, 5, 512, 2048, 1, 1, 0), (3, 32, 6, 256, 256, 3, 1, 1))]
assert all(c in _HW for c in FUSED_CASES[6:])
# the bf16 kernels take channel counts that are multiples of 64
FUSED_PARAMS = [(c, mode, dtype) for c in FUSED_CASES for mode in ("recompute", "bits", "bits+residual") for dtype in ("fp32", "bf16")
                if dtype == "fp32" or (c[3] % 64 == 0 and c[4] % 64 == 0)]


@pytest.mark.parametrize("case,mode,dtype", FUSED_PARAMS, ids=lambda v: "N{}_{}x{}_{}to{}_k{}s{}p{}".format(*v) if isinstance(v, tuple) else v)
def test_bn_backward_from_dgrad_partials(hip, case, mode, dtype):
    """r3m_conv2d_dgrad_bnred_dt, then r3m_bn_bwd_from_partials_dt (the fp32 plans' default schedule: EPI_BNRED partials -> combine with
    second_sum_scale = invstd -> apply) against the float64 BatchNorm backward of the dx the dgrad STORED."""
    N, Hi, Wi, Ci, Co, k, s, p = case
    q = (lambda t: t) if dtype == "fp32" else q_bf16
    Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
    w = q(rnd((Co, Ci, k, k), 2, -0.2, 0.2))
    dy = q(rnd((N, Co, Ho, Wo), 3))
    y = q(rnd((N, Ci, Hi, Wi), 4, -1.0, 1.5))
    res = q(rnd((N, Ci, Hi, Wi), 5))
    res_mask = rnd((N, Ci, Hi, Wi), 6) > 0.0
    scale, shift, mean, invstd = rnd((Ci,), 7, 0.5, 1.5), rnd((Ci,), 8, -0.5, 0.5), rnd((Ci,), 9, -0.2, 0.4), rnd((Ci,), 12, 0.5, 2.0)
    bn_mask_bits = rnd((N, Ci, Hi, Wi), 10) > -0.3
    v = lambda: y.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    for _ in range(4):
        y = q(torch.where(v().abs() < 1e-3, y + 0.05, y))
    assert not bool((v().abs() < 1e-5).any())
    on = bn_mask_bits if mode != "recompute" else v() > 0
    dyd, yd = dev(nhwc(dy), dtype), dev(nhwc(y), dtype)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    dxd = torch.full((N, Hi, Wi, Ci), float("nan"), device=DEV, dtype=tdt(dtype))
    wsb = hip.r3m_conv2d_dgrad_workspace_bytes(Ci, Co, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    prow = hip.r3m_conv2d_dgrad_bnred_rows(N, Hi, Wi, s)
    part = torch.full((prow, 2, Ci), float("nan"), device=DEV)
    resd = dev(nhwc(res), dtype) if mode == "bits+residual" else None
    to_words = lambda m: torch.from_numpy(pack_bits(nhwc(m)).astype(np.int64)).to(torch.int32).to(DEV)
    resb = to_words(res_mask) if mode == "bits+residual" else None
    bnb = None if mode == "recompute" else to_words(bn_mask_bits)
    coef = torch.stack([mean, invstd, scale, shift])
    coefd = coef.to(DEV)
    rc = hip.r3m_conv2d_dgrad_bnred_dt(dyd.data_ptr(), wd.data_ptr(), dxd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p,
                                       ptr(resd), ptr(resb), yd.data_ptr(), ptr(bnb), coefd[2].data_ptr(), coefd[3].data_ptr(),
                                       coefd[0].data_ptr(), part.data_ptr(), dti(dtype), st())
    assert rc == 0, hip.r3m_last_error()
    rows = N * Hi * Wi
    dz_stored = dxd.float().cpu().reshape(rows, Ci)
    assert bool(torch.isfinite(dz_stored).all()) and bool(torch.isfinite(part).all())
    y2d, on2d = nhwc(y).reshape(rows, Ci), nhwc(on).reshape(rows, Ci)
    wsb2 = hip.r3m_bn_workspace_bytes(rows, Ci)
    ws2 = torch.empty(wsb2, dtype=torch.uint8, device=DEV)
    dg0, db0 = rnd((Ci,), 41, 1.0, 2.0), rnd((Ci,), 42, -3.0, -2.0)
    for ubs, acc in ((1, 0), (0, 1), (1, 1)):
        dg = dg0.to(DEV) if acc else torch.full((Ci,), float("nan"), device=DEV)
        db = db0.to(DEV) if acc else torch.full((Ci,), float("nan"), device=DEV)
        dyo = torch.full((rows, Ci), float("nan"), dtype=tdt(dtype), device=DEV)
        rc = hip.r3m_bn_bwd_from_partials_dt(dxd.data_ptr(), ptr(bnb), yd.data_ptr(), coefd.data_ptr(), part.data_ptr(), prow, dg.data_ptr(),
                                             db.data_ptr(), dyo.data_ptr(), ws2.data_ptr(), wsb2, rows, Ci, ubs, acc, dti(dtype), st())
        assert rc == 0, hip.r3m_last_error()
        torch.cuda.synchronize()
        ref = bn_bwd_ref(dz_stored, on2d, y2d, coef, ubs)
        wit = bn_bwd_ref(dz_stored, on2d, y2d, coef, ubs, torch.float32)
        check_bwd(f"fused {mode} use_batch_stats={ubs} accumulate={acc}", rows, dtype, (dg, db, dyo), ref, wit, (dg0, db0) if acc else (None, None))


@pytest.mark.parametrize("C_,rows", [(64, 16 * 256 - 16), (64, 16 * 256 - 15), (64, 16 * 256 + 4), (2048, 16 * 64 - 16), (2048, 16 * 64 - 15),
                                     (2048, 16 * 64 + 6)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bn_backward_from_partials_slice_cap(hip, C_, rows, dtype):
    """r3m_bn_bwd_from_partials_dt with one partial row per tensor row (any blocking is the contract), so that the slice count of the fp64
    reduce sits one below, at and above its cap (256 at C = 64, 64 at C = 2048) in the BACKWARD finalize: dgamma / dbeta against the
    float64 sum of the very partials, dy against float64."""
    g = bn_geometry(hip, rows, C_, dtype)
    assert g["slices_of_rows"] == min((rows + 15) // 16, g["slice_cap"])
    inp = bn_inputs(rows, C_, dtype, "plain")
    coef = inp["coef"]
    zd, bits = run_fwd(hip, inp, "plain", 1, True, dtype)
    mask = mask_of(zd, bits)
    gg = inp["dz"].double() * mask
    part = torch.stack([gg, gg * (inp["y"].double() - coef[0].double())], 1).float().contiguous()       # [rows][2][C]
    db_ref = part[:, 0].double().sum(0)
    dg_ref = part[:, 1].double().sum(0) * coef[1].double()
    _, _, dy_ref = bn_bwd_ref(inp["dz"], mask, inp["y"], coef, 1)
    partd, yd, dzd, coefd = part.to(DEV), dev(inp["y"], dtype), dev(inp["dz"], dtype), coef.to(DEV)
    wsb = hip.r3m_bn_workspace_bytes(rows, C_)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dg, db = torch.full((C_,), float("nan"), device=DEV), torch.full((C_,), float("nan"), device=DEV)
    dyo = torch.full((rows, C_), float("nan"), dtype=tdt(dtype), device=DEV)
    rc = hip.r3m_bn_bwd_from_partials_dt(dzd.data_ptr(), bits.data_ptr(), yd.data_ptr(), coefd.data_ptr(), partd.data_ptr(), rows, dg.data_ptr(),
                                         db.data_ptr(), dyo.data_ptr(), ws.data_ptr(), wsb, rows, C_, 1, 0, dti(dtype), st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    assert rel_err(dg.cpu().numpy(), dg_ref.numpy())[0] < 1e-6
    assert rel_err(db.cpu().numpy(), db_ref.numpy())[0] < 1e-6
    assert rel_err(dyo.float().cpu().numpy(), dy_ref.numpy())[0] < TOL[dtype]["dy"]


# ---- training coefficients ------------------------------------------------------------------------------------------------------------
def _train_coeffs(hip, part, count, gamma, beta, rm, rv):
    nb, _, Cc = part.shape
    coef = torch.full((4, Cc), float("nan"), device=DEV)
    wsb = hip.r3m_bn_workspace_bytes(max(count, 1), Cc)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    partd, gd, bd = part.to(DEV), gamma.to(DEV), beta.to(DEV)
    rmd, rvd = (None, None) if rm is None else (rm.to(DEV), rv.to(DEV))
    rc = hip.r3m_bn_train_coeffs(partd.data_ptr(), nb, count, gd.data_ptr(), bd.data_ptr(), ptr(rmd), ptr(rvd), 0.1, 1e-5, coef.data_ptr(),
                                 ws.data_ptr(), wsb, Cc, st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    return coef.cpu(), None if rmd is None else rmd.cpu(), None if rvd is None else rvd.cpu()


def _check_train_coeffs(hip, part, count, Cc, with_running):
    """against the float64 sum of the fp32 partials: mean, invstd, scale, shift and the running statistics to a few fp32 ulp of their
    largest term"""
    gamma, beta = rnd((Cc,), 12, 0.5, 1.5), rnd((Cc,), 13, -0.3, 0.3)
    rm, rv = (rnd((Cc,), 14, -0.1, 0.1), rnd((Cc,), 15, 0.5, 1.5)) if with_running else (None, None)
    coef, rm_new, rv_new = _train_coeffs(hip, part, count, gamma, beta, rm, rv)
    assert bool(torch.isfinite(coef).all())
    s, ss = part[:, 0].double().sum(0), part[:, 1].double().sum(0)
    mean = s / count
    var = (ss / count - mean * mean).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + 1e-5)
    sc = gamma.double() * inv
    sh = beta.double() - mean * sc
    # the cancellation in sumsq / count - mean^2 belongs to the contract (fp64 on both sides); what the fp32 steps may add is ulps
    assert float(((coef[0].double() - mean).abs() / mean.abs().clamp_min(1e-30)).max()) <= 1 * ULP
    assert float(((coef[1].double() - inv).abs() / inv).max()) <= 4 * ULP
    assert float(((coef[2].double() - sc).abs() / sc.abs()).max()) <= 6 * ULP
    assert float(((coef[3].double() - sh).abs() / (beta.double().abs() + (mean * sc).abs())).max()) <= 6 * ULP
    if with_running:
        unbias = count / (count - 1) if count > 1 else 1.0
        rm_ref = 0.9 * rm.double() + 0.1 * mean
        rv_ref = 0.9 * rv.double() + 0.1 * var * unbias
        assert bool(torch.isfinite(rm_new).all()) and bool(torch.isfinite(rv_new).all())
        assert float(((rm_new.double() - rm_ref).abs() / (0.9 * rm.double().abs() + 0.1 * mean.abs())).max()) <= 4 * ULP
        assert float(((rv_new.double() - rv_ref).abs() / rv_ref.abs()).max()) <= 4 * ULP
    return coef, var


@pytest.mark.parametrize("with_running", [True, False], ids=["running", "no_running"])
@pytest.mark.parametrize("blk", [64, 128, 256])
@pytest.mark.parametrize("rows,C_", [(1, 64), (2, 2048), (3, 512), (777, 256), (3 * 25 * 33, 64), (2 * 56 * 56 + 5, 64), (1000, 2048)])
def test_bn_train_coeffs_blockings(hip, rows, C_, blk, with_running):
    """partials cut in blocks of 64, 128 and 256 rows with a ragged last block (the engine's conv epilogues use all three), count 1, 2, 3
    and larger, running statistics given or NULL"""
    y = rnd((rows, C_), 11, -2.0, 3.0)
    nb = (rows + blk - 1) // blk
    part = torch.zeros((nb, 2, C_))
    for i in range(nb):
        sl = y[i * blk:(i + 1) * blk]
        part[i, 0], part[i, 1] = sl.sum(0), (sl * sl).sum(0)
    _check_train_coeffs(hip, part, rows, C_, with_running)


@pytest.mark.parametrize("with_running", [True, False], ids=["running", "no_running"])
@pytest.mark.parametrize("C_,stats_rows", [(C_, r) for C_, cap in ((64, 256), (2048, 64))
                                           for r in (1, 16 * cap - 16, 16 * cap - 15, 16 * cap - 1, 16 * cap, 16 * cap + 1, 32 * cap + 5)])
def test_bn_train_coeffs_slices(hip, C_, stats_rows, with_running):
    """stats_rows = 1 and just below, at and above 16 x cap (the slice count of the fp64 reduce one under, at and clamped to its cap: 256
    at C = 64, 64 at C = 2048): the coefficients are those of the float64 sum of ALL the partial rows"""
    g = bn_geometry(hip, stats_rows, C_, "fp32")
    assert g["slices_of_rows"] == min((stats_rows + 15) // 16, g["slice_cap"])
    count = stats_rows * 8
    part = torch.stack([rnd((stats_rows, C_), 21, 2.0, 6.0), rnd((stats_rows, C_), 22, 20.0, 30.0)], 1).contiguous()   # var ~ 2.9 - 0.25
    _check_train_coeffs(hip, part, count, C_, with_running)


@pytest.mark.parametrize("C_", [64, 512, 2048])
def test_bn_train_coeffs_count_one(hip, C_):
    """count = 1 (layer4 of one frame at 32 x 32; torch refuses it): what include/r3m_hip.h defines. Exact partials (y with 8 significant
    bits, so y^2 is exact in fp32): variance exactly 0, invstd = 1 / sqrt(eps), shift = beta - y scale, running_var = 0.9 rv + 0.1 * 0,
    all finite. Partials whose sum of squares exceeds y^2: that excess is the variance and enters running_var with the unbiased factor
    taken as 1."""
    y = (rnd((1, C_), 11, -2.0, 3.0) * 64).round() / 64
    part = torch.stack([y, y * y], 1)
    coef, var = _check_train_coeffs(hip, part, 1, C_, True)
    assert float(var.abs().max()) == 0.0
    inv0 = float(1.0 / np.sqrt(np.float32(0.0) + np.float32(1e-5)))
    assert float((coef[1] - inv0).abs().max()) <= 4 * ULP * inv0 and torch.equal(coef[0], y[0])
    part2 = torch.stack([y, y * y + 0.25], 1)
    coef2, var2 = _check_train_coeffs(hip, part2, 1, C_, True)          # the reference inside uses unbias = 1 for count = 1
    assert float((var2 - 0.25).abs().max()) < 1e-6
    _check_train_coeffs(hip, part2, 1, C_, False)
