import numpy as np
import torch
import torch.nn.functional as F

DEV = "cuda:0"
EPS_BF16 = 2.0 ** -8


def rel_err(a, b):
    """max|a-b| / max|b| and ||a-b||2/||b||2 (float64)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    d = a - b
    return float(np.abs(d).max() / max(np.abs(b).max(), 1e-30)), float(np.linalg.norm(d) / max(np.linalg.norm(b), 1e-30))


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous()


def nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2).contiguous()


def _st():
    return torch.cuda.current_stream().cuda_stream


def q_bf16(x):
    """round to bf16, keep as fp32 (the value the device tensor holds)"""
    return x.to(torch.bfloat16).to(torch.float32)


def pack_bits(mask_nhwc):
    """[..] bool (NHWC element order) -> uint32 words, bit i of word w = element 32 w + i (the engine's 1-bit ReLU mask layout)."""
    flat = mask_nhwc.reshape(-1).to(torch.int64)
    pad = (-flat.numel()) % 32
    if pad:
        flat = torch.cat([flat, torch.zeros(pad, dtype=torch.int64)])
    words = (flat.view(-1, 32) << torch.arange(32, dtype=torch.int64)).sum(1)
    return (words & 0xFFFFFFFF).to(torch.int64).numpy().astype(np.uint32)


# ---- operator checks shared by the square lists (test_gpu_ops.py, test_gpu_bf16.py) and the Hi != Wi lists (test_gpu_ops_hw.py) --------
# case = (N, Hi, Wi, Ci, Co, k, stride, pad). The square modules pass Hi = Wi and leave ref64 / strict at False: what their test bodies
# did before they moved here. The tolerances are the same numbers for every caller.

def check_conv_fp32(hip, case, ref64=False, strict=False):
    """r3m_conv2d_fwd (+ BatchNorm statistic partials), _dgrad, _wgrad (+ accumulate) against F.conv2d + autograd on the CPU, in fp32
    (ref64=False) or float64. strict: outputs pre-filled with NaN, the forward run once more without statistics (flags 0, same
    tolerance), and the pixels a strided 1x1 input gradient does not touch must be exact zeros."""
    N, Hi, Wi, Ci, Co, k, s, p = case
    x = rnd((N, Ci, Hi, Wi), 1)
    w = rnd((Co, Ci, k, k), 2, -0.2, 0.2)
    rt = torch.float64 if ref64 else torch.float32
    xr = x.to(rt).requires_grad_(True)
    wr = w.to(rt).requires_grad_(True)
    y_ref = F.conv2d(xr, wr, stride=s, padding=p)
    Ho, Wo = y_ref.shape[2], y_ref.shape[3]
    dy = rnd(tuple(y_ref.shape), 3)
    y_ref.backward(dy.to(rt))
    fill = float("nan")

    xd = nhwc(x).to(DEV)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV)       # OHWI
    yd = torch.full((N, Ho, Wo, Co), fill, device=DEV) if strict else torch.empty((N, Ho, Wo, Co), device=DEV)
    rows = hip.r3m_conv2d_stats_rows(N, Hi, Wi, Co, k, s, p)
    stats = torch.zeros((rows, 2, Co), device=DEV)
    rc = hip.r3m_conv2d_fwd(xd.data_ptr(), wd.data_ptr(), yd.data_ptr(), stats.data_ptr(), N, Hi, Wi, Ci, Co, k, s, p, _st())
    assert rc == 0, hip.r3m_last_error()
    e_max, e_l2 = rel_err(nchw(yd.cpu()).numpy(), y_ref.detach().numpy())
    assert e_max < 2e-5, f"conv fwd max-rel {e_max}"
    # BatchNorm statistic partials: sum / sum of squares over rows, per output channel
    ssum = stats[:, 0].double().sum(0).cpu().numpy()
    ssq = stats[:, 1].double().sum(0).cpu().numpy()
    yr = y_ref.detach().double()
    np.testing.assert_allclose(ssum, yr.sum((0, 2, 3)).numpy(), rtol=1e-4, atol=1e-3 * float(yr.abs().max()))
    np.testing.assert_allclose(ssq, (yr * yr).sum((0, 2, 3)).numpy(), rtol=1e-4)
    if strict:
        y0 = torch.full((N, Ho, Wo, Co), fill, device=DEV)
        rc = hip.r3m_conv2d_fwd(xd.data_ptr(), wd.data_ptr(), y0.data_ptr(), None, N, Hi, Wi, Ci, Co, k, s, p, _st())
        assert rc == 0, hip.r3m_last_error()
        e_max, _ = rel_err(nchw(y0.cpu()).numpy(), y_ref.detach().numpy())
        assert e_max < 2e-5, f"conv fwd (no statistics) max-rel {e_max}"

    # dgrad
    dyd = nhwc(dy).to(DEV)
    dxd = torch.full((N, Hi, Wi, Ci), fill, device=DEV)
    wsb = hip.r3m_conv2d_dgrad_workspace_bytes(Ci, Co, k)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    rc = hip.r3m_conv2d_dgrad(dyd.data_ptr(), wd.data_ptr(), dxd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, _st())
    assert rc == 0, hip.r3m_last_error()
    dx = nchw(dxd.cpu())
    e_max, _ = rel_err(dx.numpy(), xr.grad.numpy())   # (strided 1x1: odd pixels must come back as exact zeros)
    assert e_max < 2e-5, f"conv dgrad max-rel {e_max}"
    if strict and k == 1 and s > 1:
        untouched = torch.ones((Hi, Wi), dtype=torch.bool)
        untouched[::s, ::s] = False
        assert bool((dx[:, :, untouched] == 0).all()), "strided 1x1 dgrad: a pixel without taps is not an exact zero"

    # wgrad (+ accumulate)
    dwd = torch.full((Co, k, k, Ci), fill, device=DEV) if strict else torch.empty((Co, k, k, Ci), device=DEV)
    wsb = hip.r3m_conv2d_wgrad_workspace_bytes(N, Hi, Wi, Ci, Co, k, s, p)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    rc = hip.r3m_conv2d_wgrad(xd.data_ptr(), dyd.data_ptr(), dwd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, 0, _st())
    assert rc == 0, hip.r3m_last_error()
    dw = dwd.cpu().permute(0, 3, 1, 2)
    e_max, _ = rel_err(dw.numpy(), wr.grad.numpy())
    assert e_max < 5e-5, f"conv wgrad max-rel {e_max}"
    rc = hip.r3m_conv2d_wgrad(xd.data_ptr(), dyd.data_ptr(), dwd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, 1, _st())
    assert rc == 0
    e_max, _ = rel_err(dwd.cpu().permute(0, 3, 1, 2).numpy(), 2 * wr.grad.numpy())
    assert e_max < 5e-5, f"conv wgrad accumulate max-rel {e_max}"


def check_conv_bf16(hip, case, strict=False):
    """The bf16 `_dt` entry points against float64 on the bf16-rounded operands: 2^-8 max / 2^-9 l2 of the output range for the bf16
    results, fp32 level for the statistics and the weight gradient. strict: the forward also once without statistics (flags 0)."""
    N, Hi, Wi, Ci, Co, k, s, p = case
    BF16 = 1
    x = q_bf16(rnd((N, Ci, Hi, Wi), 1))
    w = q_bf16(rnd((Co, Ci, k, k), 2, -0.2, 0.2))
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, stride=s, padding=p)
    Ho, Wo = y_ref.shape[2], y_ref.shape[3]
    dy = q_bf16(rnd(tuple(y_ref.shape), 3))
    y_ref.backward(dy.double())

    xd = nhwc(x).to(DEV).to(torch.bfloat16)
    w32 = w.permute(0, 2, 3, 1).contiguous().to(DEV)              # fp32 master, OHWI
    wd = torch.empty((Co, k, k, Ci), dtype=torch.bfloat16, device=DEV)
    assert hip.r3m_convert_bf16(w32.data_ptr(), wd.data_ptr(), w32.numel(), _st()) == 0, hip.r3m_last_error()
    torch.testing.assert_close(wd.float().cpu(), w.permute(0, 2, 3, 1), rtol=0, atol=0)
    yd = torch.full((N, Ho, Wo, Co), float("nan"), dtype=torch.bfloat16, device=DEV)
    rows = hip.r3m_conv2d_stats_rows(N, Hi, Wi, Co, k, s, p)
    stats = torch.zeros((rows, 2, Co), device=DEV)
    rc = hip.r3m_conv2d_fwd_dt(xd.data_ptr(), wd.data_ptr(), yd.data_ptr(), stats.data_ptr(), N, Hi, Wi, Ci, Co, k, s, p, BF16, _st())
    assert rc == 0, hip.r3m_last_error()
    yr = y_ref.detach()
    e_max, e_l2 = rel_err(nchw(yd.float().cpu()).numpy(), yr.numpy())
    assert e_max < EPS_BF16 and e_l2 < EPS_BF16 / 2, f"conv fwd bf16 max-rel {e_max} l2 {e_l2}"
    # BatchNorm partials come from the fp32 accumulators (before the bf16 rounding of y)
    np.testing.assert_allclose(stats[:, 0].double().sum(0).cpu().numpy(), yr.sum((0, 2, 3)).numpy(), rtol=1e-4,
                               atol=1e-3 * float(yr.abs().max()))
    np.testing.assert_allclose(stats[:, 1].double().sum(0).cpu().numpy(), (yr * yr).sum((0, 2, 3)).numpy(), rtol=1e-4)
    if strict:
        y0 = torch.full((N, Ho, Wo, Co), float("nan"), dtype=torch.bfloat16, device=DEV)
        rc = hip.r3m_conv2d_fwd_dt(xd.data_ptr(), wd.data_ptr(), y0.data_ptr(), None, N, Hi, Wi, Ci, Co, k, s, p, BF16, _st())
        assert rc == 0, hip.r3m_last_error()
        e_max, e_l2 = rel_err(nchw(y0.float().cpu()).numpy(), yr.numpy())
        assert e_max < EPS_BF16 and e_l2 < EPS_BF16 / 2, f"conv fwd bf16 (no statistics) max-rel {e_max} l2 {e_l2}"

    # dgrad
    dyd = nhwc(dy).to(DEV).to(torch.bfloat16)
    dxd = torch.full((N, Hi, Wi, Ci), float("nan"), dtype=torch.bfloat16, device=DEV)
    wsb = hip.r3m_conv2d_dgrad_workspace_bytes(Ci, Co, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    rc = hip.r3m_conv2d_dgrad_dt(dyd.data_ptr(), w32.data_ptr(), dxd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, BF16, _st())
    assert rc == 0, hip.r3m_last_error()
    e_max, e_l2 = rel_err(nchw(dxd.float().cpu()).numpy(), xr.grad.numpy())
    assert e_max < EPS_BF16 and e_l2 < EPS_BF16 / 2, f"conv dgrad bf16 max-rel {e_max} l2 {e_l2}"

    # wgrad: fp32 output (+ accumulate)
    dwd = torch.full((Co, k, k, Ci), float("nan"), device=DEV)
    wsb = hip.r3m_conv2d_wgrad_workspace_bytes_dt(N, Hi, Wi, Ci, Co, k, s, p, BF16)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    for acc in (0, 1):
        rc = hip.r3m_conv2d_wgrad_dt(xd.data_ptr(), dyd.data_ptr(), dwd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, acc,
                                     BF16, _st())
        assert rc == 0, hip.r3m_last_error()
        e_max, _ = rel_err(dwd.cpu().permute(0, 3, 1, 2).numpy(), (acc + 1) * wr.grad.numpy())
        assert e_max < 5e-5, f"conv wgrad bf16 (acc={acc}) max-rel {e_max}"


def check_dgrad_bnred(hip, case, mode, dtype):
    """r3m_conv2d_dgrad_bnred_dt: the stored input gradient and the consumer BatchNorm's backward partials against float64 (see
    test_gpu_ops.py::test_dgrad_epilogue_emits_bn_backward_partials). mode: recompute | bits | bits+residual; dtype: fp32 | bf16."""
    import pytest
    N, Hi, Wi, Ci, Co, k, s, p = case
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    dt = 0 if dtype == "fp32" else 1
    q = (lambda t: t) if dtype == "fp32" else q_bf16
    Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
    w = q(rnd((Co, Ci, k, k), 2, -0.2, 0.2))
    dy = q(rnd((N, Co, Ho, Wo), 3))
    y = q(rnd((N, Ci, Hi, Wi), 4, -1.0, 1.5))                                # the consumer BatchNorm's input
    res = q(rnd((N, Ci, Hi, Wi), 5))                                         # residual gradient joining at this tensor
    res_mask = rnd((N, Ci, Hi, Wi), 6) > 0.0
    scale = rnd((Ci,), 7, 0.5, 1.5)
    shift = rnd((Ci,), 8, -0.5, 0.5)
    mean = rnd((Ci,), 9, -0.2, 0.4)
    bn_mask_bits = rnd((N, Ci, Hi, Wi), 10) > -0.3
    # recomputed mask = fmaf(y, scale, shift) > 0 in fp32: keep every element away from the kink so the decision is unambiguous
    for _ in range(4):
        v = y.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        y = q(torch.where(v.abs() < 1e-3, y + 0.05, y))
    assert not bool(((y.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).abs() < 1e-5).any())
    # float64 expectation
    xr = torch.zeros((N, Ci, Hi, Wi), dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double(), stride=s, padding=p).backward(dy.double())
    dz = xr.grad
    if mode == "bits+residual":
        dz = dz + res.double() * res_mask
    dz_stored = dz.float() if dtype == "fp32" else dz.to(torch.bfloat16).float()
    on = bn_mask_bits if mode != "recompute" else (y.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)) > 0
    g = dz_stored.double() * on
    exp_s1 = g.sum((0, 2, 3)).numpy()
    # device
    dyd, yd = nhwc(dy).to(DEV).to(tdt), nhwc(y).to(DEV).to(tdt)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV)                           # fp32 master (dgrad converts for bf16)
    dxd = torch.full((N, Hi, Wi, Ci), float("nan"), device=DEV, dtype=tdt)
    wsb = hip.r3m_conv2d_dgrad_workspace_bytes(Ci, Co, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    rows = hip.r3m_conv2d_dgrad_bnred_rows(N, Hi, Wi, s)
    part = torch.full((rows, 2, Ci), float("nan"), device=DEV)
    resd = nhwc(res).to(DEV).to(tdt) if mode == "bits+residual" else None
    resb = torch.from_numpy(pack_bits(nhwc(res_mask)).astype(np.int64)).to(torch.int32).to(DEV) if mode == "bits+residual" else None
    bnb = None if mode == "recompute" else torch.from_numpy(pack_bits(nhwc(bn_mask_bits)).astype(np.int64)).to(torch.int32).to(DEV)
    sc, sh, mu = scale.to(DEV), shift.to(DEV), mean.to(DEV)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = hip.r3m_conv2d_dgrad_bnred_dt(dyd.data_ptr(), wd.data_ptr(), dxd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p,
                                       ptr(resd), ptr(resb), yd.data_ptr(), ptr(bnb), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(),
                                       part.data_ptr(), dt, _st())
    assert rc == 0, hip.r3m_last_error()
    dx = nchw(dxd.float().cpu())
    tol = 2e-5 if dtype == "fp32" else 2.0 ** -8
    e_dx = rel_err(dx.numpy(), dz.numpy())[0]
    if not e_dx < tol:      # say WHERE: whole tiles missing (scheduling), single rows (addressing) or everything (arithmetic)
        d = (nhwc(dx).double() - nhwc(dz.double())).abs().reshape(-1, Ci)
        bad = (~torch.isfinite(d)) | (d > tol * float(dz.abs().max()))
        rows = torch.nonzero(bad.any(1)).flatten()
        cols = torch.nonzero(bad.any(0)).flatten()
        pytest.fail(f"dgrad result: max-rel {e_dx}; non-finite {int((~torch.isfinite(d)).sum())}; {len(rows)} bad rows of {d.shape[0]} "
                    f"(first {rows[:6].tolist()}, last {rows[-3:].tolist()}, 128-row tiles {sorted(set((rows // 128).tolist()))[:12]}); "
                    f"{len(cols)} bad columns (first {cols[:6].tolist()}, last {cols[-3:].tolist()})")
    assert torch.isfinite(part).all(), "a partial row was not written"
    # the partials must describe the dz the kernel STORED (bf16: its own rounding of its own fp32 sum)
    g_dev = dx.double() * on
    got_s1 = part[:, 0].double().sum(0).cpu().numpy()
    got_s2 = part[:, 1].double().sum(0).cpu().numpy()
    ref_s1 = g_dev.sum((0, 2, 3)).numpy()
    ref_s2 = (g_dev * (y.double() - mean.double().view(1, -1, 1, 1))).sum((0, 2, 3)).numpy()
    scale1 = float(g_dev.abs().sum((0, 2, 3)).max())
    np.testing.assert_allclose(got_s1, ref_s1, rtol=0, atol=2e-6 * scale1)
    np.testing.assert_allclose(got_s2, ref_s2, rtol=0, atol=4e-6 * scale1)
    # and agree with the float64 expectation to the accuracy of the stored tensor
    np.testing.assert_allclose(got_s1, exp_s1, rtol=0, atol=(2e-5 if dtype == "fp32" else 2e-2) * scale1 / np.sqrt(N * Hi * Wi) + 1e-6 * scale1)
