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


# ---- BatchNorm passes one by one (tests/test_gpu_bn.py on the GPU, tests/test_bn_geometry.py for the case list on the CPU) ---------------
# A case is (rows, C, dtype); dtype "fp32" | "bf16". The list is derived from what the library itself reports: the plans' BatchNorm
# shapes (r3m_resnet_conv_info) and the launch geometry (r3m_debug_bn_geometry), so it follows the launchers when they change.
BN_GEOM_FIELDS = ("fwd_vec", "fwd_span", "fwd_grid", "red_vec", "rpb", "rpp", "col_blocks", "nblk", "app_vec", "app_span", "app_grid",
                  "slices", "slices_of_rows", "slice_cap")
BN_FRAME_SIZES = [(32, 32), (33, 47), (47, 33), (97, 131), (131, 97), (96, 160), (160, 96)]
BN_CHANNELS = (64, 128, 256, 512, 1024, 2048)          # every channel count behind the stem of ResNet-18 / 34 / 50
BN_LARGE = (32 * 56 * 56, 64)                          # the 56 x 56 x 64 map of 32 frames: 25.7 MB in fp32, many blocks and slices


def bn_geometry(L, rows, C, dtype):
    import ctypes
    buf = (ctypes.c_int * 16)()
    n = L.r3m_debug_bn_geometry(rows, C, 0 if dtype == "fp32" else 1, buf, 16)
    assert n == len(BN_GEOM_FIELDS), L.r3m_last_error()
    return dict(zip(BN_GEOM_FIELDS, buf[:n]))


def bn_span_tail(rows, C, vec, span):
    """where the last block of a span-wide elementwise launch ends: 'full' (n % span == 0), 'one' (one row of vectors, the smallest
    remainder a [rows][C] tensor can leave; a single vector when C == vec), 'all_but_one' (span minus one row of vectors), 'mid_walk'
    (inside the block's 256-wide walk: past its first iteration and not on an iteration boundary, or, when a row fills a whole
    iteration, after exactly two of the four), else 'part'"""
    cv = C // vec
    r = (rows * cv) % span
    if r == 0:
        return "full"
    if r == cv:
        return "one"
    if r == span - cv:
        return "all_but_one"
    if span > 256 and ((r > 256 and r % 256 != 0) or (cv == 256 and r == 512)):
        return "mid_walk"
    return "part"


def bn_class(L, rows, C, dtype):
    """everything the launchers of csrc/bn.hip can tell apart about a [rows][C] tensor, minus the sizes themselves"""
    g = bn_geometry(L, rows, C, dtype)
    nf, na = rows * C // g["fwd_vec"], rows * C // g["app_vec"]
    return (dtype, C, g["fwd_span"], nf % g["fwd_span"] == 0, g["fwd_grid"] > 1, g["col_blocks"], rows < g["rpp"], rows % g["rpb"] == 0,
            g["nblk"] > 1, g["app_span"], na % g["app_span"] == 0, g["app_grid"] > 1, g["slices"] == g["slice_cap"])


def bn_plan_shapes(L, sizes, frame_sizes, frame_counts):
    """distinct (rows, C) = (F * Ho * Wo, Co) of the BatchNorms behind the stem (the stem's own runs the fused pool kernels)"""
    from route_sig import plan_convs
    out = []
    for size in sizes:
        for (H, W) in frame_sizes:
            for F_ in frame_counts:
                h = L.r3m_resnet_create_hw(size, F_, 0, H, W)
                assert h, L.r3m_last_error()
                try:
                    for (Ci, Co, k, s, p, Hi, Wi, Ho, Wo) in plan_convs(L, h)[1:]:
                        if (F_ * Ho * Wo, Co) not in out:
                            out.append((F_ * Ho * Wo, Co))
                finally:
                    L.r3m_resnet_destroy(h)
    return out


_bn_cases = None


def bn_cases():
    """[(rows, C, dtype, why)]: (a) the BatchNorm shapes of ResNet-18 / -50 at BN_FRAME_SIZES for 1 and 3 frames, (b) per channel count and
    dtype the boundaries of every geometry class r3m_debug_bn_geometry reports, (c) one large case per dtype."""
    global _bn_cases
    if _bn_cases is not None:
        return _bn_cases
    from r3m_amd import _lib
    L = _lib.lib()
    out, seen = [], set()

    def add(rows, C, dtype, why):
        if rows >= 1 and (rows, C, dtype) not in seen:
            seen.add((rows, C, dtype))
            out.append((rows, C, dtype, why))

    for (rows, C) in bn_plan_shapes(L, (18, 50), BN_FRAME_SIZES, (1, 3)):
        for dtype in ("fp32", "bf16"):
            add(rows, C, dtype, "plan")
    for dtype in ("fp32", "bf16"):
        for C in BN_CHANNELS:
            g = bn_geometry(L, 1, C, dtype)
            rpp, rpb = g["rpp"], g["rpb"]
            for rows in (rpp - 1, rpp, rpb - 1, rpb, rpb + 1, 2 * rpb - 1, 2 * rpb, 2 * rpb + 1):
                add(rows, C, dtype, "reduce_block")
            for (vec, span) in {(g["fwd_vec"], g["fwd_span"]), (g["app_vec"], g["app_span"])}:
                rps = max(span // (C // vec), 1)                  # rows per span
                for rows in (2 * rps, 2 * rps + 1, 3 * rps - 1):
                    add(rows, C, dtype, "span_tail")
                mid = [r for r in range(2 * rps + 1, 3 * rps) if bn_span_tail(r, C, vec, span) == "mid_walk"]
                if mid:
                    add(mid[0], C, dtype, "span_tail")
            # one representative of every class a row count up to three blocks / spans can fall into
            have = {bn_class(L, r, c, d) for (r, c, d, _) in out if c == C and d == dtype}
            for rows in range(1, 3 * max(rpb, 1024 * 8 // C) + 2):
                cls = bn_class(L, rows, C, dtype)
                if cls not in have:
                    have.add(cls)
                    add(rows, C, dtype, "class")
    # a tail of literally one 16-byte vector needs one vector per row: C = 8 in bf16 (the launchers take it; no mask bits at these sizes)
    add(1025, 8, "bf16", "one_vector")
    add(2047, 8, "bf16", "one_vector")
    for dtype in ("fp32", "bf16"):
        add(BN_LARGE[0], BN_LARGE[1], dtype, "large")
    _bn_cases = out
    return out


def bn_possible_tails(C, vec, span):
    """the tail kinds (bn_span_tail) a multi-block launch over [rows][C] can end in: a row is C / vec items, so the remainder of the last
    block is a multiple of that; rows per span = span / (C / vec) when a row is shorter than the span, else every block is full"""
    rps = span // (C // vec)
    if rps <= 1:
        return {"full"}
    return {bn_span_tail(rps + k, C, vec, span) for k in range(rps)}


def bn_pair_cases():
    """[(rows, C, dtype)] for the paired tail kernels (C >= 64: a downsample block's tail): per channel count and dtype one multi-block
    case of EVERY tail kind the paired second pass can end in (bn_span_tail of the backward-apply span: apply2 / apply2_16 walk their
    span on their own), a single-block case, every case with rows <= 3, the large case, and every third case of the rest."""
    L_ = None
    out, seen = [], set()
    for i, (rows, C, dtype, why) in enumerate(bn_cases()):
        if C < 64:
            continue
        if L_ is None:
            from r3m_amd import _lib
            L_ = _lib.lib()
        g = bn_geometry(L_, rows, C, dtype)
        key = (C, dtype, bn_span_tail(rows, C, g["app_vec"], g["app_span"]), g["app_grid"] > 1)
        if key not in seen or rows <= 3 or why == "large" or i % 3 == 0:
            seen.add(key)
            out.append((rows, C, dtype))
    return out


def bn_case_id(c):
    return "{}x{}_{}_{}".format(*c)


def bn_coef_of(y, gamma, beta, eps=1e-5):
    """fp32 coefficient block [4][C] = mean, invstd, scale, shift from the float64 batch statistics of y"""
    m = y.double().mean(0)
    v = y.double().var(0, unbiased=False)
    inv = 1.0 / torch.sqrt(v + eps)
    sc = gamma.double() * inv
    return torch.stack([m, inv, sc, beta.double() - m * sc]).float()


def bn_pre_activation(inp, mode):
    """float64 t = scale y + shift [+ r] [+ scale2 y2 + shift2] with the fp32 coefficients cast to float64"""
    c = inp["coef"].double()
    t = inp["y"].double() * c[2] + c[3]
    if mode == "identity":
        t = t + inp["r"].double()
    elif mode == "downsample":
        c2 = inp["coef2"].double()
        t = t + (inp["y2"].double() * c2[2] + c2[3])
    return t


def bn_inputs(rows, C, dtype, mode, coef=None, coef2=None):
    """Inputs of one case (CPU tensors, fp32 values; bf16 cases hold bf16-representable values). Coefficients: the batch statistics of y
    / y2 unless given. y is then moved off the ReLU kink of THIS mode (|t| < 1e-3 in float64 -> y + 0.05), so that neither the mask
    recomputed in fp32 nor the bf16 sign check depends on a tie; 'near' is the fraction still within 1e-4 afterwards."""
    q = q_bf16 if dtype == "bf16" else (lambda t: t)
    inp = dict(y=q(rnd((rows, C), 11, -2.0, 3.0)), r=q(rnd((rows, C), 16, 0.0, 1.0)), y2=q(rnd((rows, C), 17, -1.0, 1.0)),
               dz=q(rnd((rows, C), 20)), gamma=rnd((C,), 12, 0.5, 1.5), beta=rnd((C,), 13, -0.3, 0.3), gamma2=rnd((C,), 18, 0.5, 1.5),
               beta2=rnd((C,), 19, -0.3, 0.3))
    inp["coef"] = bn_coef_of(inp["y"], inp["gamma"], inp["beta"]) if coef is None else coef
    inp["coef2"] = bn_coef_of(inp["y2"], inp["gamma2"], inp["beta2"]) if coef2 is None else coef2
    for _ in range(8):
        near = bn_pre_activation(inp, mode).abs() < 1e-3
        if not bool(near.any()):
            break
        inp["y"] = q(torch.where(near, inp["y"] + 0.05, inp["y"]))
    inp["near"] = float((bn_pre_activation(inp, mode).abs() <= 1e-4).double().mean())
    return inp


def bn_bwd_ref(dz, mask, y, coef, use_batch_stats, dt=torch.float64):
    """dbeta, dgamma, dy of BatchNorm (+ mask) backward with the given coefficients, evaluated in `dt` (float64: the reference;
    float32: the witness of what the formula itself loses in fp32)"""
    c = coef.to(dt)
    g = dz.to(dt) * mask.to(dt)
    yhat = (y.to(dt) - c[0]) * c[1]
    db, dg = g.sum(0), (g * yhat).sum(0)
    if use_batch_stats:
        dy = c[2] * (g - g.mean(0) - yhat * (g * yhat).mean(0))
    else:
        dy = c[2] * g
    return db, dg, dy


def unpack_bits(words, n):
    """uint32 / int32 words (numpy) -> bool [n]: element j = bit j & 31 of word j >> 5"""
    w = np.asarray(words).view(np.uint32)
    return (((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).reshape(-1)[:n]).astype(bool)
