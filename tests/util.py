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
    # C = 4 is the one channel count at which bf16 runs the 4-wide kernels: a multiple of 32 elements (mask bits), and three blocks
    # whose last one holds one vector (no bits)
    for dtype in ("fp32", "bf16"):
        add(512, 4, dtype, "narrow")
        add(513, 4, dtype, "narrow")
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
    case of EVERY tail kind the paired second pass can end in (bn_span_tail of the backward-apply span: the NB = 2 instantiations of
    bn_bwd_apply_kernel walk their span on their own), a single-block case, every case with rows <= 3, the large case, and every third case of the rest."""
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


# ---- the fused stem tail on continuous values (tests/test_gpu_ops_hw.py at N = 2, C = 64; tests/test_gpu_pool_edges.py at its launch edges) ----
def check_stem_tail_fused_vs_torch(hip, N, H, W, C, dtype):
    """r3m_bn_relu_maxpool_fwd_dt / r3m_bn_maxpool_bwd_dt against BatchNorm + ReLU + max-pool in float64 with the same coefficients: the
    body of test_gpu_ops_hw.py::test_stem_tail_fused_vs_torch_hw (its docstring describes the inputs), for any [N, H, W, C]"""
    dt = 0 if dtype == "fp32" else 1
    tdt = torch.float32 if dt == 0 else torch.bfloat16
    rows = N * H * W
    # level index = 7 * (a per-channel permutation of the pixel's place in a 3 x 3 lattice) + a random 0..6: distinct inside any window
    g9 = torch.Generator().manual_seed(60)
    perm = torch.stack([torch.randperm(9, generator=g9) for _ in range(C)], 1)                       # [9][C]
    place = ((torch.arange(H) % 3) * 3).view(H, 1) + (torch.arange(W) % 3).view(1, W)               # [H][W]
    idx = perm[place.reshape(-1)].view(1, H, W, C) * 7 + torch.floor(rnd((N, H, W, C), 61, 0.0, 7.0)).long().clamp(0, 6)
    y = ((idx - 31).float() / 4.0 + 0.125).reshape(rows, C)                                          # levels k/4 + 1/8, exact in bf16
    gam = rnd((C,), 62, 0.5, 1.5)
    m, v = y.double().mean(0), y.double().var(0, unbiased=False)
    inv = 1.0 / torch.sqrt(v + 1e-5)
    # shift each channel's zero crossing to the middle between two levels: |scale * y + shift| >= scale / 8
    sc = (gam.double() * inv)
    sh = -sc * (torch.round(m * 4.0) / 4.0)
    coef = torch.stack([m, inv, sc, sh]).float().contiguous()
    c = coef.double()
    yr = y.double().requires_grad_(True)
    t = yr * c[2] + c[3]
    assert float(t.detach().abs().min()) > 1e-3
    zr = torch.relu(t).reshape(N, H, W, C).permute(0, 3, 1, 2)
    p_ref = F.max_pool2d(zr, 3, 2, 1)
    Ho, Wo = p_ref.shape[2], p_ref.shape[3]
    dp = rnd((N, Ho, Wo, C), 64)
    dp = dp if dt == 0 else q_bf16(dp)
    p_ref.backward(nchw(dp).double())
    g = yr.grad / c[2]                          # dz routed by the pool and masked by the ReLU, as the kernel's first pass sees it
    if dt == 1:                                 # a pixel that is the maximum of up to four windows: the kernel rounds the sum of their
        g = q_bf16(g.float()).double()          # pooled gradients to bf16, as the unfused sequence stores dz (csrc/bn_pool.hip pool_quad)
    yhat = (y.double() - c[0]) * c[1]
    db_ref, dg_ref = g.sum(0), (g * yhat).sum(0)
    dy_ref = c[2] * (g - g.mean(0) - yhat * (g * yhat).mean(0))

    yd, coefd = y.to(DEV).to(tdt), coef.to(DEV)
    pd = torch.full((N, Ho, Wo, C), float("nan"), dtype=tdt, device=DEV)
    am = torch.full((N, Ho, Wo, C), 255, dtype=torch.uint8, device=DEV)
    assert hip.r3m_bn_relu_maxpool_fwd_dt(yd.data_ptr(), coefd.data_ptr(), pd.data_ptr(), am.data_ptr(), N, H, W, C, dt, _st()) == 0, \
        hip.r3m_last_error()
    e = rel_err(nchw(pd.float().cpu()).numpy(), p_ref.detach().numpy())[0]
    assert e < (1e-5 if dt == 0 else EPS_BF16), f"fused BatchNorm + ReLU + max-pool forward {e}"
    dpd = dp.to(DEV).to(tdt)
    wsb = hip.r3m_bn_workspace_bytes(rows, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dg, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    dyd = torch.full((rows, C), float("nan"), dtype=tdt, device=DEV)
    assert hip.r3m_bn_maxpool_bwd_dt(dpd.data_ptr(), am.data_ptr(), yd.data_ptr(), coefd.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                     dyd.data_ptr(), ws.data_ptr(), wsb, N, H, W, C, 1, 0, dt, _st()) == 0, hip.r3m_last_error()
    # tolerances of test_bn_train_fwd_bwd (fp32) / test_bn_bf16_fwd_bwd (bf16)
    assert rel_err(dg.cpu().numpy(), dg_ref.numpy())[0] < (1e-4 if dt == 0 else 2e-4)
    assert rel_err(db.cpu().numpy(), db_ref.numpy())[0] < (1e-4 if dt == 0 else 2e-4)
    assert rel_err(dyd.float().cpu().numpy(), dy_ref.numpy())[0] < (2e-4 if dt == 0 else EPS_BF16)


# ---- the conv epilogues and the tile queues that only the engine launched (tests/test_gpu_conv_epilogues.py) ----------------------------
# r3m_conv2d_fwd_affine_dt, r3m_conv2d_dgrad_join_dt and r3m_debug_next_launch_tile_queues against float64 on the operands the kernel
# multiplies. Ceilings: the ones check_conv_fp32 / check_conv_bf16 / check_dgrad_bnred use for the same stores (fp32 2e-5 of the output
# range; bf16 2^-8 max, 2^-9 l2: the fused stores round once). Every body asserts its input conditions on the float64 reference.
AFFINE, ACCUM, RELU = 128, 2, 16


def describe_bad(got_nhwc, ref_nhwc, tol_abs):
    """WHERE a [.., C] result is off: whole 128-row tiles (scheduling), single rows (addressing), columns (epilogue operands) or everything"""
    C_ = ref_nhwc.shape[-1]
    d = (got_nhwc.double() - ref_nhwc.double()).abs().reshape(-1, C_)
    bad = (~torch.isfinite(d)) | (d > tol_abs)
    rows = torch.nonzero(bad.any(1)).flatten()
    cols = torch.nonzero(bad.any(0)).flatten()
    return (f"non-finite {int((~torch.isfinite(d)).sum())}; {len(rows)} bad rows of {d.shape[0]} (first {rows[:6].tolist()}, last "
            f"{rows[-3:].tolist()}, 128-row tiles {sorted(set((rows // 128).tolist()))[:12]}); {len(cols)} bad columns of {C_} (first "
            f"{cols[:6].tolist()}, last {cols[-3:].tolist()})")


def assert_close_store(what, got_nchw, ref_nchw, dtype):
    """got (fp32 values, CPU, NCHW) against the float64 reference under the shared ceilings; the figures are printed before they are asserted"""
    import pytest
    e_max, e_l2 = rel_err(got_nchw.numpy(), ref_nchw.numpy())
    print(f"{what}: max-rel {e_max:.3e} l2-rel {e_l2:.3e}")
    ok = e_max < 2e-5 if dtype == "fp32" else (e_max < EPS_BF16 and e_l2 < EPS_BF16 / 2)
    if not ok:
        tol = (2e-5 if dtype == "fp32" else EPS_BF16) * float(ref_nchw.abs().max())
        pytest.fail(f"{what}: max-rel {e_max} l2-rel {e_l2}; " + describe_bad(nhwc(got_nchw), nhwc(ref_nchw), tol))


def assert_range(ref, summands, what):
    """the output range is at least 1/4 of the largest summand's: no cancellation that would make a relative ceiling meaningless"""
    top = max(float(s.abs().max()) for s in summands)
    assert float(ref.abs().max()) >= 0.25 * top > 0, f"{what}: output range {float(ref.abs().max())} against summands up to {top}"


class tile_queues:
    """`with tile_queues(hip, sets) as ctr:` the next convolution launches of this thread draw their tiles from sets x 8 zeroed counters
    (what the engine's TileCounters hands every launch); taken back on exit whatever happened"""

    def __init__(self, hip, sets=1):
        self.hip, self.sets = hip, sets
        self.ctr = torch.zeros(sets * 8, dtype=torch.int32, device=DEV)

    def __enter__(self):
        self.hip.r3m_debug_next_launch_tile_queues(self.ctr.data_ptr(), self.sets)
        return self.ctr

    def __exit__(self, *exc):
        self.hip.r3m_debug_next_launch_tile_queues(None, 0)
        return False


def assert_queues_used(ctr, sets_used, what):
    """a launch that drew its tiles from the queues leaves every counter of its set non-zero (every block takes at least one ticket);
    one that kept the static split leaves them zero"""
    c = ctr.cpu().view(-1, 8)
    used = [bool((row > 0).all()) for row in c]
    idle = [bool((row == 0).all()) for row in c]
    assert used[:sets_used] == [True] * sets_used and idle[sets_used:] == [True] * (len(c) - sets_used), f"{what}: tile counters {c.tolist()}"


def _dev_ops(case, dtype):
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    q = (lambda t: t) if dtype == "fp32" else q_bf16
    return tdt, q, (0 if dtype == "fp32" else 1)


def check_conv_affine(hip, case, flags, dtype, queues=0):
    """r3m_conv2d_fwd_affine_dt (the inference store: flags 128, 128|16, 128|2|16) against float64 [relu](conv * scale + shift [+ residual]).
    fp32: also torch.equal to r3m_conv2d_fwd followed by r3m_bn_act_fwd (the header's claim for r3m_resnet_forward, per launch).
    queues = 1: the launch once more with tile queues, torch.equal to the static one, the queues really used; queues = -1: handed over
    but the launcher must keep the static split."""
    N, Hi, Wi, Ci, Co, k, s, p = case
    tdt, q, dt = _dev_ops(case, dtype)
    x = q(rnd((N, Ci, Hi, Wi), 1))
    w = q(rnd((Co, Ci, k, k), 2, -0.2, 0.2))
    y = F.conv2d(x.double(), w.double(), stride=s, padding=p)
    Ho, Wo = y.shape[2], y.shape[3]
    sd = float(y.pow(2).mean().sqrt())
    scale = rnd((Co,), 21, 0.5, 1.5)
    shift = rnd((Co,), 22, -0.6, 0.6) * sd
    res = q(rnd(tuple(y.shape), 23) * sd) if flags & ACCUM else None
    terms = [y * scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1).expand_as(y)] + ([res.double()] if res is not None else [])
    t = sum(terms[1:], terms[0])
    ref = torch.relu(t) if flags & RELU else t
    what = f"affine forward {dtype} flags {flags} {case}"
    assert_range(ref, terms, what)
    if flags & RELU:
        zeros = float((ref == 0).double().mean())
        assert 0.2 <= zeros <= 0.8, f"{what}: {zeros:.2f} of the reference outputs are zero"
    if res is not None:
        assert float(res.abs().max()) > 0

    xd = nhwc(x).to(DEV).to(tdt)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV).to(tdt)               # OHWI (bf16: the values are bf16 already)
    sc, sh = scale.to(DEV), shift.to(DEV)

    def launch():
        out = nhwc(res).to(DEV).to(tdt) if res is not None else torch.full((N, Ho, Wo, Co), float("nan"), dtype=tdt, device=DEV)
        rc = hip.r3m_conv2d_fwd_affine_dt(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), sc.data_ptr(), sh.data_ptr(), N, Hi, Wi, Ci, Co, k, s, p,
                                          flags, dt, _st())
        assert rc == 0, hip.r3m_last_error()
        return out

    out = launch()
    assert_close_store(what, nchw(out.float().cpu()), ref, dtype)
    if dtype == "fp32":
        yd = torch.full((N, Ho, Wo, Co), float("nan"), device=DEV)
        assert hip.r3m_conv2d_fwd(xd.data_ptr(), wd.data_ptr(), yd.data_ptr(), None, N, Hi, Wi, Ci, Co, k, s, p, _st()) == 0, hip.r3m_last_error()
        coef = torch.stack([torch.zeros(Co), torch.ones(Co), scale, shift]).contiguous().to(DEV)
        z = torch.full((N, Ho, Wo, Co), float("nan"), device=DEV)
        rd = nhwc(res).to(DEV) if res is not None else None
        rc = hip.r3m_bn_act_fwd(yd.data_ptr(), coef.data_ptr(), None if rd is None else rd.data_ptr(), None, None, z.data_ptr(), N * Ho * Wo, Co,
                                1 if flags & RELU else 0, None, _st())
        assert rc == 0, hip.r3m_last_error()
        if not torch.equal(out, z):
            import pytest
            pytest.fail(f"{what}: the fused store differs from conv + bn_act_fwd: " + describe_bad(out.cpu(), z.cpu(), 0.0))
    if queues:
        with tile_queues(hip, 1) as ctr:
            out_q = launch()
            assert_queues_used(ctr, 1 if queues > 0 else 0, what)
        if not torch.equal(out_q, out):
            import pytest
            pytest.fail(f"{what}: the launch with tile queues differs from the static split: " + describe_bad(out_q.cpu(), out.cpu(), 0.0))


def check_dgrad_join(hip, case, mode, dtype, queues=0):
    """r3m_conv2d_dgrad_join_dt against float64. mode 'accumulate': dx_old + dgrad with dx_old non-zero everywhere; at a strided 1x1 the
    pixels of the tap-less parity classes must come back bit-identical. mode 'join': dgrad + residual_grad * [bits], dx pre-filled with NaN.
    queues = n > 0: once more with n counter sets of tile queues of which the launches that reach the threshold use one each (all that run,
    in these cases), torch.equal to the static launch."""
    import pytest
    N, Hi, Wi, Ci, Co, k, s, p = case
    tdt, q, dt = _dev_ops(case, dtype)
    Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
    w = q(rnd((Co, Ci, k, k), 2, -0.2, 0.2))
    dy = q(rnd((N, Co, Ho, Wo), 3))
    xr = torch.zeros((N, Ci, Hi, Wi), dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double(), stride=s, padding=p).backward(dy.double())
    dg = xr.grad
    sd = float(dg.pow(2).mean().sqrt())
    what = f"dgrad {mode} {dtype} {case}"
    if mode == "accumulate":
        old = q(rnd((N, Ci, Hi, Wi), 31, 0.25, 1.0) * torch.where(rnd((N, Ci, Hi, Wi), 32) > 0, 1.0, -1.0) * sd)
        assert bool((old != 0).all()), f"{what}: the old contents must be non-zero everywhere"
        terms, ref = [dg, old.double()], dg + old.double()
        res = bits = None
    else:
        res = q(rnd((N, Ci, Hi, Wi), 5) * sd)
        mask = rnd((N, Ci, Hi, Wi), 6) > 0.0
        frac = float(mask.double().mean())
        assert 0.2 <= frac <= 0.8, f"{what}: {frac:.2f} of the bits are set"
        assert float((res.double() * mask).abs().max()) > 0
        terms, ref = [dg, res.double() * mask], dg + res.double() * mask
        bits = torch.from_numpy(pack_bits(nhwc(mask)).astype(np.int64)).to(torch.int32).to(DEV)
    assert_range(ref, terms, what)

    dyd = nhwc(dy).to(DEV).to(tdt)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV)                        # fp32 master (the entry point transposes / converts)
    wsb = hip.r3m_conv2d_dgrad_workspace_bytes(Ci, Co, k)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    resd = nhwc(res).to(DEV).to(tdt) if res is not None else None

    def launch():
        dxd = nhwc(old).to(DEV).to(tdt) if mode == "accumulate" else torch.full((N, Hi, Wi, Ci), float("nan"), dtype=tdt, device=DEV)
        rc = hip.r3m_conv2d_dgrad_join_dt(dyd.data_ptr(), wd.data_ptr(), dxd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p,
                                          1 if mode == "accumulate" else 0, None if resd is None else resd.data_ptr(),
                                          None if bits is None else bits.data_ptr(), dt, _st())
        assert rc == 0, hip.r3m_last_error()
        return dxd

    dxd = launch()
    dx = nchw(dxd.float().cpu())
    assert_close_store(what, dx, ref, dtype)
    if mode == "accumulate" and k == 1 and s > 1:
        untouched = torch.ones((Hi, Wi), dtype=torch.bool)
        untouched[::s, ::s] = False
        assert bool(untouched.any()) and torch.equal(dx[:, :, untouched], old[:, :, untouched]), \
            f"{what}: a pixel of a parity class without taps did not keep its old contents bit for bit"
    if queues:
        with tile_queues(hip, queues) as ctr:
            dx_q = launch()
            launches = 1 if (s == 1 or k == 1) else 4
            assert_queues_used(ctr, launches, what)
        if not torch.equal(dx_q, dxd):
            pytest.fail(f"{what}: the launch with tile queues differs from the static split: " + describe_bad(dx_q.cpu(), dxd.cpu(), 0.0))


def check_conv_queues(hip, case, kind, used=True):
    """fp32 r3m_conv2d_fwd with statistics (kind 'fwd_stats') or r3m_conv2d_dgrad (kind 'dgrad'; four counter sets, one per parity launch of
    a stride-2 3x3) with tile queues: NaN-prefilled output against float64 (a tile no queue serves stays NaN) and torch.equal to the
    static launch (per tile the order of the MFMA sums is the same). used = False: the launcher must keep the static split."""
    import pytest
    N, Hi, Wi, Ci, Co, k, s, p = case
    x = rnd((N, Ci, Hi, Wi), 1)
    w = rnd((Co, Ci, k, k), 2, -0.2, 0.2)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    what = f"tile queues {kind} {case}"
    if kind == "fwd_stats":
        ref = F.conv2d(x.double(), w.double(), stride=s, padding=p)
        Ho, Wo = ref.shape[2], ref.shape[3]
        xd = nhwc(x).to(DEV)
        rows = hip.r3m_conv2d_stats_rows(N, Hi, Wi, Co, k, s, p)
        sets, launches = 1, 1

        def launch():
            yd = torch.full((N, Ho, Wo, Co), float("nan"), device=DEV)
            stats = torch.full((rows, 2, Co), float("nan"), device=DEV)
            rc = hip.r3m_conv2d_fwd(xd.data_ptr(), wd.data_ptr(), yd.data_ptr(), stats.data_ptr(), N, Hi, Wi, Ci, Co, k, s, p, _st())
            assert rc == 0, hip.r3m_last_error()
            return yd, stats
    else:
        Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
        dy = rnd((N, Co, Ho, Wo), 3)
        xr = torch.zeros((N, Ci, Hi, Wi), dtype=torch.float64, requires_grad=True)
        F.conv2d(xr, w.double(), stride=s, padding=p).backward(dy.double())
        ref = xr.grad
        dyd = nhwc(dy).to(DEV)
        wsb = hip.r3m_conv2d_dgrad_workspace_bytes(Ci, Co, k)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
        sets = 4
        launches = 1 if s == 1 else (4 if k == 3 else 1)

        def launch():
            dxd = torch.full((N, Hi, Wi, Ci), float("nan"), device=DEV)
            rc = hip.r3m_conv2d_dgrad(dyd.data_ptr(), wd.data_ptr(), dxd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, _st())
            assert rc == 0, hip.r3m_last_error()
            return dxd, None

    out_s, stats_s = launch()
    with tile_queues(hip, sets) as ctr:
        out_q, stats_q = launch()
        assert_queues_used(ctr, launches if used else 0, what)
    assert_close_store(what + " (queues)", nchw(out_q.cpu()), ref, "fp32")
    assert_close_store(what + " (static)", nchw(out_s.cpu()), ref, "fp32")
    if not torch.equal(out_q, out_s):
        pytest.fail(f"{what}: the launch with tile queues differs from the static split: " + describe_bad(out_q.cpu(), out_s.cpu(), 0.0))
    if stats_s is not None:
        assert torch.isfinite(stats_q).all(), f"{what}: a statistics row was not written"
        assert torch.equal(stats_q, stats_s), f"{what}: the statistics partials differ between the queue and the static launch"
        yr = ref.double()
        np.testing.assert_allclose(stats_q[:, 0].double().sum(0).cpu().numpy(), yr.sum((0, 2, 3)).numpy(), rtol=1e-4, atol=1e-3 * float(yr.abs().max()))
        np.testing.assert_allclose(stats_q[:, 1].double().sum(0).cpu().numpy(), (yr * yr).sum((0, 2, 3)).numpy(), rtol=1e-4)


# ---- the objective, the language-reward head and the optimizers at their launch edges (tests/test_gpu_objective.py,
# tests/test_gpu_langrew_edges.py, tests/test_gpu_optim_steps.py; the head's older tests in tests/test_gpu_lang.py share the references) ----
GUARD_BYTES = 256
GUARD_PATTERN = 0xA5


def guarded_bytes(nbytes):
    """a device byte buffer of nbytes + a 256-byte guard holding a byte pattern: hand the kernel `nbytes` and check the guard afterwards"""
    buf = torch.empty(nbytes + GUARD_BYTES, dtype=torch.uint8, device=DEV)
    buf[nbytes:] = GUARD_PATTERN
    return buf


def assert_guard_intact(buf, nbytes, what):
    g = buf[nbytes:].cpu()
    bad = torch.nonzero(g != GUARD_PATTERN).flatten()
    assert g.numel() == GUARD_BYTES and bad.numel() == 0, f"{what}: {bad.numel()} guard bytes behind the {nbytes}-byte workspace were overwritten (first at +{bad[:4].tolist()})"


def infonce_torch(scores, mask):
    """trainer.py:95-110 on a [15,B] score table in the batched row order (pos1-3, in-clip negs 1-3, then k-major permuted negs)."""
    eps = 1e-8
    tot = 0
    for j in range(3):
        pos = scores[j]
        negs = torch.stack([scores[3 + j]] + [scores[6 + 3 * k + j] for k in range(3)], -1)
        tot = tot - torch.log(eps + (torch.exp(pos) / (eps + torch.exp(pos) + torch.exp(negs).sum(-1))))
    return ((tot / 3) * mask).mean()


def langrew_layers(D, H, LD, seed=0):
    """the five Linear layers of the head (models_language.py:43-51), fp32, drawn from `seed`"""
    import torch.nn as nn
    K1 = 2 * D + LD
    layers = [nn.Linear(K1, H), nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, 1)]
    torch.manual_seed(seed)
    for l in layers:
        nn.init.uniform_(l.weight, -1.0 / np.sqrt(l.in_features), 1.0 / np.sqrt(l.in_features))
        nn.init.uniform_(l.bias, -0.1, 0.1)
    return layers


def langrew_scores_call_by_call(layers, alle, feats, perm):
    """[15,B] scores of the reference's 15 get_reward calls (trainer.py:72-92), a torch MLP evaluated call by call
    (models_language.py:43-55) in the dtype of `layers` / `alle` / `feats`"""
    def G(a, b):
        x = torch.cat([a, b, feats], -1)
        for l in layers[:-1]:
            x = torch.relu(l(x))
        return layers[-1](x).squeeze(-1)

    e0, eg, es0, es1, es2 = [alle[:, i] for i in range(5)]
    sc = [G(e0, eg), G(e0, es1), G(e0, es2), G(e0, e0), G(e0, es0), G(e0, es1)]
    for k in range(3):
        for j, other in enumerate((eg, es1, es2)):
            p = perm[3 * k + j]
            sc.append(G(e0[p], other[p]))
    return torch.stack(sc)


LANG_BFRAME = [1, 3, 4, 0, 2, 3] + [1, 3, 4] * 3      # frame role of the second image of call q (csrc/lang.hip lang_bframe)


def langrew_bf16_model(wb, alle0, feats, perm, wts):
    """float64 MLP with a bf16 rounding exactly where the bf16 head stores bf16 (input rows, weights, the GEMM result and every hidden
    activation; straight-through in the backward pass). wb: [(weight, bias)] x 5 float64 leaf tensors requiring grad; alle0 [B,5,D],
    feats [B,LD], wts [15,B] on the CPU. Returns (scores [15,B] float64, d/d alle, flat parameter gradients) of sum(scores * wts)."""
    def r16(t):
        return t + (t.to(torch.bfloat16).to(torch.float64) - t).detach()
    B = alle0.shape[0]
    a64 = alle0.double().clone().requires_grad_(True)
    rows = []
    for q in range(15):
        src = torch.arange(B) if q < 6 else perm[q - 6].cpu().long()
        rows.append(torch.cat([a64[src, 0], a64[src, LANG_BFRAME[q]], feats.cpu().double()], dim=1))
    x = r16(torch.cat(rows, dim=0))
    for (w, b) in wb[:4]:
        x = r16(torch.relu(r16(x @ r16(w).T) + b))
    s_model = (x @ wb[4][0].T + wb[4][1]).reshape(15, B)
    (s_model * wts.cpu().double()).sum().backward()
    g_model = torch.cat([t.grad.reshape(-1) for (w, b) in wb for t in (w, b)])
    return s_model.detach(), a64.grad, g_model


def assert_edge_figures(what, got, wit, ceil, witnessed=()):
    """got / wit: {name: error of the GPU result / of the same oracle evaluated in float32 on the CPU}, both against float64; ceil:
    {name: ceiling}. Every figure is printed before anything is asserted. A figure at or over its ceiling passes only when (what, name) is
    listed in `witnessed` (the caller's docstring carries its measured figures) AND it is within 4 x the float32 oracle's own error."""
    import pytest
    fails = []
    for k, e in got.items():
        w, c = wit.get(k, float("nan")), ceil[k]
        over = not e < c
        print(f"EDGE {what} | {k}: gpu {e:.3e} cpu-fp32 {w:.3e} ceiling {c:.0e}" + (" OVER" if over else ""), flush=True)
        if over and not ((what, k) in witnessed and e <= 4.0 * w):
            fails.append(f"{k}: {e:.3e} against the ceiling {c:.0e} (float32 oracle on the CPU: {w:.3e})")
    if fails:
        pytest.fail(f"{what}: " + "; ".join(fails))


# ---- the general stem kernels at their launch edges (tests/test_gpu_stem_edges.py on the GPU, tests/test_stem_cases.py for the case
# list on the CPU; section 1 of tests/test_gpu_resolution.py draws its inputs from stem_inputs) --------------------------------------------
# r3m_stem_gen_prep / _fwd / _wgrad / _input_grad (csrc/stem_gen.hip) element by element against float64 F.conv2d on the operands the
# kernel multiplies. Ceilings: the ones check_conv_fp32 / check_conv_bf16 / assert_close_store use for the same stores.
STEM_TILE = 256              # output pixels of one forward tile: csrc/stem_gen.hip stem_fwd_gen_kernel `m0 = blk * 256`
STEM_FWD_BLOCKS = 512        # most forward blocks: csrc/stem_gen.hip launch_stem_fwd_gen `grid = ntiles < 512 ? ntiles : 512`
STEM_WG_BLOCKS = 512         # most weight-gradient blocks: csrc/stem_dev.h `#define R3M_STEM_WG_BLOCKS 512` (launch_stem_wgrad_gen `nb`)
STEM_MEAN = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64).view(1, 3, 1, 1)
STEM_STD = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64).view(1, 3, 1, 1)

# (F, H, W): the smallest shapes at which each condition of STEM_CONDITIONS occurs (tests/test_stem_cases.py recomputes them)
STEM_EDGE_CASES = [
    (1, 32, 32), (2, 32, 32),                    # the minimum size: Ho Wo = 256, a tile is a frame, nothing straddles
    (17, 32, 34),                                # Ho Wo = 272: the frame boundaries fall at every multiple of 16 of a tile
    (2, 34, 32),                                 # a last tile of 32 live pixels behind a straddling tile
    (3, 33, 35),                                 # odd H and W, Wo = 18, 2 of 4 tiles straddle, the last tile holds 150 pixels
    (3, 65, 63), (2, 63, 129), (2, 64, 66),      # Wo = 32, 65, 33: 1, 3, 2 input-gradient M tiles; W: 1, 3, 2 trips of the col2im lane loop
    (1, 32, 64),                                 # W = 64: exactly one full trip of the lane loop
    (27, 37, 32),                                # F Ho = 513 weight-gradient rows: one block takes a second row
    (33, 32, 32),                                # 528 weight-gradient rows, no forward straddle
    (33, 128, 128),                              # 528 forward tiles, no straddle: the forward's second trip
    (35, 126, 125),                              # 543 tiles, 34 straddle, last tile 163 pixels, 2205 weight-gradient rows
    (2, 32, 503),                                # the forward's largest LDS footprint (136 KiB), with a straddling tile
    (2, 37, 512), (2, 512, 37),                  # the widest staged row (Wo = 256: a tile is one row) and its transpose (F Ho = 512)
    (1, 511, 509),                               # Wo = 255: tiles drift a pixel per row; odd H: invalid waves in the last parity group
]


def stem_case_id(c):
    return "F{}_{}x{}".format(*c)


def stem_case_props(F_, H, W):
    """what the launchers and kernels of csrc/stem_gen.hip can tell apart about F frames of H x W, from (F, H, W) alone"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    HWo = Ho * Wo
    M = F_ * HWo
    ntiles = (M + STEM_TILE - 1) // STEM_TILE
    first = [t * STEM_TILE // HWo for t in range(ntiles)]
    last = [min(t * STEM_TILE + STEM_TILE - 1, M - 1) // HWo for t in range(ntiles)]
    straddling = [t for t in range(ntiles) if first[t] != last[t]]
    assert all(last[t] - first[t] <= 1 for t in range(ntiles))            # Ho Wo >= 256: at most two frames per tile
    rows_p = ((H + 1) // 2, H // 2)                                        # input rows of parity 0 / 1
    groups = (rows_p[0] + 3) // 4                                          # launch_stem_input_grad_gen: blocks per (frame, parity)
    return dict(
        Ho=Ho, Wo=Wo, M=M, ntiles=ntiles, straddling=len(straddling), last_fill=M - (ntiles - 1) * STEM_TILE,
        straddle_phases=sorted({(f * HWo) % STEM_TILE for f in range(1, F_)}),          # where in its tile a frame starts
        second_trip_straddles=any(t >= STEM_FWD_BLOCKS for t in straddling),
        rows_per_tile_max=(Wo + STEM_TILE - 2) // Wo + 1,
        wg_rows=F_ * Ho, wo_odd=Wo % 2 == 1,
        m_tiles=(Wo + 31) // 32, m_tail=Wo % 32, lane_trips=(W + 63) // 64, lane_tail=W % 64,
        dgrad_groups=groups, invalid_waves=tuple(4 * groups - r for r in rows_p))


# condition -> predicate over (F, H, W, stem_case_props): the edges the case list is there for; every one must hold for some case
STEM_CONDITIONS = {
    "one frame, a tile is the frame": lambda F_, H, W, p: F_ == 1 and p["M"] == STEM_TILE,
    "frames of exactly one tile: no straddle": lambda F_, H, W, p: F_ > 1 and p["Ho"] * p["Wo"] == STEM_TILE and p["straddling"] == 0,
    "frame starts at every multiple of 16 of a tile": lambda F_, H, W, p: p["straddle_phases"] == list(range(0, 256, 16)),
    "last tile of 32 live pixels with a straddling tile": lambda F_, H, W, p: p["last_fill"] == 32 and p["straddling"] >= 1,
    "odd H and odd W with straddling tiles": lambda F_, H, W, p: H % 2 == 1 and W % 2 == 1 and p["straddling"] >= 2,
    "partial last tile that is no multiple of a wave": lambda F_, H, W, p: p["last_fill"] % 64 != 0 and p["last_fill"] % 32 != 0,
    "one full input-gradient M tile": lambda F_, H, W, p: p["m_tiles"] == 1 and p["m_tail"] == 0,
    "two M tiles, a tail of one": lambda F_, H, W, p: p["m_tiles"] == 2 and p["m_tail"] == 1,
    "three M tiles, a tail of one": lambda F_, H, W, p: p["m_tiles"] == 3 and p["m_tail"] == 1,
    "lane loop: one trip with idle lanes": lambda F_, H, W, p: p["lane_trips"] == 1 and p["lane_tail"] != 0,
    "lane loop: exactly one full trip": lambda F_, H, W, p: W == 64,
    "lane loop: two trips": lambda F_, H, W, p: p["lane_trips"] == 2 and p["lane_tail"] != 0,
    "lane loop: three trips": lambda F_, H, W, p: p["lane_trips"] == 3 and p["lane_tail"] != 0,
    "odd Wo: the weight gradient pads to Wo2": lambda F_, H, W, p: p["wo_odd"] and p["Wo"] > 1,
    "even Wo": lambda F_, H, W, p: not p["wo_odd"],
    "weight gradient: exactly one block takes a second row": lambda F_, H, W, p: p["wg_rows"] == STEM_WG_BLOCKS + 1,
    "weight gradient: exactly as many rows as blocks": lambda F_, H, W, p: p["wg_rows"] == STEM_WG_BLOCKS,
    "weight gradient second trip, forward without straddle or second trip":
        lambda F_, H, W, p: p["wg_rows"] > STEM_WG_BLOCKS and p["straddling"] == 0 and p["ntiles"] <= STEM_FWD_BLOCKS,
    "weight gradient second trip with straddling frames": lambda F_, H, W, p: p["wg_rows"] > STEM_WG_BLOCKS and p["straddling"] > 0,
    "forward second trip without straddle": lambda F_, H, W, p: p["ntiles"] > STEM_FWD_BLOCKS and p["straddling"] == 0,
    "forward second trip with a straddling tile in it": lambda F_, H, W, p: p["ntiles"] > STEM_FWD_BLOCKS and p["second_trip_straddles"],
    "a tile is exactly one output row (W = 512)": lambda F_, H, W, p: p["Wo"] == STEM_TILE and W == 512,
    "64 input-gradient groups per parity, H even": lambda F_, H, W, p: p["dgrad_groups"] == 64 and H % 2 == 0,
    "tiles drift one pixel per row": lambda F_, H, W, p: p["Wo"] == STEM_TILE - 1,
    "odd H: an invalid wave in the last group of one parity only": lambda F_, H, W, p: H % 2 == 1 and p["invalid_waves"] == (0, 1),
    "sixteen output rows per tile": lambda F_, H, W, p: p["Wo"] == 16,
    "H != W both ways": lambda F_, H, W, p: H != W,
}


def stem_inputs(F_, H, W, seed):
    """integer frames 0..255 [F,3,H,W], conv1 weights OHWI randn * 0.1, dY randn [F,Ho,Wo,64]"""
    g = torch.Generator().manual_seed(seed)
    x = torch.floor(torch.rand(F_, 3, H, W, generator=g) * 256).clamp(0, 255)
    w = torch.randn(64, 7, 7, 3, generator=g) * 0.1                     # OHWI
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(F_, Ho, Wo, 64, generator=g)
    return x, w, dy, Ho, Wo


def stem_edge_setup(case, dtype):
    """the inputs of a case and the float64 operands the kernels multiply: the normalised image (bf16: rounded once), the weights OIHW
    (bf16: rounded; `w_master`: the fp32 master the input gradient multiplies), dY NCHW (bf16: rounded)"""
    F_, H, W = case
    x, w, dy, Ho, Wo = stem_inputs(F_, H, W, 1000 * H + W + F_)
    xn32 = (x / 255.0 - STEM_MEAN.float()) / STEM_STD.float()          # fp32, the arithmetic of stem_normalize
    q = (lambda t: t.to(torch.bfloat16)) if dtype == "bf16" else (lambda t: t)
    return dict(F=F_, H=H, W=W, Ho=Ho, Wo=Wo, dt=1 if dtype == "bf16" else 0, tdt=torch.bfloat16 if dtype == "bf16" else torch.float32,
                x=x, w=w, dy=dy, xn32=xn32, xn=q(xn32).double(), w_op=q(w).double().permute(0, 3, 1, 2).contiguous(),
                w_master=w.double().permute(0, 3, 1, 2).contiguous(), dy_op=q(dy).double().permute(0, 3, 1, 2).contiguous())


def _scalar(v):
    return torch.as_tensor(float(v), dtype=torch.float64)


def stem_gen_prep_dev(hip, s):
    """r3m_stem_gen_prep into a NaN-filled (all-ones bytes) image; returns the device byte buffer"""
    nbytes = hip.r3m_stem_gen_image_bytes(s["F"], s["H"], s["W"], s["dt"])
    assert nbytes == s["F"] * s["H"] * s["W"] * 3 * (2 if s["dt"] else 4)
    xn = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)     # 0xFFFF / 0xFFFFFFFF: a NaN in either type
    xd = s["x"].to(DEV).contiguous()
    assert hip.r3m_stem_gen_prep(xd.data_ptr(), xn.data_ptr(), s["F"], s["H"], s["W"], s["dt"], _st()) == 0, hip.r3m_last_error()
    return xn


def _stem_frames(F_):
    return sorted({0, F_ // 2, F_ - 1})


def check_stem_gen_prep(hip, case, dtype):
    """the pre-pass: xn[f][iy][ix * 3 + c] (the layout csrc/stem_gen.hip stem_prep_gen_kernel writes, r3m_stem_gen_image_bytes long) is
    bit for bit torch CPU fp32 (x / 255 - mean) / std, for bf16 that value rounded once"""
    s = stem_edge_setup(case, dtype)
    xn = stem_gen_prep_dev(hip, s)
    got = xn.view(s["tdt"]).view(s["F"], s["H"], s["W"], 3).cpu()
    want = nhwc(s["xn32"]).to(s["tdt"])
    assert bool(torch.isfinite(got.float()).all()), f"stem prep {dtype} {case}: an element was not written"
    diff = int((got.view(torch.int16 if s["dt"] else torch.int32) != want.view(torch.int16 if s["dt"] else torch.int32)).sum())
    print(f"stem prep {dtype} {case}: {diff} of {want.numel()} elements differ in their bits")
    assert diff == 0


def check_stem_gen_forward(hip, case, dtype):
    """r3m_stem_gen_fwd with and without statistics under assert_close_store's ceilings, the BatchNorm partials per 256-pixel tile, and
    frames 0 / middle / last bit-identical to 1-frame calls (a pixel's MFMA sums do not depend on where its tile starts)."""
    import pytest
    s = stem_edge_setup(case, dtype)
    F_, H, W, Ho, Wo, dt, tdt = (s[k] for k in ("F", "H", "W", "Ho", "Wo", "dt", "tdt"))
    y_ref = F.conv2d(s["xn"], s["w_op"], stride=2, padding=3)
    what = f"stem forward {dtype} {case}"
    assert_range(y_ref, [_scalar(s["xn"].abs().max() * s["w_op"].abs().max())], what)
    xn = stem_gen_prep_dev(hip, s)
    wd = s["w"].to(DEV).contiguous()
    M = F_ * Ho * Wo
    nt = (M + STEM_TILE - 1) // STEM_TILE

    def launch(xn_, frames, with_stats):
        y = torch.full((frames, Ho, Wo, 64), float("nan"), dtype=tdt, device=DEV)
        st_ = torch.full(((frames * Ho * Wo + STEM_TILE - 1) // STEM_TILE, 2, 64), float("nan"), device=DEV) if with_stats else None
        rc = hip.r3m_stem_gen_fwd(xn_.data_ptr(), wd.data_ptr(), y.data_ptr(), None if st_ is None else st_.data_ptr(), frames, H, W, dt, _st())
        assert rc == 0, hip.r3m_last_error()
        return y, st_

    y, stats = launch(xn, F_, True)
    y0, _ = launch(xn, F_, False)
    assert_close_store(what + " (statistics)", nchw(y.float().cpu()), y_ref, dtype)
    assert_close_store(what + " (stats = NULL)", nchw(y0.float().cpu()), y_ref, dtype)
    # BatchNorm partials, tile by tile. gg_stats (csrc/conv_dev.h) sums the fp32 ACCUMULATORS, before the store rounds them: for bf16 too
    # the reference is the unrounded float64 result. Pixels past M were cleared after the K loop and add nothing.
    yy = torch.zeros(nt * STEM_TILE, 64, dtype=torch.float64)
    yy[:M] = nhwc(y_ref).reshape(M, 64)
    yy = yy.view(nt, STEM_TILE, 64)
    r1, a1, r2 = yy.sum(1), yy.abs().sum(1), (yy * yy).sum(1)
    got = stats.double().cpu()
    assert tuple(got.shape) == (nt, 2, 64)
    e1, e2 = (got[:, 0] - r1).abs() / a1, (got[:, 1] - r2).abs() / r2
    e1[~torch.isfinite(e1)] = float("inf")
    e2[~torch.isfinite(e2)] = float("inf")
    print(f"{what}: statistics per tile, worst |s1 - sum y| / sum|y| {float(e1.max()):.3e}, |s2 - sum y^2| / sum y^2 {float(e2.max()):.3e} "
          f"({nt} tiles, last holds {M - (nt - 1) * STEM_TILE} pixels)")
    bad = torch.nonzero(((e1 > 1e-4) | (e2 > 1e-4)).any(1)).flatten()
    if bad.numel():
        pytest.fail(f"{what}: the statistics of {bad.numel()} of {nt} tiles are off (first {bad[:8].tolist()}, last {bad[-3:].tolist()}): worst "
                    f"s1 {float(e1.max()):.3e} s2 {float(e2.max()):.3e} against 1e-4")
    # frame independence, exact
    if F_ > 1:
        fb = H * W * 3 * (2 if dt else 4)
        for f in _stem_frames(F_):
            y1, _ = launch(xn[f * fb:(f + 1) * fb].clone(), 1, True)
            if not torch.equal(y1[0], y[f]):
                pytest.fail(f"{what}: frame {f} of the {F_}-frame call differs from a 1-frame call on its data: "
                            + describe_bad(y[f].float().cpu(), y1[0].float().cpu(), 0.0))
        print(f"{what}: frames {_stem_frames(F_)} bit-identical to 1-frame calls")


def check_stem_gen_wgrad(hip, case, dtype):
    """r3m_stem_gen_wgrad with accumulate 0 into NaN, then accumulate 1 on top: max-rel < 5e-5 of the range against 1 x and 2 x float64"""
    s = stem_edge_setup(case, dtype)
    F_, H, W, dt, tdt = (s[k] for k in ("F", "H", "W", "dt", "tdt"))
    wr = s["w_op"].clone().requires_grad_(True)
    F.conv2d(s["xn"], wr, stride=2, padding=3).backward(s["dy_op"])
    dw_ref = wr.grad                                                    # OIHW
    what = f"stem weight gradient {dtype} {case}"
    assert_range(dw_ref, [_scalar(s["xn"].abs().max() * s["dy_op"].abs().max())], what)
    xn = stem_gen_prep_dev(hip, s)
    dyd = s["dy"].to(tdt).to(DEV).contiguous()
    dw = torch.full((64, 7, 7, 3), float("nan"), device=DEV)
    wsb = hip.r3m_stem_gen_wgrad_ws_bytes()
    ws = guarded_bytes(wsb)
    for acc in (0, 1):
        rc = hip.r3m_stem_gen_wgrad(xn.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ws.data_ptr(), F_, H, W, acc, dt, _st())
        assert rc == 0, hip.r3m_last_error()
        e_max, e_l2 = rel_err(dw.cpu().permute(0, 3, 1, 2).numpy(), (acc + 1) * dw_ref.numpy())
        print(f"{what} accumulate {acc}: max-rel {e_max:.3e} l2-rel {e_l2:.3e}")
        assert e_max < 5e-5, f"{what} accumulate {acc}: max-rel {e_max}"
    assert_guard_intact(ws, wsb, what)


def check_stem_gen_input_grad(hip, case, dtype):
    """r3m_stem_gen_input_grad (fp32 NCHW output for both dtypes): accumulate 0 into NaN and accumulate 1 onto a base that is non-zero
    everywhere, max-rel < 2e-5 of the range, every element finite, frames 0 / middle / last bit-identical to 1-frame calls"""
    import pytest
    s = stem_edge_setup(case, dtype)
    F_, H, W, Ho, Wo, dt, tdt = (s[k] for k in ("F", "H", "W", "Ho", "Wo", "dt", "tdt"))
    # (bf16) dZ against the fp32 master weights, then d(normalised) / d(frame value) = 1 / (255 std)
    dx_ref = torch.nn.grad.conv2d_input((F_, 3, H, W), s["w_master"], s["dy_op"], stride=2, padding=3) / (255.0 * STEM_STD)
    what = f"stem input gradient {dtype} {case}"
    top = _scalar(s["dy_op"].abs().max() * s["w_master"].abs().max() / (255.0 * float(STEM_STD.min())))
    assert_range(dx_ref, [top], what)
    sd = float(dx_ref.pow(2).mean().sqrt())
    base = rnd((F_, 3, H, W), 31, 0.25, 1.0) * torch.where(rnd((F_, 3, H, W), 32) > 0, 1.0, -1.0) * sd
    assert bool((base != 0).all()), f"{what}: the base must be non-zero everywhere"
    ref_acc = dx_ref + base.double()
    assert_range(ref_acc, [dx_ref, base], what + " accumulate")
    dyd = s["dy"].to(tdt).to(DEV).contiguous()
    wd = s["w"].to(DEV).contiguous()

    def launch(dz, frames, old):
        dx = torch.full((frames, 3, H, W), float("nan"), device=DEV) if old is None else old.to(DEV).contiguous()
        rc = hip.r3m_stem_gen_input_grad(dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), frames, H, W, 0 if old is None else 1, dt, _st())
        assert rc == 0, hip.r3m_last_error()
        return dx

    dx = launch(dyd, F_, None)
    dxa = launch(dyd, F_, base)
    for name, got, ref in (("accumulate 0", dx, dx_ref), ("accumulate 1", dxa, ref_acc)):
        g = got.cpu()
        assert bool(torch.isfinite(g).all()), f"{what} {name}: {int((~torch.isfinite(g)).sum())} elements of [F,3,H,W] are not finite"
        e_max, e_l2 = rel_err(g.numpy(), ref.numpy())
        print(f"{what} {name}: max-rel {e_max:.3e} l2-rel {e_l2:.3e}")
        if not e_max < 2e-5:
            d = (g.double() - ref).abs() > 2e-5 * float(ref.abs().max())
            rows = torch.nonzero(d.any(3).any(1).any(0)).flatten()
            cols = torch.nonzero(d.any(2).any(1).any(0)).flatten()
            pytest.fail(f"{what} {name}: max-rel {e_max}; {int(d.sum())} elements off in {len(rows)} rows (first {rows[:6].tolist()}, last "
                        f"{rows[-3:].tolist()}) and {len(cols)} columns (first {cols[:6].tolist()}, last {cols[-3:].tolist()})")
    if F_ > 1:
        for f in _stem_frames(F_):
            one = launch(dyd[f:f + 1].contiguous(), 1, None)
            assert torch.equal(one[0], dx[f]), f"{what}: frame {f} of the {F_}-frame call differs from a 1-frame call on its data"
        print(f"{what}: frames {_stem_frames(F_)} bit-identical to 1-frame calls")
