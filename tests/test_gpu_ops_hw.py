"""-m gpu: the layer kernels one by one on feature maps whose height and width DIFFER, through the C ABI, against float64 on the CPU.

The square operator tests (test_gpu_ops.py, test_gpu_bf16.py, test_gpu_fuzz.py) pass the same number for Hi and Wi, so a kernel that
reads the wrong one of the two passes them; the encoder-level tests at H != W (test_gpu_resolution.py) have gates wide enough for
ReLU / max-pool decision flips. Here every kernel condition that treats the two extents differently gets a case on each side, with
the tolerances of the square tests (tests/util.py holds the shared bodies): the arithmetic per output element is the same sum of
k k Ci products whatever the map's shape.

The case lists are plain module constants (building them needs the library's host-only plan queries, not a GPU):
tests/test_dispatch.py::test_every_engine_route_at_non_square_sizes_has_an_operator_case checks on the CPU that every dispatch
signature the engine can reach at a supported non-square frame size is run by one of them.

The lists are built when the module is imported, through the library's plan queries: a missing or stale library shows as an import
error here and in that CPU test (every other CPU test needs the library too).

profiles/r07_ops_hw_mutants.txt: the mutation check. Three mutants that read Hi for Wi in one place each, one per kernel family, are
described there with the reason each stays in bounds. RUN so far: the wgrad_win.hip padding-mask cursor (passes the square convolution
lists, fails test_conv_fwd_dgrad_wgrad_hw by a wrong value). NOT RUN: the conv_pw.hip tap row stride and the conv.hip window kernel row
decode. Two mutants of host-side eligibility conditions change no value and fail the pinned routes of tests/test_dispatch.py on the
CPU. Run times are in the same file."""
import pytest
import torch
import torch.nn.functional as F

from r3m_amd import _lib
from route_sig import plan_convs
from util import DEV, EPS_BF16, check_conv_bf16, check_conv_fp32, check_dgrad_bnred, check_stem_tail_fused_vs_torch, nchw, nhwc, q_bf16, rel_err, rnd

pytestmark = pytest.mark.gpu

BF16 = 1


def st():
    return torch.cuda.current_stream().cuda_stream


def _plan_cases(sizes, frames, N, keep=lambda c: True):
    """distinct (N, Hi, Wi, Ci, Co, k, s, p) of the convolutions behind the stem of the given ResNets at the given frame sizes, from the
    engine's own plan table (r3m_resnet_conv_info), so the list cannot drift from the engine"""
    L = _lib.lib()
    out = []
    for size in sizes:
        for (H, W) in frames:
            h = L.r3m_resnet_create_hw(size, N, 0, H, W)
            assert h, L.r3m_last_error()
            try:
                for (Ci, Co, k, s, p, Hi, Wi, Ho, Wo) in plan_convs(L, h)[1:]:
                    c = (N, Hi, Wi, Ci, Co, k, s, p)
                    if keep(c) and c not in out:
                        out.append(c)
            finally:
                L.r3m_resnet_destroy(h)
    return out


# ---- (N, Hi, Wi, Ci, Co, k, stride, pad), by the kernel condition each group is there for ----------------------------------------------
HW_CONV_GROUPS = {
    # stride-2 3x3 input gradients whose four parity launches run on TWO kernel families (conv_pw.hip pw_gemm_form: Wg < 4 || Hg < 2
    # per parity class): routes (13, 13, 21, 21) when the height is short, (13, 21, 13, 21) when the width is. No square map does this.
    "mixed_dgrad": [(3, 3, 32, 256, 512, 3, 2, 1), (3, 32, 3, 256, 512, 3, 2, 1), (3, 9, 7, 128, 256, 3, 2, 1), (3, 7, 9, 128, 256, 3, 2, 1),
                    (3, 16, 7, 256, 512, 3, 2, 1), (3, 16, 7, 128, 256, 3, 2, 1), (3, 3, 32, 512, 512, 3, 2, 1)],
    # the maps the engine really makes: every layer geometry of ResNet-18 / -50 at two wide, two tall frame sizes (one of each with
    # odd extents at every level: 25 x 33, 13 x 17, 7 x 9, 4 x 5)
    "real_maps": _plan_cases((18, 50), [(96, 160), (160, 96), (97, 131), (131, 97)], 3),
    # extremes of the supported range, layers 3 / 4 of 96 x 512, 512 x 96 (6 x 32, 32 x 6, 3 x 16, 16 x 3) and 33 x 512, 512 x 33 frames
    # (3 x 32, 32 x 3, 2 x 16, 16 x 2): the window kernel on 32-row 6-column maps, off it on 6-row 32-column ones; maps lower than 2 or
    # narrower than 4 after the stride leave the persistent kernel for the 16-wide-K / gather kernels with 512..2048 channels
    "extremes": _plan_cases((18, 50), [(96, 512), (512, 96), (33, 512), (512, 33)], 1, keep=lambda c: c[1] * c[2] <= 192),
    # one-pixel-wide and one-pixel-high maps (the ABI takes them), 3x3 and 1x1
    "one_pixel": [(2, 1, 9, 128, 128, 3, 1, 1), (2, 9, 1, 128, 128, 3, 1, 1), (2, 1, 9, 64, 64, 3, 1, 1), (2, 9, 1, 64, 64, 3, 1, 1),
                  (2, 1, 12, 256, 512, 1, 1, 0), (2, 12, 1, 512, 256, 1, 1, 0), (2, 1, 12, 128, 256, 3, 2, 1), (2, 12, 1, 128, 256, 3, 2, 1)],
    # conv.hip conv3x3_win_eligible: Wi <= 28 and nothing of Hi -- each side of the threshold with a height on the other side of it
    "window_width": [(2, 40, 28, 128, 128, 3, 1, 1), (2, 40, 29, 128, 128, 3, 1, 1), (2, 6, 28, 128, 128, 3, 1, 1),
                     (2, 6, 29, 128, 128, 3, 1, 1)],
    # conv_pw.hip pw_gemm_form: Wg < 4 || Hg < 2 (gather form: 64-wide 3x3 / stride 1, forwards of stride 2) -- Wg 3 / 4 with Hg 9,
    # Hg 1 / 2 with Wg 9
    "persistent_extent": [(2, 9, 3, 64, 64, 3, 1, 1), (2, 9, 4, 64, 64, 3, 1, 1), (2, 2, 9, 64, 64, 3, 1, 1),
                          (2, 17, 5, 128, 256, 3, 2, 1), (2, 17, 7, 128, 256, 3, 2, 1), (2, 1, 17, 128, 256, 3, 2, 1),
                          (2, 3, 17, 128, 256, 3, 2, 1)],
    # wgrad_win.hip: Wo < 2 leaves the shared-window weight gradient (Wo = 1: the 9 x 1 maps of one_pixel; Wo = 2 here); row segments per
    # 32-row K step depend on the width only (33 x 5: seven segments per step, 5 x 33: steps without a row start)
    "wgrad_window_width": [(2, 9, 2, 128, 128, 3, 1, 1), (2, 9, 2, 64, 64, 3, 1, 1), (3, 33, 5, 64, 128, 3, 1, 1), (3, 5, 33, 64, 128, 3, 1, 1)],
    # stride 2 with (odd, even), (even, odd), (odd, odd) extents, 3x3 and 1x1: the four parity classes of the input gradient have four
    # different (Hg, Wg); a strided 1x1 leaves pixels without taps (checked to be exact zeros)
    "stride2_parity": [(2, 13, 10, 128, 128, 3, 2, 1), (2, 10, 13, 128, 128, 3, 2, 1), (2, 13, 11, 128, 128, 3, 2, 1),
                       (2, 13, 10, 128, 256, 1, 2, 0), (2, 10, 13, 128, 256, 1, 2, 0), (2, 13, 11, 128, 256, 1, 2, 0),
                       (2, 11, 20, 64, 128, 3, 2, 1), (2, 20, 11, 64, 128, 1, 2, 0)],
    # persistent kernel with more tiles than workers (512 four-wave blocks) and a partial last tile, one wide and one tall map: the M of
    # the square list's N = 23 and N = 90 cases at 56 x 56 on maps half as large
    "many_tiles": [(46, 28, 56, 64, 128, 1, 1, 0), (180, 56, 28, 128, 128, 3, 2, 1)],
}
HW_CONV_CASES = list(dict.fromkeys(c for g in HW_CONV_GROUPS.values() for c in g))

_ALL = ("recompute", "bits", "bits+residual")
# ---- dgrad + BatchNorm-backward partials: (case, modes) ------------------------------------------------------------------------------
HW_BNRED_GROUPS = {
    # 3x3 / stride 1 on the window kernel, a wide and a tall map (fp32; bf16: kernel-row kernel)
    "window": [((2, 10, 24, 128, 128, 3, 1, 1), _ALL), ((2, 24, 10, 128, 128, 3, 1, 1), _ALL), ((3, 4, 5, 512, 512, 3, 1, 1), _ALL),
               ((3, 16, 2, 512, 512, 3, 1, 1), _ALL)],
    # ... on the persistent kernel's gather form (64-wide)
    "gather_form": [((3, 24, 40, 64, 64, 3, 1, 1), _ALL), ((3, 40, 24, 64, 64, 3, 1, 1), _ALL)],
    # stride 2 with an odd extent: four parity launches appending their partial rows (r3m_conv2d_dgrad_bnred_rows(N, Hi, Wi, 2))
    "stride2_odd": [((2, 13, 10, 128, 128, 3, 2, 1), _ALL), ((2, 10, 13, 128, 128, 3, 2, 1), _ALL), ((3, 25, 33, 128, 128, 3, 2, 1), _ALL),
                    ((3, 20, 12, 256, 256, 3, 2, 1), _ALL)],
    # pointwise
    "pointwise": [((3, 6, 10, 1024, 256, 1, 1, 0), _ALL), ((3, 40, 24, 256, 64, 1, 1, 0), _ALL), ((3, 3, 5, 512, 2048, 1, 1, 0), _ALL),
                  ((3, 5, 3, 2048, 512, 1, 1, 0), _ALL), ((3, 24, 40, 64, 256, 1, 1, 0), _ALL), ((3, 24, 40, 256, 64, 1, 1, 0), _ALL)],
    # 3x3 / stride 1 wider than the window kernel allows: the masked residual join + partials run the gather kernel (route 21), an
    # epilogue the square list only runs on the window kernel
    "wide_join": [((3, 3, 32, 256, 256, 3, 1, 1), _ALL), ((3, 6, 32, 256, 256, 3, 1, 1), _ALL), ((3, 32, 6, 256, 256, 3, 1, 1), _ALL)],
    # the mixed-family stride-2 input gradients, mask recomputed (the form the strided-output kernel admits)
    "mixed_dgrad": [(c, ("recompute",)) for c in HW_CONV_GROUPS["mixed_dgrad"]] + [((3, 32, 3, 512, 512, 3, 2, 1), ("recompute",))],
}
HW_BNRED_CASES = [(c, mode, dtype) for g in HW_BNRED_GROUPS.values() for (c, modes) in g for mode in modes for dtype in ("fp32", "bf16")]

# ---- bf16 ----------------------------------------------------------------------------------------------------------------------------
HW_BF16_GROUPS = {
    "real_maps": [c for c in HW_CONV_GROUPS["real_maps"] if c[3] % 64 == 0 and c[4] % 64 == 0],
    "extremes": [c for c in HW_CONV_GROUPS["extremes"] if c[3] % 64 == 0 and c[4] % 64 == 0],
    "mixed_dgrad": HW_CONV_GROUPS["mixed_dgrad"][:4],
    # wgrad_bf16.hip all-taps weight gradient: (Wi & 7) == 0 && Wi >= 8 && Hi >= 4 -- Wi in {8, 16, 24} x Hi in {3, 4, 5}, and transposed
    "wgrad_all_taps": [(2, h, w, 64, 128, 3, 1, 1) for w in (8, 16, 24) for h in (3, 4, 5)] +
                      [(2, w, h, 64, 128, 3, 1, 1) for w in (8, 16, 24) for h in (3, 4, 5)],
    # kernel-row weight gradient (128-wide): the FAST K-step path needs 32 / Wo + 1 <= Ho, i.e. Ho Wo > 32 -- symmetric in the two extents,
    # so the transposes are a second shape on the same side: off (3 x 10, 10 x 3), on (3 x 12, 12 x 3)
    "wgrad_fast_path": [(2, 3, 10, 128, 128, 3, 1, 1), (2, 10, 3, 128, 128, 3, 1, 1), (2, 3, 12, 128, 128, 3, 1, 1), (2, 12, 3, 128, 128, 3, 1, 1)],
    "stride2_parity": [c for c in HW_CONV_GROUPS["stride2_parity"]],
    # a 64-wide 3x3 / stride-1 map too wide for the kernel-row kernel's staged rows (conv_row16.hip: 2 Wi + 2): the 9 x 128 layer1 map of a
    # 33 x 512 frame runs the halo kernel (31) in the default mode; 128-wide outputs leave it from Wi = 32 on
    "row16_too_wide": [(1, 9, 128, 64, 64, 3, 1, 1), (2, 6, 40, 128, 128, 3, 1, 1), (2, 5, 56, 64, 128, 3, 1, 1)],
}
HW_BF16_CASES = list(dict.fromkeys(c for g in HW_BF16_GROUPS.values() for c in g))
# 3x3 / stride 1 on the kernel-row kernel (conv_row16.hip, eligibility by 2 Wi + 2 staged rows: 128-wide outputs up to Wi = 30) and,
# switched, on the halo kernel (conv_bf16.hip, tile choice by halo_lds_bytes(.., Wi)): wide and tall, 64- and 128-wide outputs
HW_ROW16_CASES = [(2, 6, 30, 128, 128, 3, 1, 1), (2, 30, 6, 128, 128, 3, 1, 1), (3, 24, 40, 64, 64, 3, 1, 1), (3, 40, 24, 64, 64, 3, 1, 1),
                  (2, 5, 30, 64, 128, 3, 1, 1), (2, 56, 5, 128, 64, 3, 1, 1)]


def _ids(c):
    return "N{}_{}x{}_{}to{}_k{}s{}p{}".format(*c)


@pytest.mark.parametrize("case", HW_CONV_CASES, ids=_ids)
def test_conv_fwd_dgrad_wgrad_hw(hip, case):
    check_conv_fp32(hip, case, ref64=True, strict=True)


@pytest.mark.parametrize("case,mode,dtype", HW_BNRED_CASES, ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_dgrad_epilogue_emits_bn_backward_partials_hw(hip, case, mode, dtype):
    check_dgrad_bnred(hip, case, mode, dtype)


@pytest.mark.parametrize("case", HW_BF16_CASES, ids=_ids)
def test_conv_bf16_fwd_dgrad_wgrad_hw(hip, case):
    check_conv_bf16(hip, case, strict=True)


@pytest.mark.parametrize("kernel", ["kernel_row", "halo"])
@pytest.mark.parametrize("case", HW_ROW16_CASES, ids=_ids)
def test_conv3x3_bf16_kernel_row_and_halo_kernel_hw(hip, case, kernel):
    old = hip.r3m_debug_set_conv3x3_bf16(1 if kernel == "kernel_row" else 0)
    try:
        check_conv_bf16(hip, case, strict=True)
    finally:
        hip.r3m_debug_set_conv3x3_bf16(old)


# ---- transpose witnesses: exact integers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("s", [1, 2])
def test_conv3x3_pixel_codes_are_exact_hw(hip, s, dtype):
    """5 x 9 map, x[n, iy, ix, c] = a small integer code of (iy, ix) on ONE channel per pixel, weights small integers different for every
    tap and channel pair: every product and sum is an integer below 2^8 (exact in bf16 and fp32), so forward, dgrad and wgrad must
    EQUAL float64. An (iy, ix) swap, a transposed tap order or a row stride taken from Hi gives different integers."""
    N, Hi, Wi, Ci, Co, k, p = 2, 5, 9, 64, 128, 3, 1
    dt = 0 if dtype == "fp32" else 1
    tdt = torch.float32 if dt == 0 else torch.bfloat16
    x = torch.zeros((N, Hi, Wi, Ci))
    for n in range(N):
        for iy in range(Hi):
            for ix in range(Wi):
                x[n, iy, ix, (7 * iy + 3 * ix + 5 * n) % Ci] = 1 + (iy * Wi + ix + n) % 3          # one channel per pixel
    co, ci, kh, kw = torch.meshgrid(torch.arange(Co), torch.arange(Ci), torch.arange(3), torch.arange(3), indexing="ij")
    w = ((kh * 3 + kw) + 2 * ((co + 3 * ci) % 2)).float() - 4.0                                     # -4..6, differs for every tap
    Ho, Wo = (Hi + 2 - 3) // s + 1, (Wi + 2 - 3) // s + 1
    oy, ox = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    dy = torch.zeros((N, Ho, Wo, Co))
    for n in range(N):
        dy[n, oy, ox, (11 * oy + 5 * ox + n) % Co] = (1 + (oy * Wo + ox + 2 * n) % 3).float()      # one channel per output pixel
    xr, wr = nchw(x).double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, stride=s, padding=p)
    y_ref.backward(nchw(dy).double())
    assert float(y_ref.detach().abs().max()) < 256 and float(xr.grad.abs().max()) < 256       # integers a bf16 holds exactly

    xd, dyd = x.to(DEV).to(tdt), dy.to(DEV).to(tdt)
    w32 = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = w32.to(tdt)
    yd = torch.full((N, Ho, Wo, Co), float("nan"), dtype=tdt, device=DEV)
    assert hip.r3m_conv2d_fwd_dt(xd.data_ptr(), wd.data_ptr(), yd.data_ptr(), None, N, Hi, Wi, Ci, Co, k, s, p, dt, st()) == 0, hip.r3m_last_error()
    torch.testing.assert_close(nchw(yd.float().cpu()).double(), y_ref.detach(), rtol=0, atol=0)
    dxd = torch.full((N, Hi, Wi, Ci), float("nan"), dtype=tdt, device=DEV)
    wsb = hip.r3m_conv2d_dgrad_workspace_bytes(Ci, Co, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    assert hip.r3m_conv2d_dgrad_dt(dyd.data_ptr(), w32.data_ptr(), dxd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, dt, st()) == 0, \
        hip.r3m_last_error()
    torch.testing.assert_close(nchw(dxd.float().cpu()).double(), xr.grad, rtol=0, atol=0)
    dwd = torch.full((Co, k, k, Ci), float("nan"), device=DEV)
    wsb = hip.r3m_conv2d_wgrad_workspace_bytes_dt(N, Hi, Wi, Ci, Co, k, s, p, dt)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    assert hip.r3m_conv2d_wgrad_dt(xd.data_ptr(), dyd.data_ptr(), dwd.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, 0, dt, st()) == 0, \
        hip.r3m_last_error()
    torch.testing.assert_close(dwd.cpu().permute(0, 3, 1, 2).double(), wr.grad, rtol=0, atol=0)


# ---- pools ----------------------------------------------------------------------------------------------------------------------------
POOL_MAPS = [(12, 9), (7, 16), (25, 33), (3, 5), (49, 66)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("H,W", POOL_MAPS)
def test_maxpool_hw(hip, H, W, dtype):
    """r3m_maxpool_fwd / _bwd[_dt] against F.max_pool2d(3, 2, 1) + autograd: tolerances of test_maxpool / test_pools_bf16"""
    N, C = 2, 64
    dt = 0 if dtype == "fp32" else 1
    tdt = torch.float32 if dt == 0 else torch.bfloat16
    qq = (lambda t: t) if dt == 0 else q_bf16
    z = qq(torch.relu(rnd((N, C, H, W), 41)))   # post-ReLU: plenty of exact-zero ties
    zr = z.double().requires_grad_(True)
    p_ref = F.max_pool2d(zr, 3, 2, 1)
    Ho, Wo = p_ref.shape[2], p_ref.shape[3]
    dp = qq(rnd(tuple(p_ref.shape), 42))
    p_ref.backward(dp.double())
    zd = nhwc(z).to(DEV).to(tdt)
    pd = torch.full((N, Ho, Wo, C), float("nan"), dtype=tdt, device=DEV)
    am = torch.full((N, Ho, Wo, C), 255, dtype=torch.uint8, device=DEV)
    assert hip.r3m_maxpool_fwd_dt(zd.data_ptr(), pd.data_ptr(), am.data_ptr(), N, H, W, C, dt, st()) == 0, hip.r3m_last_error()
    torch.testing.assert_close(nchw(pd.float().cpu()).double(), p_ref.detach(), rtol=0, atol=0)
    dzd = torch.full((N, H, W, C), float("nan"), dtype=tdt, device=DEV)
    dpd = nhwc(dp).to(DEV).to(tdt)
    assert hip.r3m_maxpool_bwd_dt(dpd.data_ptr(), am.data_ptr(), dzd.data_ptr(), N, H, W, C, dt, st()) == 0, hip.r3m_last_error()
    got = nchw(dzd.float().cpu()).double()
    assert torch.isfinite(got).all()
    # gradients may legitimately land on a different element of an all-zero (tied) window; after the ReLU mask they agree
    mask = (z > 0).double()
    tol = 1e-6 if dt == 0 else 2 * EPS_BF16
    torch.testing.assert_close(got * mask, zr.grad * mask, rtol=tol, atol=tol)
    if dt == 0:
        torch.testing.assert_close(got.sum(), zr.grad.sum(), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(12, 9), (25, 33)])
def test_stem_tail_fused_vs_torch_hw(hip, H, W, dtype):
    """r3m_bn_relu_maxpool_fwd_dt / r3m_bn_maxpool_bwd_dt (what the engine runs behind the stem) against BatchNorm + ReLU + max-pool in
    float64 with the same coefficients. The inputs are kept away from the ReLU kink, and a max-pool window never holds two different
    positive values that a rounding could reorder or that are equal: y is drawn from a grid of well separated levels, distinct inside
    every 3 x 3 window (the zeros behind the ReLU still tie), so the float64 argmax is the only argmax the kernel can pick."""
    check_stem_tail_fused_vs_torch(hip, 2, H, W, 64, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [512, 2048])
@pytest.mark.parametrize("HW", [1, 2, 15, 20, 49, 256])
def test_avgpool_hw(hip, HW, C, dtype):
    """r3m_avgpool_fwd / _bwd[_dt] for the map sizes layer4 ends in (1 = 32 x 32 frames ... 256 = 512 x 512) against float64: tolerances
    of test_avgpool (fp32) and test_pools_bf16 (bf16: forward fp32 level, backward the exact bf16 rounding of dh / HW)"""
    N = 3
    dt = 0 if dtype == "fp32" else 1
    tdt = torch.float32 if dt == 0 else torch.bfloat16
    x = rnd((N, HW, C), 51)
    x = x if dt == 0 else q_bf16(x)
    hd = torch.full((N, C), float("nan"), device=DEV)
    xd = x.to(DEV).to(tdt)
    assert hip.r3m_avgpool_fwd_dt(xd.data_ptr(), hd.data_ptr(), N, HW, C, dt, st()) == 0, hip.r3m_last_error()
    assert rel_err(hd.cpu().numpy(), x.double().mean(1).numpy())[0] < 1e-6
    dh = rnd((N, C), 52)
    dxd = torch.full((N, HW, C), float("nan"), dtype=tdt, device=DEV)
    dhd = dh.to(DEV)
    assert hip.r3m_avgpool_bwd_dt(dhd.data_ptr(), dxd.data_ptr(), N, HW, C, dt, st()) == 0, hip.r3m_last_error()
    want = (dh.double() / HW).unsqueeze(1).expand(N, HW, C)
    if dt == 0:
        torch.testing.assert_close(dxd.cpu().double(), want, rtol=1e-6, atol=1e-7)
    else:
        torch.testing.assert_close(dxd.float().cpu(), q_bf16(dh / float(HW)).unsqueeze(1).expand(N, HW, C), rtol=0, atol=0)
