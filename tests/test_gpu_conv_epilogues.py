"""-m gpu: the convolution epilogues and the scheduling mode that only r3m_resnet_forward / _backward launched, one launch at a time
through the C ABI against float64 on the CPU (the bodies and ceilings are in tests/util.py):

* the inference stores (flags 128, 128|16, 128|2|16) through r3m_conv2d_fwd_affine_dt: the fp32 window kernel, the fp32 persistent
  kernel on its three tiles (128 x 128, 256 x 64, the 512 x 64 burst variant), the bf16 gather, halo and kernel-row kernels; fp32 also
  bit for bit against r3m_conv2d_fwd + r3m_bn_act_fwd;
* the accumulating input gradient of the downsample branch and the masked residual join without BatchNorm partials through
  r3m_conv2d_dgrad_join_dt, both dtypes;
* the per-XCD tile queues of the fp32 persistent kernel through r3m_debug_next_launch_tile_queues: outputs pre-filled with NaN, compared
  with float64 and bit for bit with the static split, and the counters read back to see which of the two the launcher really ran.

The case lists are plain module constants: tests/test_dispatch.py pins their routes, checks that every queue case passes the launcher's
threshold, and matches every launch of the engine at the non-square frame sizes against them flag for flag, all without a GPU.

profiles/r11_conv_epilogue_mutants.txt: the mutation check and the run times."""
import pytest
import torch

from util import ACCUM, AFFINE, DEV, RELU, check_conv_affine, check_conv_queues, check_dgrad_join

pytestmark = pytest.mark.gpu

A, AR, AAR = AFFINE, AFFINE | RELU, AFFINE | ACCUM | RELU
ALL3, RELU2 = (A, AR, AAR), (AR, AAR)

# ---- inference stores, fp32: (N, Hi, Wi, Ci, Co, k, stride, pad) -> the flag sets run on it ---------------------------------------------
AFFINE_FP32_GROUPS = {
    # 3x3 / stride 1, 128-wide, Wi <= 28: the window kernel (built for the two ReLU forms only). 480 and 588 rows: a ragged last tile
    "window": [((2, 10, 24, 128, 128, 3, 1, 1), RELU2), ((2, 24, 10, 128, 128, 3, 1, 1), RELU2), ((3, 14, 14, 256, 256, 3, 1, 1), RELU2)],
    # persistent kernel, pointwise form, 128 x 128 tile: 720 / 1080 rows (ragged), wide and tall; 64 -> 256 is layer1.0 of ResNet-50
    "pointwise_128": [((3, 12, 20, 64, 256, 1, 1, 0), ALL3), ((3, 20, 12, 256, 128, 1, 1, 0), ALL3), ((3, 18, 20, 128, 512, 1, 1, 0), ALL3)],
    # ... gather form, 128 x 128 tile: 3x3 / stride 1 wider than the window kernel takes (wide, tall, 330 rows: ragged), 3x3 / stride 2
    "gather_128": [((2, 6, 32, 128, 128, 3, 1, 1), ALL3), ((2, 5, 33, 128, 128, 3, 1, 1), ALL3), ((1, 40, 29, 128, 128, 3, 1, 1), ALL3),
                   ((3, 13, 10, 128, 256, 3, 2, 1), ALL3), ((3, 10, 13, 64, 128, 3, 2, 1), ALL3)],
    # the eight-wave tiles of 64-wide outputs: K >= 2 Nc with 128|16 runs the burst variant on the 512 x 64 tile, with 128|2|16 the
    # normal variant on the 256 x 64 tile; K = 64 stays on the 256 x 64 tile with every flag set. 2880 rows: more than one tile, ragged
    "tile_64": [((3, 24, 40, 64, 64, 3, 1, 1), ALL3), ((3, 40, 24, 64, 64, 3, 1, 1), RELU2), ((3, 24, 40, 256, 64, 1, 1, 0), ALL3),
                ((3, 40, 24, 64, 64, 1, 1, 0), ALL3)],
    # the downsample branch: 1x1 / stride 2 (gather form, one tap), even / odd / mixed extents
    "downsample": [((2, 13, 10, 128, 256, 1, 2, 0), (A,)), ((2, 10, 13, 128, 256, 1, 2, 0), (A,)), ((2, 13, 11, 256, 512, 1, 2, 0), (A,)),
                   ((2, 20, 12, 64, 128, 1, 2, 0), (A,))],
    # a one-pixel map (layer4 of a 32 x 32 frame): the window kernel and the pointwise form on three rows
    "one_pixel": [((3, 1, 1, 512, 512, 3, 1, 1), RELU2), ((3, 1, 1, 512, 2048, 1, 1, 0), ALL3)],
}
AFFINE_FP32_CASES = [(c, fl) for g in AFFINE_FP32_GROUPS.values() for (c, fls) in g for fl in fls]
# launches the engine does not make (r3m_debug_conv_fuses_affine answers 0): the window kernel without ReLU, a statistics flag on top, a
# width the persistent kernel does not take (96: the gather kernel, which has no inference store); bf16: 32 input channels
AFFINE_REFUSED = [((2, 10, 24, 128, 128, 3, 1, 1), A, 0), ((3, 12, 20, 64, 256, 1, 1, 0), A | 1, 0), ((2, 13, 13, 32, 96, 3, 2, 1), AR, 0),
                  ((3, 12, 20, 64, 256, 1, 1, 0), A | 1, 1), ((2, 13, 13, 32, 128, 3, 2, 1), AR, 1)]

# ---- inference stores, bf16 ------------------------------------------------------------------------------------------------------------
AFFINE_BF16_GROUPS = {
    # route 30, the gather kernel: 1x1 (Co = 64, 128, 256; ragged M), 1x1 / stride 2, 3x3 / stride 2, wide and tall
    "gather": [((3, 12, 20, 64, 256, 1, 1, 0), ALL3), ((3, 24, 40, 256, 64, 1, 1, 0), ALL3), ((3, 20, 12, 256, 128, 1, 1, 0), ALL3),
               ((2, 13, 10, 128, 256, 1, 2, 0), ALL3), ((2, 10, 13, 128, 256, 1, 2, 0), (A,)), ((3, 13, 10, 128, 256, 3, 2, 1), ALL3),
               ((3, 10, 13, 64, 128, 3, 2, 1), RELU2), ((3, 1, 1, 512, 2048, 1, 1, 0), ALL3), ((3, 40, 24, 64, 64, 1, 1, 0), RELU2)],
    # 3x3 / stride 1 maps too wide for the kernel-row kernel's staged rows: the halo kernel (31) in the DEFAULT mode (layer1 / layer2 of
    # a 33 x 512 frame)
    "row16_too_wide": [((1, 9, 128, 64, 64, 3, 1, 1), RELU2), ((2, 6, 40, 128, 128, 3, 1, 1), RELU2)],
    # routes 32 (kernel-row kernel, the default) and 31 (halo kernel, r3m_debug_set_conv3x3_bf16(0)): 3x3 / stride 1, wide and tall,
    # Co = 64 and 128, ragged M (360 = 128 + 128 + 104 rows; 2880 = 11 x 256 + 64)
    "conv3x3": [((2, 6, 30, 128, 128, 3, 1, 1), RELU2), ((2, 30, 6, 128, 128, 3, 1, 1), RELU2), ((3, 24, 40, 64, 64, 3, 1, 1), RELU2),
                ((3, 40, 24, 64, 64, 3, 1, 1), RELU2), ((2, 5, 30, 64, 128, 3, 1, 1), RELU2), ((2, 56, 5, 128, 64, 3, 1, 1), RELU2)],
}
AFFINE_BF16_CASES = [(c, fl) for g in ("gather", "row16_too_wide") for (c, fls) in AFFINE_BF16_GROUPS[g] for fl in fls]
AFFINE_BF16_3X3_CASES = [(c, fl) for (c, fls) in AFFINE_BF16_GROUPS["conv3x3"] for fl in fls]

# ---- input gradients: (case, mode) ------------------------------------------------------------------------------------------------------
JOIN_GROUPS = {
    # the downsample branch's accumulate, 1x1 / stride 2 at (odd, even), (even, odd), (odd, odd), (even, even) extents: three of the four
    # parity classes have no tap and must be skipped, not zeroed. fp32: the strided-output form of the persistent kernel (route 13)
    "accumulate_stride2": [((2, 13, 10, 128, 256, 1, 2, 0), "accumulate"), ((2, 10, 13, 128, 256, 1, 2, 0), "accumulate"),
                           ((2, 13, 11, 128, 256, 1, 2, 0), "accumulate"), ((2, 20, 12, 64, 128, 1, 2, 0), "accumulate"),
                           ((3, 9, 15, 256, 512, 1, 2, 0), "accumulate"),
                           # the one class with a tap is narrower than the persistent kernel takes (Wg = 3): the gather kernel (21)
                           ((2, 10, 6, 256, 512, 1, 2, 0), "accumulate")],
    # ... 1x1 / stride 1, 64 -> 256: layer1.0 of ResNet-50 (a 64-wide input gradient: the 256 x 64 tile)
    "accumulate_stride1": [((3, 12, 20, 64, 256, 1, 1, 0), "accumulate"), ((3, 20, 12, 64, 256, 1, 1, 0), "accumulate")],
    # the masked join without partials: 3x3 / stride 1 at 64 channels (the first block of an fp32 ResNet-18 / -34 plan, exactly as the
    # engine passes it: residual + its bits, no BatchNorm operands), 128 and 256 channels, wide and tall; 1x1 (the bottleneck's first conv)
    "join": [((3, 24, 40, 64, 64, 3, 1, 1), "join"), ((3, 40, 24, 64, 64, 3, 1, 1), "join"), ((2, 10, 24, 128, 128, 3, 1, 1), "join"),
             ((2, 24, 10, 128, 128, 3, 1, 1), "join"), ((3, 6, 32, 256, 256, 3, 1, 1), "join"), ((3, 32, 6, 256, 256, 3, 1, 1), "join"),
             ((3, 12, 20, 256, 64, 1, 1, 0), "join"), ((3, 20, 12, 512, 128, 1, 1, 0), "join"), ((3, 40, 24, 256, 64, 1, 1, 0), "join"),
             ((3, 12, 20, 512, 128, 1, 1, 0), "join"),
             # a 64-channel map too wide for the bf16 kernel-row kernel (layer1 of a 33 x 512 frame): the halo kernel in the default mode
             ((1, 9, 128, 64, 64, 3, 1, 1), "join")],
}
JOIN_CASES = [cm for g in JOIN_GROUPS.values() for cm in g]

# ---- tile queues, fp32: the launcher hands them on from 64 row panels (conv_pw.hip launch_pw_shape) -----------------------------------------
# (kind, case, flags or None, used). 3 x 56 x 56 = 9408 rows = 73.5 tiles of 128: gridM = 74 = 9 x 8 + 2, a ragged last group of panels
# and a ragged last tile; 90 x 90 = 8100 rows: gridM = 64; 89 x 90 = 8010 rows: gridM = 63, the static split although queues are handed
# over. 64-wide outputs: 6 x 56 x 56 = 18816 rows = 73.5 tiles of 256 (the launches that take the 512 x 64 burst tile would need twice that).
QUEUE_CASES = [
    ("fwd_stats", (3, 56, 56, 64, 128, 1, 1, 0), None, True),          # pointwise, gridM 74, gridN 1
    ("fwd_stats", (3, 56, 56, 64, 256, 1, 1, 0), None, True),          # gridN 2
    ("fwd_stats", (1, 90, 90, 64, 128, 1, 1, 0), None, True),          # gridM 64
    ("fwd_stats", (1, 89, 90, 64, 128, 1, 1, 0), None, False),         # gridM 63: static
    ("fwd_stats", (6, 56, 56, 64, 64, 1, 1, 0), None, True),           # 256 x 64 tile, gridM 74
    ("fwd_stats", (3, 56, 56, 128, 128, 3, 2, 1), None, False),        # gather form, 2352 rows: static
    ("affine", (3, 56, 56, 64, 256, 1, 1, 0), AAR, True),              # gridN 2, the residual read through the queue's tile index
    ("affine", (3, 56, 56, 128, 128, 3, 1, 1), AR, True),              # gather form, 128 x 128 tile
    ("affine", (6, 56, 56, 64, 64, 3, 1, 1), AAR, True),               # gather form, 256 x 64 tile
    ("affine", (1, 89, 90, 64, 128, 1, 1, 0), A, False),
    ("dgrad", (3, 56, 56, 128, 64, 1, 1, 0), None, True),              # plain, pointwise, 128-wide input gradient
    ("dgrad", (3, 56, 56, 512, 128, 1, 1, 0), None, True),             # gridN 4
    ("dgrad", (3, 112, 112, 128, 128, 3, 2, 1), None, True),           # four parity launches of 9408 rows, four counter sets
    ("accumulate", (3, 112, 112, 128, 256, 1, 2, 0), None, True),      # the one parity class with a tap; three sets stay unused
]


def _ids(v):
    if isinstance(v, tuple) and len(v) == 8:
        return "N{}_{}x{}_{}to{}_k{}s{}p{}".format(*v)
    return str(v)


@pytest.mark.parametrize("case,flags", AFFINE_FP32_CASES, ids=_ids)
def test_affine_store_fp32(hip, case, flags):
    check_conv_affine(hip, case, flags, "fp32")


@pytest.mark.parametrize("case,flags", AFFINE_BF16_CASES, ids=_ids)
def test_affine_store_bf16(hip, case, flags):
    check_conv_affine(hip, case, flags, "bf16")


@pytest.mark.parametrize("kernel", ["kernel_row", "halo"])
@pytest.mark.parametrize("case,flags", AFFINE_BF16_3X3_CASES, ids=_ids)
def test_affine_store_bf16_kernel_row_and_halo_kernel(hip, case, flags, kernel):
    old = hip.r3m_debug_set_conv3x3_bf16(1 if kernel == "kernel_row" else 0)
    try:
        check_conv_affine(hip, case, flags, "bf16")
    finally:
        hip.r3m_debug_set_conv3x3_bf16(old)


@pytest.mark.parametrize("case,flags,dt", AFFINE_REFUSED, ids=_ids)
def test_affine_store_is_refused_where_the_engine_would_not_fuse(hip, case, flags, dt):
    N, Hi, Wi, Ci, Co, k, s, p = case
    Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
    tdt = torch.float32 if dt == 0 else torch.bfloat16
    x = torch.zeros((N, Hi, Wi, Ci), dtype=tdt, device=DEV)
    w = torch.zeros((Co, k, k, Ci), dtype=tdt, device=DEV)
    out = torch.full((N, Ho, Wo, Co), 7.0, dtype=tdt, device=DEV)
    sc = torch.ones(Co, device=DEV)
    rc = hip.r3m_conv2d_fwd_affine_dt(x.data_ptr(), w.data_ptr(), out.data_ptr(), sc.data_ptr(), sc.data_ptr(), N, Hi, Wi, Ci, Co, k, s, p,
                                      flags, dt, torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    msg = hip.r3m_last_error().decode()
    assert "conv2d_fwd_affine" in msg and f"flags {flags}" in msg, msg
    assert bool((out == 7.0).all()), "a refused launch wrote its output"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case,mode", JOIN_CASES, ids=_ids)
def test_dgrad_accumulate_and_masked_join(hip, case, mode, dtype):
    check_dgrad_join(hip, case, mode, dtype)


def test_dgrad_join_refuses_what_the_engine_never_asks(hip):
    z = torch.zeros(64 * 64 * 9 * 4, dtype=torch.float32, device=DEV)
    args = (z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.numel() * 4, 1, 4, 4, 64, 64)
    st = torch.cuda.current_stream().cuda_stream
    assert hip.r3m_conv2d_dgrad_join_dt(*args, 1, 1, 0, 0, None, None, 0, st) != 0 and b"one of the two" in hip.r3m_last_error()
    assert hip.r3m_conv2d_dgrad_join_dt(*args, 1, 1, 0, 1, z.data_ptr(), z.data_ptr(), 0, st) != 0 and b"one of the two" in hip.r3m_last_error()
    assert hip.r3m_conv2d_dgrad_join_dt(*args, 1, 1, 0, 0, z.data_ptr(), None, 0, st) != 0 and b"mask bits" in hip.r3m_last_error()
    assert hip.r3m_conv2d_dgrad_join_dt(*args, 3, 1, 1, 1, None, None, 0, st) != 0 and b"downsample" in hip.r3m_last_error()
    assert bool((z == 0).all())


@pytest.mark.parametrize("kind,case,flags,used", QUEUE_CASES, ids=_ids)
def test_tile_queues_equal_the_static_split(hip, kind, case, flags, used):
    if kind == "affine":
        check_conv_affine(hip, case, flags, "fp32", queues=1 if used else -1)
    elif kind == "accumulate":
        check_dgrad_join(hip, case, "accumulate", "fp32", queues=4)
    else:
        check_conv_queues(hip, case, kind, used=used)
