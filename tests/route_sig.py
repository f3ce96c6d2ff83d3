"""Dispatch signatures (no GPU, no pytest): which kernel families a convolution launch takes, classed the way the coverage test of
tests/test_dispatch.py compares the engine's launches with the operator tests' case lists.

A signature is (dtype, dgrad, flags, mask_bits, routes, k, stride, Co % 128 == 0, wide | tall | square): everything the dispatch
(csrc/conv.hip gg_route, conv_bf16.hip gg16_route) can tell apart, minus the sizes themselves."""
import ctypes as C

STATS, ACCUM, MASKED_ADD, BNRED, AFFINE, RELU = 1, 2, 4, 64, 128, 16
# (dgrad, flags, mask_bits) the operator entry points of include/r3m_hip.h can ask for: r3m_conv2d_fwd[_dt] with / without statistics,
# r3m_conv2d_dgrad[_dt], r3m_conv2d_dgrad_bnred_dt in its three modes. The engine's other epilogues (accumulate onto a stored
# gradient, masked join without partials, eval-BatchNorm forwards) have no entry point of their own.
OPERATOR_EPILOGUES = {(0, STATS, 0), (0, 0, 0), (1, 0, 0), (1, BNRED, 0), (1, BNRED, 1), (1, BNRED | MASKED_ADD, 1)}
BNRED_MODES = {"recompute": (BNRED, 0), "bits": (BNRED, 1), "bits+residual": (BNRED | MASKED_ADD, 1)}


def shape_class(Hi, Wi):
    return "wide" if Wi > Hi else "tall" if Hi > Wi else "square"


def routes(L, case, dgrad, flags, bits, dt):
    """route of every launch, () when the dispatch refuses the combination"""
    N, Hi, Wi, Ci, Co, k, s, p = case
    buf = (C.c_int * 8)()
    n = L.r3m_debug_conv_route(N, Hi, Wi, Ci, Co, k, s, p, dgrad, flags, bits, dt, buf, 8)
    return tuple(buf[:max(n, 0)])


def signature(L, case, dgrad, flags, bits, dt):
    N, Hi, Wi, Ci, Co, k, s, p = case
    return (dt, dgrad, flags, bits, routes(L, case, dgrad, flags, bits, dt), k, s, Co % 128 == 0, shape_class(Hi, Wi))


def conv_case_signatures(L, cases, dt):
    """what check_conv_fp32 / check_conv_bf16 (tests/util.py, strict) launch for each case: forward with and without statistics, plain
    input gradient"""
    return {signature(L, c, dg, fl, 0, dt): c for c in cases for (dg, fl) in ((0, STATS), (0, 0), (1, 0))}


def bnred_case_signatures(L, cases):
    """what check_dgrad_bnred launches for each (case, mode, dtype)"""
    return {signature(L, c, 1, *BNRED_MODES[mode], 0 if dtype == "fp32" else 1): (c, mode, dtype) for (c, mode, dtype) in cases}


def plan_convs(L, h):
    """[(Ci, Co, k, stride, pad, Hi, Wi, Ho, Wo)] of a plan, conv1 (the stem) first"""
    v = [C.c_int() for _ in range(9)]
    out = []
    for i in range(L.r3m_resnet_num_convs(h)):
        assert L.r3m_resnet_conv_info(h, i, *[C.byref(x) for x in v]) == 0, L.r3m_last_error()
        out.append(tuple(x.value for x in v))
    return out


def plan_blocks(convs, size):
    """[(convs of the block in order, downsample conv or None)] from a plan's conv table (torchvision module order)"""
    convs = convs[1:]
    n = 3 if size == 50 else 2
    out, i = [], 0
    while i < len(convs):
        body = convs[i:i + n]
        i += n
        ds = None
        if i < len(convs) and convs[i][2] == 1 and convs[i][0] == body[0][0] and convs[i][1] == body[-1][1] and \
                (convs[i][3] == 2 or convs[i][0] != convs[i][1]):
            ds = convs[i]
            i += 1
        out.append((body, ds))
    return out


def engine_launches(L, size, dt, F, H, W):
    """[(case, dgrad, flags, mask_bits)] of every forward and input-gradient launch behind the stem of one plan, with the flags
    csrc/engine.hip asks: forward with statistics (training) and plain (eval with a backward), input gradients as plan_backward asks
    them (fp32 plans fuse the BatchNorm-backward partials, bf16 plans do not), fused inference forwards where
    r3m_debug_conv_fuses_affine answers 1 for the whole block. The one derivation for tests/test_resolution_plan.py and
    tests/test_dispatch.py."""
    h = L.r3m_resnet_create_hw(size, F, dt, H, W)
    assert h, L.r3m_last_error()
    try:
        blocks = plan_blocks(plan_convs(L, h), size)
    finally:
        L.r3m_resnet_destroy(h)
    fuse_bnred = dt == 0
    out = []

    def add(c, dgrad, flags, bits=0):
        Ci, Co, k, s, p, Hi, Wi = c[:7]
        out.append(((F, Hi, Wi, Ci, Co, k, s, p), dgrad, flags, bits))

    for bi, (body, ds) in enumerate(blocks):
        for c in body + ([ds] if ds else []):
            add(c, 0, STATS)
            add(c, 0, 0)
        for j in range(len(body) - 1, 0, -1):
            add(body[j], 1, BNRED if fuse_bnred else 0)
        if ds:
            add(body[0], 1, 0)
            add(ds, 1, ACCUM)
        else:
            add(body[0], 1, MASKED_ADD | (BNRED if fuse_bnred and bi > 0 else 0), 1 if bi > 0 else 0)
        want = [(c, AFFINE | RELU) for c in body[:-1]] + [(body[-1], AFFINE | ACCUM | RELU)] + ([(ds, AFFINE)] if ds else [])
        fused = all(L.r3m_debug_conv_fuses_affine(F, c[5], c[6], c[0], c[1], c[2], c[3], c[4], fl, dt) == 1 for c, fl in want)
        for c, fl in want:
            add(c, 0, fl if fused else 0)
    return out
