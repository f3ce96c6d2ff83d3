"""Dispatch signatures (no GPU, no pytest): which kernel families a convolution launch takes, classed the way the coverage test of
tests/test_dispatch.py compares the engine's launches with the operator tests' case lists.

A signature is (dtype, dgrad, flags, mask_bits, routes, k, stride, Co % 128 == 0, wide | tall | square): everything the dispatch
(csrc/conv.hip gg_route, conv_bf16.hip gg16_route) can tell apart, minus the sizes themselves."""
import collections
import ctypes as C

STATS, ACCUM, MASKED_ADD, BNRED, AFFINE, RELU = 1, 2, 4, 64, 128, 16
BIAS, MASK_OUT = 8, 32         # only the language-reward head asks these: Linear + bias + ReLU forward, ReLU mask on the stored input gradient
# (dgrad, flags, mask_bits) the operator entry points of include/r3m_hip.h can ask for: r3m_conv2d_fwd[_dt] with / without statistics,
# r3m_conv2d_dgrad[_dt], r3m_conv2d_dgrad_bnred_dt in its three modes, r3m_conv2d_dgrad_join_dt (accumulate onto a stored gradient;
# masked join without partials -- its residual bits are not the mask_bits of a signature, which are the BatchNorm partials'),
# r3m_conv2d_fwd_affine_dt (the three eval-BatchNorm stores of inference). Nothing the engine launches is left without one. The last two
# are the language-reward head's (csrc/lang.hip mlp_forward / mlp_backward), reached through r3m_langrew_* (head_launches below).
OPERATOR_EPILOGUES = {(0, STATS, 0), (0, 0, 0), (1, 0, 0), (1, BNRED, 0), (1, BNRED, 1), (1, BNRED | MASKED_ADD, 1),
                      (1, ACCUM, 0), (1, MASKED_ADD, 0), (1, MASKED_ADD, 1),
                      (0, AFFINE, 0), (0, AFFINE | RELU, 0), (0, AFFINE | ACCUM | RELU, 0),
                      (0, BIAS | RELU, 0), (1, MASK_OUT, 0)}
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


def affine_case_signatures(L, cases, dt):
    """what check_conv_affine launches for each (case, flags)"""
    return {signature(L, c, 0, fl, 0, dt): (c, fl) for (c, fl) in cases}


def join_case_signatures(L, cases, dt):
    """what check_dgrad_join launches for each (case, mode): mode 'accumulate' -> EPI_ACCUM, 'join' -> EPI_MASKED_ADD with residual bits and
    no BatchNorm partials. The engine asks the join with mask_bits 0 (first block) and 1 (bf16 plans: the bits it would hand the partials
    it does not fuse); without EPI_BNRED the dispatch never sees them, which signature() shows: both are recorded."""
    out = {}
    for (c, mode) in cases:
        if mode == "accumulate":
            out[signature(L, c, 1, ACCUM, 0, dt)] = (c, mode)
        else:
            for bits in (0, 1):
                out[signature(L, c, 1, MASKED_ADD, bits, dt)] = (c, mode)
    return out


def head_launches(R, K1, H, dt):
    """[(case, dgrad, flags)] of the GEMM launches of one language-reward head pass over R rows (csrc/lang.hip): a Linear(K -> H) is the
    1x1 convolution of R one-pixel images. fp32: forward with bias + ReLU (24) for K1 -> H and H -> H, input gradient plain for layer 0
    and with the ReLU mask of the layer below (32) for layers 1-3. The bf16 head asks plain stores (flags 0) throughout."""
    lin = lambda K: (R, 1, 1, K, H, 1, 1, 0)
    fwd = 0 if dt else BIAS | RELU
    return [(lin(K1), 0, fwd), (lin(H), 0, fwd), (lin(K1), 1, 0), (lin(H), 1, 0 if dt else MASK_OUT)]


def head_signature(L, case, dgrad, flags, dt):
    """(dtype, dgrad, flags, routes, Co % 128 == 0) of one head launch: k, stride and the map are 1 x 1 for every one of them"""
    return (dt, dgrad, flags, routes(L, case, dgrad, flags, 0, dt), case[4] % 128 == 0)


def pw_queue_grids(L, case, dgrad, flags):
    """[(gridM, gridN)] of every launch of an fp32 convolution on the persistent kernel, from the tile sizes csrc/conv_pw.hip launch_pw_gemm
    picks: 128 x 128 for outputs a multiple of 128 wide; else 256 x 64, or 512 x 64 for the burst launches (dense output rows, K >= 2 N,
    flags 0 / statistics / 128|16 / partials with the mask recomputed). launch_pw_shape hands the tile queues on when gridM >= 64 and
    min(tiles, resident blocks) >= 64, which gridM >= 64 implies on any device of 64 CUs or more. () when a launch takes another kernel."""
    N, Hi, Wi, Ci, Co, k, s, p = case
    r = routes(L, case, dgrad, flags, 0, 0)
    if not r or any(x not in (11, 12, 13) for x in r):
        return ()
    Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
    if not dgrad:
        Ms, Nc, K = [N * Ho * Wo], Co, (1 if (k == 1 and s == 1 and p == 0) else k * k) * Ci
    elif s == 1:
        Ms, Nc, K = [N * Hi * Wi], Ci, (1 if (k == 1 and p == 0) else k * k) * Co
    else:       # one launch per parity class that has taps (and extent); strided output rows: never the burst tile
        Ms = []
        for py in (0, 1):
            for px in (0, 1):
                Hg, Wg = (Hi - py + 1) // 2, (Wi - px + 1) // 2
                taps = sum(1 for kh in range(k) for kw in range(k) if (py + p - kh) % 2 == 0 and (px + p - kw) % 2 == 0)
                if Hg > 0 and Wg > 0 and not (taps == 0 and flags == ACCUM):
                    Ms.append(N * Hg * Wg)
        Nc, K = Ci, None
    assert len(Ms) == len(r), (case, Ms, r)
    out = []
    for M, route in zip(Ms, r):
        if Nc % 128 == 0:
            BM, BN = 128, 128
        else:
            burst = route != 13 and K >= 2 * Nc and flags in (0, STATS, AFFINE | RELU, BNRED)
            BM, BN = (512 if burst else 256), 64
        out.append((-(-M // BM), Nc // BN))
    return tuple(out)


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


# ---- the weight gradients behind the stem (csrc/wgrad.hip wgrad_plan, through r3m_debug_wgrad_route) ------------------------------------------
WG_TAPS_SIMPLE, WG_TAPS_GATHER, WG_ROWS, WG_WINDOW, WG16_TAPS, WG16_ROWS, WG16_ALL_TAPS = 40, 41, 42, 43, 50, 51, 52
WG_ROUTES = {0: (WG_TAPS_SIMPLE, WG_TAPS_GATHER, WG_ROWS, WG_WINDOW), 1: (WG16_TAPS, WG16_ROWS, WG16_ALL_TAPS)}
WgPlan = collections.namedtuple("WgPlan", "route tile bk fast split rows_per_split tilesN gx lds_bytes")


def wgrad_plan(L, case, dt):
    """the plan of one weight-gradient launch, case = (N, Hi, Wi, Ci, Co, k, stride, pad)"""
    buf = (C.c_int * 9)()
    assert L.r3m_debug_wgrad_route(*case, dt, buf, 9) == 9, L.r3m_last_error()
    return WgPlan(*buf)


def wgrad_variant(r):
    """the kernel instantiation a plan names: the route and the fields that pick a template variant inside it"""
    return (r.route, r.tile, r.bk, r.fast)


def wgrad_operator_cases():
    """[(origin, case, dtype)] of every weight gradient the GPU operator tests run and compare (tests/test_gpu_ops.py, test_gpu_ops_hw.py,
    test_gpu_fuzz.py): fp32 against F.conv2d autograd, bf16 against float64 / exact integers"""
    import test_gpu_fuzz as Z
    import test_gpu_ops as O
    import test_gpu_ops_hw as T
    sq = lambda c: (c[0], c[1], c[1]) + tuple(c[2:])
    out = [("ops", sq(c), 0) for c in O.CONV_CASES]
    out += [("ops_hw", c, 0) for c in T.HW_CONV_CASES] + [("ops_hw", c, 1) for c in T.HW_BF16_CASES + T.HW_ROW16_CASES]
    out += [("ops_hw", (2, 5, 9, 64, 128, 3, s, 1), dt) for s in (1, 2) for dt in (0, 1)]       # test_conv3x3_pixel_codes_are_exact_hw
    out += [("fuzz", sq(c), 0) for c in Z.FP32_CASES] + [("fuzz", sq(c), 1) for c in Z.BF16_CASES]
    return out
