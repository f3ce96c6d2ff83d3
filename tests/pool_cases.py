"""Case lists, input builders and float64 references of the max-pool and the fused stem tail (no GPU, no pytest): csrc/bn_pool.hip
maxpool_fwd_kernel / maxpool_bwd_kernel, bn_relu_maxpool_fwd_kernel / bn_relu_maxpool_fwd16_kernel, bn_bwd_reduce_pool_kernel and
bn_bwd_apply_pool_kernel. tests/test_gpu_pool_edges.py runs the lists on the GPU; tests/test_pool_cases.py checks on the CPU, through
r3m_debug_pool_geometry, that the lists hold every launch condition they were written for, and that the references agree with
F.max_pool2d(return_indices=True) in float64.

INPUTS ON A LATTICE, so that the references are exact and the comparisons are equalities. y takes six levels k/4 in [-1, 1.5]; per
channel scale is a power of two from {0.5, 1, 2}, shift and mean lie on k/4, invstd is a power of two. Then
    t = fma(y, scale, shift)  on k/8, |t| <= 5         yhat = (y - mean) * invstd  on k/8, |yhat| <= 4.5
are exact in fp32 AND in bf16 (8 significant bits hold every k/8 up to 32), and so is relu(t). With six levels (the two top ones drawn twice as often) most 3 x 3 windows hold
their maximum more than once (the argmax is then decided by the scan order alone); a fixed share of t is exactly 0 (channel classes 0
and 3: the strict t > 0 of the backward's mask decides), and in channel class 3 only the top level is positive, so about a fifth of
its windows are all zero behind the ReLU. dp lies on k/8 with |dp| <= 2: the sum of the up to four pooled gradients that meet in one
pixel is on k/8 with |g| <= 8, exact in bf16, dy = scale g too (k/16, <= 16). The sums: every term of sum g is a multiple of 1/8 and
every term of sum g yhat a multiple of 1/64, so any partial sum below 2^24 / 64 in magnitude is exact in fp32 whatever the order;
fused_case asserts sum |g yhat| < 2^18 per channel. No input or coefficient is a negative zero, and none arises: y scale + shift
is +0 whenever it is 0 (round to nearest), as is y - mean.

REFERENCES. The window taps are unfolded from a -inf padded copy and numpy.argmax over the 9 taps returns the FIRST maximum, i.e. the
window code 3 i + j in row-major scan order (what include/r3m_hip.h and the header of csrc/bn_pool.hip promise, and what ATen does); the
input gradient is the scatter of dp by those codes; sums are float64.

A case is (name, (N, Hi, Wi, C)); the name says which condition of the launch geometry it is there for (tests/test_pool_cases.py holds
the conditions as predicates over the query's answer and requires a case on each side of every one). All are tiny: the largest
tensor has about 10^5 elements."""
import functools

import numpy as np

GUARD = 64                      # sentinel elements on either side of every output buffer
SIZE_CAP = 170_000              # elements of the largest tensor of a case
POOL_SEG = 8                    # csrc/bn_pool.hip: output rows one block of the bf16 row-walking forward owns
LEVELS = np.array([-1.0, -0.5, 0.0, 0.5, 1.0, 1.5])
LEVEL_WEIGHTS = np.array([1.0, 1.0, 1.0, 1.0, 2.0, 2.0])

GEOM_FIELDS = ("Ho", "Wo", "fwd_rows", "fwd_segs", "fwd_blocks", "fwd_threads", "fwd_items", "rq", "red_blocks", "red_threads", "red_items",
               "per_cv", "G", "red_lds", "red_cap", "app_blocks", "app_threads", "V")


def pool_geometry(L, N, Hi, Wi, C, dtype):
    """r3m_debug_pool_geometry as a dict (the launchers' own figures, nothing launched)"""
    import ctypes
    buf = (ctypes.c_int * 18)()
    n = L.r3m_debug_pool_geometry(N, Hi, Wi, C, 0 if dtype == "fp32" else 1, buf, 18)
    assert n == 18, L.r3m_last_error()
    return dict(zip(GEOM_FIELDS, list(buf)))


def out_hw(Hi, Wi):
    return (Hi + 2 - 3) // 2 + 1, (Wi + 2 - 3) // 2 + 1


def has_backward(C):
    """the channel counts r3m_bn_maxpool_bwd_dt takes"""
    return C >= 8 and C <= 1024 and (C & (C - 1)) == 0


# ---- the fused stem tail: (name, (N, Hi, Wi, C)) ----------------------------------------------------------------------------------
FUSED_CASES = [
    # extents 1, 2, 3 mixed with a larger other extent; odd and even parity of each (an odd extent: the last quad row / column has no
    # second pixel, va / vb of pool_quad are false there)
    ("extent_1x1", (2, 1, 1, 64)),
    ("extent_1x7", (2, 1, 7, 64)),
    ("extent_7x1", (2, 7, 1, 64)),
    ("extent_2x2", (3, 2, 2, 64)),
    ("extent_2x9", (2, 2, 9, 64)),
    ("extent_3x3", (1, 3, 3, 64)),
    ("parity_even_odd", (2, 6, 5, 64)),
    ("parity_odd_even", (2, 5, 6, 64)),
    # POOL_SEG: Ho = 8 (one full segment, from an odd and an even Hi), 9 (a second segment of one row), 16, 17 (three segments)
    ("seg_ho8_odd", (2, 15, 6, 64)),
    ("seg_ho8_even", (2, 16, 5, 64)),
    ("seg_ho9", (2, 17, 18, 64)),
    ("seg_ho16", (2, 32, 5, 64)),
    ("seg_ho17", (3, 33, 5, 64)),
    # the thread loops of the row-owning kernels: items exactly 1024 and just above per dtype at C = 64 (V = 4 fp32, 8 bf16), and the
    # same through channels
    ("trips_1024_fp32", (1, 3, 128, 64)),
    ("trips_1040_fp32", (1, 3, 130, 64)),
    ("trips_1024_bf16", (1, 3, 256, 64)),
    ("trips_1032_bf16", (1, 3, 258, 64)),
    ("trips_channels", (1, 3, 66, 256)),
    # pool_row_threads rounds up to 64: idle threads (Wo = 1, 3, 5 at C = 64 are extent_7x1, parity_even_odd, extent_2x9), threads per
    # channel vector that are no power of two, 1 / 2 / 3 of them, the smallest C
    ("per_cv_odd", (2, 5, 34, 64)),
    ("per_cv_1", (2, 3, 1, 1024)),
    ("per_cv_2", (2, 2, 3, 1024)),
    ("per_cv_3", (1, 3, 5, 1024)),
    ("per_cv_5_6", (2, 3, 9, 256)),
    ("per_cv_9_10", (1, 3, 18, 256)),
    ("c8", (2, 5, 7, 8)),
    ("c32", (2, 9, 7, 32)),
    # the reduce: more than 8 quad rows per block; 8 with as many blocks as the workspace holds; a short last block that spans frames
    ("rq_15", (3, 40, 16, 64)),
    ("rq_8_cap", (3, 25, 33, 64)),
    ("last_block_spans", (5, 5, 33, 64)),
    # forward only: channel counts the backward refuses. 24: no power of two, bf16 runs the one-output-per-thread kernel too
    ("fwd_c24", (2, 9, 7, 24)),
    ("fwd_c24_blocks", (3, 17, 18, 24)),
    ("fwd_c2048", (1, 5, 9, 2048)),
]

# ---- the plain max-pool: (name, (N, Hi, Wi, C)); C a multiple of 4, block of 256 (pixel, 4 channels) items ---------------------------
MAXPOOL_CASES = [
    ("1x1_c4", (1, 1, 1, 4)),
    ("1x7_c4", (2, 1, 7, 4)),
    ("7x1_c4", (3, 7, 1, 4)),
    ("2x2_c64", (1, 2, 2, 64)),
    ("2x9_c64", (2, 2, 9, 64)),
    ("3x3_c64", (3, 3, 3, 64)),
    ("6x5_c64", (2, 6, 5, 64)),
    ("5x6_c4", (3, 5, 6, 4)),
    ("17x18_c4", (3, 17, 18, 4)),
    ("33x5_c64", (2, 33, 5, 64)),
    ("3x258_c4", (1, 3, 258, 4)),
    ("25x33_c64", (3, 25, 33, 64)),
    ("16x16_c64", (2, 16, 16, 64)),          # both totals a multiple of 256
]


def case_id(c):
    return c[0]


def case_seed(shape):
    N, Hi, Wi, C = shape
    return ((N * 131 + Hi) * 521 + Wi) * 67 + C


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def lattice_coef(C):
    """[4][C] float64 = mean, invstd, scale, shift (the coefficient block's row order). Channel class c % 4: shift 0 (t = 0 at y = 0),
    +1/4, -1/4, and -scale (only the top level is positive, t = 0 at y = 1)."""
    c = np.arange(C)
    scale = np.array([0.5, 1.0, 2.0])[c % 3]
    shift = np.where(c % 4 == 3, -scale, np.array([0.0, 0.25, -0.25, 0.0])[c % 4])
    mean = np.array([0.25, -0.5, 0.0, 0.75, -0.25])[c % 5]
    invstd = np.array([1.0, 2.0, 0.5, 1.0, 0.5, 2.0, 1.0])[c % 7]
    return np.stack([mean, invstd, scale, shift])


def lattice_y(shape):
    """[N, Hi, Wi, C] float64, the six levels drawn with the two top ones twice as likely as the others: 60 - 70 % of the full 3 x 3
    windows then hold their maximum more than once"""
    rng = np.random.default_rng(case_seed(shape))
    return LEVELS[rng.choice(len(LEVELS), size=shape, p=LEVEL_WEIGHTS / LEVEL_WEIGHTS.sum())]


def lattice_dp(shape_in):
    """[N, Ho, Wo, C] float64 on k/8, |dp| <= 2"""
    N, Hi, Wi, C = shape_in
    Ho, Wo = out_hw(Hi, Wi)
    rng = np.random.default_rng(case_seed(shape_in) + 1)
    return rng.integers(-16, 17, size=(N, Ho, Wo, C)) / 8.0


def lattice_bases(C):
    """dgamma / dbeta buffers to accumulate onto, on k/4 (different ones for the two)"""
    rng = np.random.default_rng(C)
    return rng.integers(4, 9, size=C) / 4.0, rng.integers(-12, -7, size=C) / 4.0


def lattice_z(shape):
    """[N, Hi, Wi, C] float64 for the plain max-pool: few levels, negative ones too, and twice as many zeros as anything else"""
    rng = np.random.default_rng(case_seed(shape) + 2)
    return np.array([-0.5, 0.0, 0.0, 0.25, 0.5, 1.0])[rng.integers(0, 6, size=shape)]


# ---- references -------------------------------------------------------------------------------------------------------------------------
def window_taps(z):
    """[9, N, Ho, Wo, C]: tap 3 i + j of window (py, px) is pixel (2 py - 1 + i, 2 px - 1 + j), -inf outside the image"""
    N, Hi, Wi, C = z.shape
    Ho, Wo = out_hw(Hi, Wi)
    zp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf)
    zp[:, 1:Hi + 1, 1:Wi + 1] = z
    return np.stack([zp[:, i:i + 2 * Ho:2, j:j + 2 * Wo:2] for i in range(3) for j in range(3)])


def maxpool_ref(z):
    """pooled values and first-maximum window codes (uint8) of MaxPool2d(3, 2, 1) on NHWC float64"""
    taps = window_taps(z)
    return taps.max(0), taps.argmax(0).astype(np.uint8)


def maxpool_bwd_ref(dp, code, Hi, Wi):
    """dz [N, Hi, Wi, C]: every pooled gradient goes to the pixel its window code names; float64 sums"""
    N, Ho, Wo, C = dp.shape
    dzp = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, C))
    for t in range(9):
        i, j = divmod(t, 3)
        dzp[:, i:i + 2 * Ho:2, j:j + 2 * Wo:2] += np.where(code == t, dp, 0.0)
    return dzp[:, 1:Hi + 1, 1:Wi + 1].copy()


def argmax_counts(code, Hi, Wi):
    """per pixel, the number of windows whose argmax it is"""
    return maxpool_bwd_ref(np.ones(code.shape), code, Hi, Wi)


def tie_stats(z):
    """what a lattice tensor holds: windows whose maximum occurs more than once (all of them / those with a positive maximum), windows
    whose maximum is 0 (behind a ReLU: all zero), and the pixels that are the argmax of exactly 1, 2 and 4 windows"""
    taps = window_taps(z)
    p, code = taps.max(0), taps.argmax(0)
    multi = (taps == p[None]).sum(0) >= 2
    cnt = argmax_counts(code, z.shape[1], z.shape[2])
    return dict(windows=p.size, tied=int(multi.sum()), tied_positive=int((multi & (p > 0)).sum()), all_zero=int((p == 0).sum()),
                hit1=int((cnt == 1).sum()), hit2=int((cnt == 2).sum()), hit4=int((cnt == 4).sum()))


@functools.lru_cache(maxsize=None)
def maxpool_case(shape):
    """inputs and references of one plain max-pool case (float64 numpy, read-only)"""
    N, Hi, Wi, C = shape
    z = lattice_z(shape)
    p, code = maxpool_ref(z)
    dp = lattice_dp(shape)
    out = dict(z=z, p=p, code=code, dp=dp, dz=maxpool_bwd_ref(dp, code, Hi, Wi))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fused_case(shape):
    """inputs and references of one fused case (float64 numpy, read-only): y, coef [4][C], t, the activated z, pooled p, codes, dp,
    the masked gradient g = dz [t > 0], yhat, and the eval-mode backward dy = scale g, dbeta = sum g, dgamma = sum g yhat"""
    N, Hi, Wi, C = shape
    coef = lattice_coef(C)
    mean, invstd, scale, shift = coef
    y = lattice_y(shape)
    t = y * scale + shift
    z = np.maximum(t, 0.0)
    p, code = maxpool_ref(z)
    dp = lattice_dp(shape)
    g = np.where(t > 0, maxpool_bwd_ref(dp, code, Hi, Wi), 0.0)
    yhat = (y - mean) * invstd
    assert float(np.abs(g * yhat).reshape(-1, C).sum(0).max()) < 2.0 ** 18, "a partial sum of g yhat could round in fp32"
    out = dict(y=y, coef=coef, t=t, z=z, p=p, code=code, dp=dp, g=g, yhat=yhat, dy=scale * g, dbeta=g.reshape(-1, C).sum(0),
               dgamma=(g * yhat).reshape(-1, C).sum(0))
    for v in out.values():
        v.setflags(write=False)
    return out


def train_bwd_ref(case, dtype=np.float64):
    """dbeta, dgamma, dy of the batch-statistics backward on the case's g, evaluated in `dtype` (float64: the reference; float32: the
    witness of what the formula itself loses in fp32, tests/test_gpu_bn.py)"""
    C = case["y"].shape[-1]
    g, yhat = case["g"].reshape(-1, C).astype(dtype), case["yhat"].reshape(-1, C).astype(dtype)
    scale = case["coef"][2].astype(dtype)
    db, dg = g.sum(0), (g * yhat).sum(0)
    return db, dg, scale * (g - g.mean(0) - yhat * (g * yhat).mean(0))


# ---- launch conditions over the query's answer: name -> predicate(geometry dict, (N, Hi, Wi, C)); each needs a case per dtype -------------
def last_block_spans_frames(g, shape):
    """the last reduce block is short (fewer than rq quad rows) and holds rows of more than one frame"""
    quad_rows = shape[0] * g["Ho"]
    first = (g["red_blocks"] - 1) * g["rq"]
    return g["red_blocks"] > 1 and quad_rows - first < g["rq"] and first // g["Ho"] != (quad_rows - 1) // g["Ho"]


def some_block_spans_frames(g, shape):
    return any((b * g["rq"]) // g["Ho"] != (min((b + 1) * g["rq"], shape[0] * g["Ho"]) - 1) // g["Ho"] for b in range(g["red_blocks"]))


BACKWARD_CONDITIONS = {
    # thread loops of bn_bwd_reduce_pool_kernel / bn_bwd_apply_pool_kernel: one trip, exactly one full trip, a second trip of a few
    # items, a second trip reached through the channel count
    "items_below_1024": lambda g, s: g["red_items"] < 1024,
    "items_exactly_1024": lambda g, s: g["red_items"] == 1024,
    "items_just_above_1024": lambda g, s: 1024 < g["red_items"] <= 1024 + 64,
    "second_trip_through_channels": lambda g, s: g["red_items"] > 1024 and s[3] > 64,
    # pool_row_threads
    "items_below_64": lambda g, s: g["red_items"] < 64,
    "idle_threads": lambda g, s: g["red_threads"] > g["red_items"] > 64,
    "no_idle_threads": lambda g, s: g["red_threads"] == g["red_items"],
    # the two-stage LDS combine
    "per_cv_1": lambda g, s: g["per_cv"] == 1,
    "per_cv_2": lambda g, s: g["per_cv"] == 2,
    "per_cv_3": lambda g, s: g["per_cv"] == 3,
    "per_cv_below_8": lambda g, s: 4 <= g["per_cv"] < 8,
    "per_cv_8": lambda g, s: g["per_cv"] == 8,
    "per_cv_above_8_not_pow2": lambda g, s: g["per_cv"] > 8 and g["per_cv"] & (g["per_cv"] - 1) != 0,
    "per_cv_no_multiple_of_G": lambda g, s: g["per_cv"] % g["G"] != 0,
    # pool_reduce_geometry
    "rq_above_8": lambda g, s: g["rq"] > 8 and g["red_blocks"] > 1,
    "rq_8_many_blocks": lambda g, s: g["rq"] == 8 and g["red_blocks"] > 1,
    "single_block": lambda g, s: g["red_blocks"] == 1,
    "blocks_equal_cap": lambda g, s: g["red_blocks"] == g["red_cap"] > 1,
    "blocks_below_cap": lambda g, s: g["red_blocks"] < g["red_cap"],
    "last_block_short_spans_frames": last_block_spans_frames,
    "inner_block_spans_frames": some_block_spans_frames,
    "single_block_whole_frames": lambda g, s: g["red_blocks"] == 1 and s[0] > 1,
    # extents
    "H_1": lambda g, s: s[1] == 1, "H_2": lambda g, s: s[1] == 2, "H_3": lambda g, s: s[1] == 3,
    "W_1": lambda g, s: s[2] == 1, "W_2": lambda g, s: s[2] == 2, "W_3": lambda g, s: s[2] == 3,
    "H_odd_above_3": lambda g, s: s[1] % 2 == 1 and s[1] > 3, "H_even_above_3": lambda g, s: s[1] % 2 == 0 and s[1] > 3,
    "W_odd_above_3": lambda g, s: s[2] % 2 == 1 and s[2] > 3, "W_even_above_3": lambda g, s: s[2] % 2 == 0 and s[2] > 3,
    # channels
    "C_8": lambda g, s: s[3] == 8, "C_32": lambda g, s: s[3] == 32, "C_64": lambda g, s: s[3] == 64, "C_256": lambda g, s: s[3] == 256,
    "C_1024": lambda g, s: s[3] == 1024,
}

# the bf16 row-walking forward (fwd_rows = 1) and the one-output-per-thread kernel (fwd_rows = 0)
FORWARD_CONDITIONS = {
    "bf16": {
        "one_segment_full": lambda g, s: g["fwd_rows"] and g["Ho"] == POOL_SEG and s[0] >= 2,
        "one_segment_short": lambda g, s: g["fwd_rows"] and g["Ho"] < POOL_SEG,
        "second_segment_of_one_row": lambda g, s: g["fwd_rows"] and g["Ho"] == POOL_SEG + 1 and s[0] >= 2,
        "two_full_segments": lambda g, s: g["fwd_rows"] and g["Ho"] == 2 * POOL_SEG and s[0] >= 2,
        "three_segments": lambda g, s: g["fwd_rows"] and g["fwd_segs"] == 3 and s[0] >= 2,
        "segment_starts_behind_an_odd_Hi": lambda g, s: g["fwd_rows"] and g["fwd_segs"] > 1 and s[1] % 2 == 1,
        "segment_starts_behind_an_even_Hi": lambda g, s: g["fwd_rows"] and g["fwd_segs"] > 1 and s[1] % 2 == 0,
        "items_exactly_1024": lambda g, s: g["fwd_rows"] and g["fwd_items"] == 1024,
        "items_just_above_1024": lambda g, s: g["fwd_rows"] and 1024 < g["fwd_items"] <= 1024 + 64,
        "second_trip_through_channels": lambda g, s: g["fwd_rows"] and g["fwd_items"] > 1024 and s[3] > 64,
        "items_below_64": lambda g, s: g["fwd_rows"] and g["fwd_items"] < 64,
        "idle_threads": lambda g, s: g["fwd_rows"] and g["fwd_threads"] > g["fwd_items"] > 64,
        "C_2048": lambda g, s: g["fwd_rows"] and s[3] == 2048,
        "C_8": lambda g, s: g["fwd_rows"] and s[3] == 8,
        "templated_kernel_one_block": lambda g, s: not g["fwd_rows"] and g["fwd_blocks"] == 1,
        "templated_kernel_ragged_last_block": lambda g, s: not g["fwd_rows"] and g["fwd_blocks"] > 1 and (s[0] * g["Ho"] * g["Wo"] * s[3] // 8) % 256 != 0,
    },
    "fp32": {
        "one_block": lambda g, s: g["fwd_blocks"] == 1,
        "ragged_last_block": lambda g, s: g["fwd_blocks"] > 1 and (s[0] * g["Ho"] * g["Wo"] * s[3] // 4) % 256 != 0,
        "full_last_block": lambda g, s: g["fwd_blocks"] > 1 and (s[0] * g["Ho"] * g["Wo"] * s[3] // 4) % 256 == 0,
        "C_24": lambda g, s: s[3] == 24,
        "C_8": lambda g, s: s[3] == 8,
        "C_2048": lambda g, s: s[3] == 2048,
    },
}
