"""Case lists and float64 references of the resampling kernels (no GPU, no pytest): csrc/augment.hip crop_resize_kernel and
resize_crop_bwd_kernel, csrc/augment_dev.h bilinear_sample, and the crop pre-passes of the 224 stem (csrc/stem_dev.h StemCrop,
csrc/stem_bf16.hip stem_prep16_crop_u8_kernel). tests/test_gpu_resample_edges.py runs the lists on the GPU, tests/test_resample_cases.py
checks on the CPU that the lists hold every class they were written for and that the references agree with torch's float64
F.interpolate and its autograd.

One axis of a resample is (n_in, full, off, n): n_in source pixels are resized to `full`, of which the window [off, off + n) is
computed. The kernels take the source index and the interpolation weight of a window pixel in fp32,

    s = max(fl32(fma(dst + off + 0.5, fl32(n_in / full), -0.5)), 0),   i0 = int(s),   i1 = i0 + (i0 < n_in - 1),   l = s - i0,

and axis_taps() repeats exactly that: (dst + off + 0.5) has at most 12 significant bits and the fp32 scale 24, so their product
(36 bits, no smaller than 2^-13 here) and its sum with -0.5 are exact in float64 and ONE rounding to float32 is the fma's. l = s - i0
is exact in fp32. Everything after the index -- 1 - l, p / 255, the interpolation, * 255 -- the references do in float64.

FORWARD BOUND. bilinear_sample rounds to fp32 eight times between the source pixels and the value it returns. Every rounded quantity
is at most 1 (255 for the last), the weights of an interpolation step add up to 1, so a rounding made on each of its inputs counts
once, and each is at most 2^-24 relative (2^-25 absolute on values below 1, which covers the second-order terms):
    1  v = p / 255             (the four taps; (float)p is exact for bytes and for float frames)
    2  hx = 1 - lx
    3  lx * v01                (and lx * v11: the two rows are averaged by the y step)
    4  t0 = fma(hx, v00, .)    (and t1)
    5  hy = 1 - ly
    6  ly * t1
    7  fma(hy, t0, .)
    8  * 255
k = 8:  FWD_BOUND = 8 * 2^-24 * 255 = 1.216e-4 absolute, below the atol = 2e-4 of tests/test_gpu_augment.py.

ADJOINT BOUND, per source pixel (iy, ix): (n_y + n_x + 4) * 2^-24 * S, where n_y (n_x) is the number of window rows (columns) whose
taps include iy (ix) -- the length of the two fma chains of resize_crop_bwd_kernel -- and S = |A_y|^T |dout| |A_x| is the same sum of
absolute values; the 4 are 1 - l and the clamped (1 - l) + l of resize_tap_weight on each axis. S == 0 (no window pixel taps the
source pixel) means an exact zero.
"""
import collections
import functools

import numpy as np

U = 2.0 ** -24                  # unit roundoff of float32
FWD_ROUNDINGS = 8
FWD_BOUND = FWD_ROUNDINGS * U * 255.0
SIZE_CAP = 120_000              # pixels of the frames or of the output of one resize / crop case ("about 10^5")
GUARD = 64                      # sentinel elements on either side of every output buffer


# ---- one axis ------------------------------------------------------------------------------------------------------------------
def axis_taps(n_in, full, off, n):
    """(i0, i1, l) of the window pixels off .. off + n - 1, in the kernels' fp32 arithmetic; l is float32"""
    d = np.arange(n, dtype=np.float64) + off + 0.5
    scale = np.float32(n_in) / np.float32(full)                          # IEEE fp32 division
    s = np.maximum((d * np.float64(scale) - 0.5).astype(np.float32), np.float32(0))
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, s - i0.astype(np.float32)


@functools.lru_cache(maxsize=None)
def axis_matrix(n_in, full, off, n):
    """A [n, n_in] float64: row d holds the two tap weights of window pixel d (their sum on one pixel where the tap clamps)"""
    i0, i1, l = axis_taps(n_in, full, off, n)
    A = np.zeros((n, n_in))
    r = np.arange(n)
    np.add.at(A, (r, i0), 1.0 - l.astype(np.float64))
    np.add.at(A, (r, i1), l.astype(np.float64))
    A.setflags(write=False)
    return A


def axis_tap_counts(n_in, full, off, n):
    """per source pixel, the number of window pixels with a non-zero tap weight on it"""
    return (axis_matrix(n_in, full, off, n) != 0).sum(0)


def index_error(n_in):
    """|s_fp32 - s_exact| of one axis: the fp32 scale is off by at most 2^-24 relative, which (dst + 0.5) * scale <= n_in turns into
    n_in 2^-24; the fma's one rounding of a result below n_in adds as much."""
    return 2.0 * U * n_in


# ---- references ------------------------------------------------------------------------------------------------------------------
def forward_ref(planes, ay, ax):
    """planes [..., n_in_y, n_in_x] (0..255) -> [..., n_y, n_x] float64: A_y (p / 255) A_x^T * 255"""
    Ay, Ax = axis_matrix(*ay), axis_matrix(*ax)
    return Ay @ (np.asarray(planes, dtype=np.float64) / 255.0) @ Ax.T * 255.0


Adjoint = collections.namedtuple("Adjoint", "din S n_y n_x")


def adjoint_ref(dout, ay, ax):
    """dout [..., n_y, n_x] -> din = A_y^T dout A_x, S = |A_y|^T |dout| |A_x| [..., n_in_y, n_in_x], tap counts n_y [n_in_y], n_x [n_in_x]"""
    Ay, Ax = axis_matrix(*ay), axis_matrix(*ax)
    g = np.asarray(dout, dtype=np.float64)
    return Adjoint(Ay.T @ g @ Ax, np.abs(Ay).T @ np.abs(g) @ np.abs(Ax), axis_tap_counts(*ay), axis_tap_counts(*ax))


def adjoint_bound(adj):
    return (adj.n_y[:, None] + adj.n_x[None, :] + 4) * U * adj.S


def crop_resize_ref(frames, boxes, fpb, Ho, Wo):
    """frames [N, C, Hi, Wi], boxes [nb, 4] = (top, left, height, width), frame n takes box n // fpb -> [N, C, Ho, Wo] float64"""
    frames = np.asarray(frames)
    out = np.empty(frames.shape[:2] + (Ho, Wo))
    for n in range(frames.shape[0]):
        t, l, h, w = [int(v) for v in boxes[n // fpb]]
        out[n] = forward_ref(frames[n, :, t:t + h, l:l + w], (h, Ho, 0, Ho), (w, Wo, 0, Wo))
    return out


def first_bad(err, tol):
    """None, or the index of the first element with err > tol (or a NaN) and its two figures"""
    bad = ~(err <= tol)
    if not bad.any():
        return None
    i = np.unravel_index(int(np.argmax(bad)), bad.shape)
    return tuple(int(v) for v in i), float(err[i]), float(np.broadcast_to(tol, err.shape)[i])


# ---- r3m_resize_crop / r3m_resize_crop_backward: axis classes -----------------------------------------------------------------------
# name -> (class, (n_in, full, off, n))
AXES = {
    "ident9": ("identity", (9, 9, 0, 9)),
    "ident9_last": ("identity", (9, 9, 8, 1)),
    "up2": ("up2", (5, 10, 0, 10)),
    "down2": ("down2", (10, 5, 0, 5)),
    "in1": ("in1", (1, 7, 0, 7)),
    "in1_mid": ("in1", (1, 7, 2, 3)),
    "in2": ("in2", (2, 9, 0, 9)),
    "full1": ("full1", (5, 1, 0, 1)),
    "up3": ("strong_up", (3, 224, 0, 224)),
    "up7": ("strong_up", (7, 224, 0, 224)),
    "up7_first": ("strong_up", (7, 224, 0, 1)),
    "up7_last": ("strong_up", (7, 224, 223, 1)),
    "up7_mid": ("strong_up", (7, 224, 37, 50)),
    "down509": ("strong_down", (509, 32, 0, 32)),
    "down509_mid": ("strong_down", (509, 32, 5, 11)),
    "down512": ("strong_down", (512, 7, 0, 7)),
    "r224": ("ratio", (224, 256, 0, 256)),
    "r224_mid": ("ratio", (224, 256, 16, 224)),
    "r341": ("ratio", (341, 256, 0, 256)),
    "r341_mid": ("ratio", (341, 256, 31, 100)),
    "r7_5": ("ratio", (7, 5, 0, 5)),
    "r7_5_last": ("ratio", (7, 5, 4, 1)),
}
AXIS_CLASSES = ("identity", "up2", "down2", "in1", "in2", "full1", "strong_up", "strong_down", "ratio")
# classes whose source index is exact in fp32 (ratio 1 or a power of two): the references then equal torch float64 to rounding
EXACT_INDEX_AXES = ("ident9", "ident9_last", "up2", "down2")
# (height axis, width axis); every pair is also run transposed
_PAIRS = [
    ("ident9", "up2"), ("up2", "down2"), ("down2", "in1"), ("in1", "in2"), ("in2", "full1"), ("full1", "up3"), ("up3", "down512"),
    ("up7", "r7_5"), ("down509", "up7_mid"), ("down512", "ident9"), ("r7_5", "in2"), ("r224", "r341"), ("r341_mid", "r224_mid"),
    ("up7_first", "r341"), ("r7_5_last", "up7_last"), ("ident9_last", "down509_mid"), ("in1_mid", "down509"), ("ident9", "down2"),
    ("ident9", "ident9_last"),          # the identity on both axes: the output is fl32(fl32(p / 255) * 255) bit for bit
]
RESIZE_CASES = [p for ab in _PAIRS for p in (ab, ab[::-1])]
# the cases mutant (c) of profiles/resample_edges.txt may run on: full_Wo >= full_Ho
RESIZE_CASES_WIDE_FULL = [c for c in RESIZE_CASES if AXES[c[1]][1][1] >= AXES[c[0]][1][1]]


def resize_case(case):
    """(N, C, ay, ax) of a RESIZE_CASES entry: four planes where they fit the size cap, else one"""
    ay, ax = AXES[case[0]][1], AXES[case[1]][1]
    px = max(ay[0] * ax[0], ay[3] * ax[3])
    N, C = (2, 2) if 4 * px <= SIZE_CAP else (1, 1)
    return N, C, ay, ax


def resize_case_pixels(case):
    N, C, ay, ax = resize_case(case)
    return N * C * max(ay[0] * ax[0], ay[3] * ax[3])


def case_seed(*key):
    return sum((i + 1) * 7919 * sum(ord(ch) for ch in str(k)) for i, k in enumerate(key)) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def resize_inputs(case):
    """(x_u8 [N,C,Hi,Wi] uint8, x_f float32 in 0..255 with fractions, dout [N,C,Ho,Wo] float32, prefill [N,C,Hi,Wi] float32)"""
    N, C, ay, ax = resize_case(case)
    rng = np.random.default_rng(case_seed(*case))
    x_u8 = rng.integers(0, 256, (N, C, ay[0], ax[0]), dtype=np.uint8)
    x_f = (rng.random((N, C, ay[0], ax[0])) * 255.0).astype(np.float32)
    dout = rng.standard_normal((N, C, ay[3], ax[3])).astype(np.float32)
    prefill = rng.standard_normal((N, C, ay[0], ax[0])).astype(np.float32)
    for a in (x_u8, x_f, dout, prefill):
        a.setflags(write=False)
    return x_u8, x_f, dout, prefill


@functools.lru_cache(maxsize=None)
def resize_refs(case):
    """(forward of x_u8, forward of x_f, Adjoint of dout): computed once, shared, read-only"""
    N, C, ay, ax = resize_case(case)
    x_u8, x_f, dout, _ = resize_inputs(case)
    out = (forward_ref(x_u8, ay, ax), forward_ref(x_f, ay, ax), adjoint_ref(dout, ay, ax))
    for a in (out[0], out[1], out[2].din, out[2].S):
        a.setflags(write=False)
    return out


# ---- r3m_crop_resize ----------------------------------------------------------------------------------------------------------------
CROP_FRAME = (12, 17)           # Hi x Wi of the box cases


def edge_boxes(Hi, Wi, Ho, Wo):
    """the boxes every output size is run on: whole frame, 1 x 1, 1 x W, H x 1, one box on each edge, one in each corner, and a box of
    exactly the output size (the identity) where the frame holds one"""
    b = [(0, 0, Hi, Wi), (5, 6, 1, 1), (3, 0, 1, Wi), (0, 9, Hi, 1),
         (0, 4, 5, 6), (Hi - 5, 3, 5, 9), (2, 0, 7, 4), (3, Wi - 6, 6, 6),
         (0, 0, 4, 5), (0, Wi - 5, 3, 5), (Hi - 4, 0, 4, 6), (Hi - 3, Wi - 4, 3, 4)]
    if Ho <= Hi - 2 and Wo <= Wi - 3:
        b.append((2, 3, Ho, Wo))
    return b


CropCase = collections.namedtuple("CropCase", "name N C Hi Wi Ho Wo fpb boxes")


def _crop(name, N, C, Ho, Wo, fpb, boxes=None, frame=CROP_FRAME):
    Hi, Wi = frame
    nb = -(-N // fpb)
    pool = boxes if boxes is not None else edge_boxes(Hi, Wi, Ho, Wo)
    return CropCase(name, N, C, Hi, Wi, Ho, Wo, fpb, tuple(pool[i % len(pool)] for i in range(nb)))


CROP_CASES = [
    _crop("1x1_C1", 13, 1, 1, 1, 1),
    _crop("1x9_C4", 13, 4, 1, 9, 1),
    _crop("1x9_C3_N7_fpb3", 7, 3, 1, 9, 3, boxes=[(0, 0, 12, 17), (9, 13, 3, 4), (5, 6, 1, 1)]),
    _crop("9x1_C4_fpb5", 65, 4, 9, 1, 5),
    _crop("5x7_C3", 13, 3, 5, 7, 1),
    _crop("5x7_C1_fpb3", 37, 1, 5, 7, 3),
    _crop("224x224_C1", 2, 1, 224, 224, 1, boxes=[(9, 13, 3, 4), (0, 0, 12, 17)]),
    _crop("3x300_C3_fpb5", 10, 3, 3, 300, 5, boxes=[(0, 12, 3, 5), (3, 0, 1, 17)]),
    _crop("3x300_C1", 12, 1, 3, 300, 1),
    # launch edges of the 256-thread blocks: 1, 255, 256 and 257 elements, and 1025 frames (the 64-bit index decode)
    _crop("total1", 1, 1, 1, 1, 1, boxes=[(11, 16, 1, 1)]),
    _crop("total255", 5, 3, 1, 17, 1),
    _crop("total256", 1, 4, 8, 8, 1, boxes=[(8, 0, 4, 6)]),
    _crop("total257", 1, 1, 1, 257, 1, boxes=[(3, 11, 6, 6)]),
    _crop("N1025_2x3_fpb5", 1025, 1, 2, 3, 5, boxes=[(0, 0, 4, 5), (3, 4, 1, 1), (0, 0, 2, 3), (1, 1, 2, 3), (0, 4, 4, 1), (2, 0, 2, 5)],
          frame=(4, 5)),
]
CROP_OUTPUT_SIZES = {(1, 1), (1, 9), (9, 1), (5, 7), (224, 224), (3, 300)}


@functools.lru_cache(maxsize=None)
def crop_inputs(name):
    c = {c.name: c for c in CROP_CASES}[name]
    rng = np.random.default_rng(case_seed(name))
    x_u8 = rng.integers(0, 256, (c.N, c.C, c.Hi, c.Wi), dtype=np.uint8)
    x_f = (rng.random((c.N, c.C, c.Hi, c.Wi)) * 255.0).astype(np.float32)
    x_u8.setflags(write=False)
    x_f.setflags(write=False)
    return x_u8, x_f


@functools.lru_cache(maxsize=None)
def crop_refs(name):
    c = {c.name: c for c in CROP_CASES}[name]
    out = tuple(crop_resize_ref(x, c.boxes, c.fpb, c.Ho, c.Wo) for x in crop_inputs(name))
    for a in out:
        a.setflags(write=False)
    return out


# ---- r3m_stem_prep_crop ---------------------------------------------------------------------------------------------------------------
# Boxes sorted by what stem_prep16_crop_u8_kernel branches on: bw / 224 below, at and above 1.5 (a pixel pair shares its dword loads up
# to there), the identity, bw of 1-3 (both taps of many pixels in one byte pair), boxes that end at the row's last byte (clamped load
# addresses) and start at its first, one- and two-row boxes, boxes in the last rows of the last frame (the end of the allocation).
WIDE = (6, 512)
WIDE_BOXES = [(0, 5, 6, 1), (1, 511, 2, 1), (0, 0, 1, 2), (3, 509, 3, 3), (0, 100, 6, 224), (0, 288, 6, 224), (2, 0, 4, 335),
              (0, 176, 5, 336), (4, 175, 2, 337), (0, 0, 6, 500), (5, 12, 1, 500)]
StemCropCase = collections.namedtuple("StemCropCase", "name F fpb Hi Wi boxes")
STEM_CROP_CASES = [
    StemCropCase("wide_F11_fpb1", 11, 1, *WIDE, tuple(WIDE_BOXES)),
    StemCropCase("wide_F11_fpb5", 11, 5, *WIDE, ((0, 176, 5, 336), (2, 0, 4, 335), (5, 12, 1, 500))),
    StemCropCase("wide_F2_fpb5", 2, 5, *WIDE, ((4, 175, 2, 337),)),
    StemCropCase("wide_F1", 1, 1, *WIDE, ((5, 12, 1, 500),)),
    StemCropCase("w4_F11_fpb5", 11, 5, 5, 4, ((0, 0, 5, 4), (3, 1, 2, 3), (4, 0, 1, 4))),      # Wi = 4: every dword load clamped to column 0
    StemCropCase("w4_F2_fpb1", 2, 1, 5, 4, ((0, 3, 5, 1), (4, 2, 1, 2))),
    StemCropCase("w3_F2_fpb1", 2, 1, 2, 3, ((0, 0, 2, 3), (1, 2, 1, 1))),                      # Wi < 4: the generic kernel on bytes
    StemCropCase("w1_F2_fpb5", 2, 5, 3, 1, ((1, 0, 2, 1),)),
]
STEM_CROP_WIDTHS = {1, 2, 3, 224, 335, 336, 337, 500}


@functools.lru_cache(maxsize=None)
def stem_crop_inputs(name):
    c = {c.name: c for c in STEM_CROP_CASES}[name]
    rng = np.random.default_rng(case_seed(name))
    x_u8 = rng.integers(0, 256, (c.F, 3, c.Hi, c.Wi), dtype=np.uint8)
    x_f = (rng.random((c.F, 3, c.Hi, c.Wi)) * 255.0).astype(np.float32)
    x_u8.setflags(write=False)
    x_f.setflags(write=False)
    return x_u8, x_f


@functools.lru_cache(maxsize=None)
def stem_crop_ref(name, is_u8):
    c = {c.name: c for c in STEM_CROP_CASES}[name]
    out = crop_resize_ref(stem_crop_inputs(name)[0 if is_u8 else 1], c.boxes, c.fpb, 224, 224)
    out.setflags(write=False)
    return out
