"""An independent model of what the launch profiler (csrc/capi.hip prof_begin / prof_bytes / prof_end, r3m_profile_*) must report for a
convolution launch: class, launches, GEMM extents, FLOPs and algorithmic bytes. Plain Python on integers; this file never calls the
library. What only the dispatch can know (the split-K factor of a weight gradient, the routes of a launch, the number of statistics
rows a forward writes) comes in as arguments, from tests/route_sig.py and the library's own queries.

A case is (N, Hi, Wi, Ci, Co, k, stride, pad); dt is 0 (fp32) or 1 (bf16 activations).

FLOPs
  forward, weight gradient   2 N Ho Wo Co k^2 Ci
  input gradient, stride 1   2 N Hi Wi Ci k^2 Co
  input gradient, stride s   2 Ci Co N x the number of (input pixel, kernel tap) pairs whose tap is compatible with the pixel's parity
                             class: (iy + pad - ky) % s == 0 and (ix + pad - kx) % s == 0. The pairs are counted by enumeration over
                             (iy mod s, ix mod s, ky, kx), and a pair whose output pixel (iy + pad - ky) / s falls outside the output
                             map (a tap on padding) is counted too: this is the work the gather GEMM performs (it multiplies a zero
                             row there), not the smaller number of multiplications the mathematical operation needs.
  stem                       2 F Ho Wo 64 147

Algorithmic bytes: operands read once and results written once (the header comment of r3m_profile_collect_bytes). Per launch:
  e x (elements of the GEMM's input tensor that some (output row, tap) pair of the launch reads: padding and pixels no tap reaches are
       not traffic, e.g. three quarters of the input of a 1x1 / stride-2 convolution)
  + e x the weights of the launch's taps + e x the result
  + what the epilogue flags add: statistics rows (8 bytes per row and channel, written), bias (4 Nc), eval-BatchNorm scale and shift
    (8 Nc), the old result it adds onto (e x result), a masked residual (e x result + 1 bit per element), the activation whose sign
    masks the stored gradient (e x result), BatchNorm-backward partials (the BatchNorm input e x result, its mask as bits or as scale and
    shift to recompute it (8 Nc), the mean (4 Nc), 8 bytes per partial row and channel written)
  weight gradient: e x (dY + the input elements in range) + 4 split Co k^2 Ci for the split-K slabs (its reduce is not bracketed).
e = 4 (fp32) or 2 (bf16); weights of a bf16 launch are the bf16 image, every per-channel vector and every partial row is fp32.

Class: a GEMM launch is wide (0) when the GEMM's output width is a multiple of 128, or when a bf16 3x3 launch runs the kernel-row
route (32); else narrow (1). A weight gradient is wide (2) when both channel counts are multiples of 128, else narrow (3). Stem launches
are narrow (1 forward, 3 weight gradient)."""
import collections

GEMM_WIDE, GEMM_NARROW, WGRAD_WIDE, WGRAD_NARROW = 0, 1, 2, 3
STATS, ACCUM, MASKED_ADD, BIAS, RELU, MASK_OUT, BNRED, AFFINE = 1, 2, 4, 8, 16, 32, 64, 128
ROUTE_BF16_ROW = 32

# one bracketed launch: what a CSV row of r3m_profile_dump_to holds (class, M, N, K, taps) and its FLOPs and bytes
Launch = collections.namedtuple("Launch", "kclass M N K taps flops bytes")


def esize(dt):
    return 2 if dt else 4


def out_hw(case):
    N, Hi, Wi, Ci, Co, k, s, p = case
    return (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1


def forward_flops(case):
    N, Hi, Wi, Ci, Co, k, s, p = case
    Ho, Wo = out_hw(case)
    return 2 * N * Ho * Wo * Co * k * k * Ci


def wgrad_flops(case):
    return forward_flops(case)


def class_taps(r, k, s, p):
    """kernel offsets compatible with the input coordinates of residue r (mod s)"""
    return [kk for kk in range(k) if (r + p - kk) % s == 0]


def dgrad_pairs(case):
    """(input pixel, kernel tap) pairs of one frame whose tap is compatible with the pixel's parity class, taps on padding included"""
    N, Hi, Wi, Ci, Co, k, s, p = case
    pairs = 0
    for ry in range(s):
        for rx in range(s):
            pixels = len(range(ry, Hi, s)) * len(range(rx, Wi, s))
            pairs += pixels * len(class_taps(ry, k, s, p)) * len(class_taps(rx, k, s, p))
    return pairs


def dgrad_flops(case):
    N, Hi, Wi, Ci, Co, k, s, p = case
    return 2 * Ci * Co * N * dgrad_pairs(case)


def stem_flops(F, Ho, Wo):
    return 2 * F * Ho * Wo * 64 * 147


def fwd_inputs_in_range(n_in, n_out, k, s, p):
    """how many of the n_in input coordinates of one dimension some (output coordinate, kernel offset) pair reads"""
    return len({o * s - p + kk for o in range(n_out) for kk in range(k)} & set(range(n_in)))


def gemm_class(width, dt, k, route=None):
    return GEMM_WIDE if width % 128 == 0 or (dt == 1 and k == 3 and route == ROUTE_BF16_ROW) else GEMM_NARROW


def wgrad_class(case):
    return WGRAD_WIDE if case[3] % 128 == 0 and case[4] % 128 == 0 else WGRAD_NARROW


def epilogue_bytes(flags, bits, M, Nc, e, stats_rows):
    """what the epilogue flags add to input + weights + result; `bits`: the BatchNorm-backward mask comes as bits"""
    out = M * Nc
    b = 0
    if flags & STATS:
        b += 8 * stats_rows * Nc
    if flags & BIAS:
        b += 4 * Nc
    if flags & AFFINE:
        b += 8 * Nc
    if flags & ACCUM:
        b += e * out
    if flags & MASKED_ADD:
        b += e * out + out / 8
    if flags & MASK_OUT:
        b += e * out
    if flags & BNRED:
        b += e * out + (out / 8 if bits else 8 * Nc) + 4 * Nc + 8 * ((M + 63) // 64) * Nc
    return b


def forward_launches(case, dt, flags=0, routes=(), stats_rows=0):
    """the one launch of a forward; routes: what route_sig.routes lists for it (only the bf16 kernel-row route changes the class)"""
    N, Hi, Wi, Ci, Co, k, s, p = case
    Ho, Wo = out_hw(case)
    e = esize(dt)
    M = N * Ho * Wo
    x = N * fwd_inputs_in_range(Hi, Ho, k, s, p) * fwd_inputs_in_range(Wi, Wo, k, s, p) * Ci
    by = e * (x + Co * k * k * Ci + M * Co) + epilogue_bytes(flags, 0, M, Co, e, stats_rows)
    return [Launch(gemm_class(Co, dt, k, routes[0] if routes else None), M, Co, Ci, k * k, forward_flops(case), by)]


def dgrad_launches(case, dt, flags=0, bits=0, routes=()):
    """the launches of an input gradient: one at stride 1; at stride s one per parity class that has pixels, except that a class without
    taps is skipped when the launch only adds onto a stored gradient (flags == ACCUM: there is nothing to add)"""
    N, Hi, Wi, Ci, Co, k, s, p = case
    Ho, Wo = out_hw(case)
    e = esize(dt)
    out = []
    for ry in range(s):
        for rx in range(s):
            ys, xs = range(ry, Hi, s), range(rx, Wi, s)
            ty, tx = class_taps(ry, k, s, p), class_taps(rx, k, s, p)
            taps = len(ty) * len(tx)
            if not ys or not xs or (taps == 0 and (flags & ACCUM) and not (flags & MASKED_ADD)):
                continue
            M = N * len(ys) * len(xs)
            # rows / columns of dY this class reads: oy = (iy + pad - ky) / s inside the output map
            rows = {(iy + p - ky) // s for iy in ys for ky in ty} & set(range(Ho))
            cols = {(ix + p - kx) // s for ix in xs for kx in tx} & set(range(Wo))
            dy = N * len(rows) * len(cols) * Co if taps else 0
            by = e * (dy + Ci * taps * Co + M * Ci) + epilogue_bytes(flags, bits, M, Ci, e, 0)
            route = routes[len(out)] if len(routes) > len(out) else None
            out.append(Launch(gemm_class(Ci, dt, k, route), M, Ci, Co, taps, 2 * M * Ci * taps * Co, by))
    return out


def wgrad_launches(case, dt, split):
    """the one bracketed launch of a weight gradient (its split-K reduce is not bracketed); split: route_sig.wgrad_plan(...).split"""
    N, Hi, Wi, Ci, Co, k, s, p = case
    Ho, Wo = out_hw(case)
    e = esize(dt)
    M = N * Ho * Wo
    x = N * fwd_inputs_in_range(Hi, Ho, k, s, p) * fwd_inputs_in_range(Wi, Wo, k, s, p) * Ci
    by = e * (M * Co + x) + 4 * split * Co * k * k * Ci
    return [Launch(wgrad_class(case), M, Co, Ci, k * k, wgrad_flops(case), by)]


def stem_hw(H, W):
    return (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1


def stem_launches(F, H, W, dt, op, stats_rows=0, image_bytes=None):
    """conv1 (7x7 / stride 2 / pad 3, 3 -> 64) as the stem kernels run it, op 'fwd' | 'wgrad': a GEMM of M = F Ho Wo rows, 64 columns and
    K = 147 with one 'tap'. Bytes: the normalised image once (every pixel is in range; image_bytes when the kernel reads a padded image,
    else F H W 3 elements), conv1's fp32 weights (forward) and the result or dY; the stem weight gradient's partial sums leave through a
    fixed-size workspace that its unpack pass reduces (not bracketed, not counted)."""
    Ho, Wo = stem_hw(H, W)
    e = esize(dt)
    M = F * Ho * Wo
    img = F * H * W * 3 * e if image_bytes is None else image_bytes
    by = img + M * 64 * e
    if op == "fwd":
        by += 4 * 64 * 147 + 8 * stats_rows * 64
    return [Launch(GEMM_NARROW if op == "fwd" else WGRAD_NARROW, M, 64, 147, 1, stem_flops(F, Ho, Wo), by)]


def totals(launches):
    """per class: [launches, FLOPs, bytes]"""
    t = [[0, 0, 0] for _ in range(4)]
    for l in launches:
        t[l.kclass][0] += 1
        t[l.kclass][1] += l.flops
        t[l.kclass][2] += l.bytes
    return t
