"""CPU: the case lists of tests/test_gpu_resample_edges.py (tests/resample_cases.py) hold every class they were written for and stay
under the size cap, and the float64 references agree with torch's float64 F.interpolate(align_corners=False) + crop and its autograd.

torch takes the source index in float64, the references in the kernels' fp32. Where the resize ratio is 1 or a power of two the fp32
index is exact and the two agree to 1e-12. Elsewhere the fp32 index is off by at most d = 2 * 2^-24 * n_in per axis
(resample_cases.index_error: one rounding of the scale, one of the fma). A bilinear interpolant is piecewise linear and continuous in
the index, the clamps at 0 and at the last pixel included, with slope at most the largest difference of neighbouring pixels, so
    forward:  |ref - torch| <= (d_y + d_x) * 255
and a tap weight moves by at most d, on at most the n + 2 window pixels that tap a source pixel before or after the move, so
    adjoint:  |ref - torch| <= max|dout| * (d_y + d_x) * (n_y + 2) * (n_x + 2)      per source pixel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_cases as R


def _torch_forward(x, ay, ax):
    y = F.interpolate(torch.from_numpy(np.asarray(x, dtype=np.float64)) / 255.0, size=(ay[1], ax[1]), mode="bilinear",
                      align_corners=False) * 255.0
    return y[:, :, ay[2]:ay[2] + ay[3], ax[2]:ax[2] + ax[3]]


# ---- the lists -------------------------------------------------------------------------------------------------------------------
def test_every_axis_class_is_on_the_height_and_on_the_width_beside_another_class():
    assert len(set(R.RESIZE_CASES)) == len(R.RESIZE_CASES)
    for cls in R.AXIS_CLASSES:
        on_h = [c for c in R.RESIZE_CASES if R.AXES[c[0]][0] == cls and R.AXES[c[1]][0] != cls]
        on_w = [c for c in R.RESIZE_CASES if R.AXES[c[1]][0] == cls and R.AXES[c[0]][0] != cls]
        assert on_h and on_w, cls
        assert any(c[::-1] in on_w for c in on_h), cls
    assert {c for c, _ in R.AXES.values()} == set(R.AXIS_CLASSES)
    used = {n for c in R.RESIZE_CASES for n in c}
    assert used == set(R.AXES), set(R.AXES) - used


def test_the_named_axes_are_in_the_list():
    ax = {a for _, a in R.AXES.values()}
    resize = {a[:2] for a in ax}
    for pair in ((5, 10), (10, 5), (3, 224), (7, 224), (509, 32), (512, 7), (224, 256), (341, 256), (7, 5)):
        assert pair in resize, pair
    assert any(a[0] == a[1] for a in ax) and any(a[0] == 1 for a in ax) and any(a[0] == 2 for a in ax) and any(a[1] == 1 for a in ax)
    for (n_in, full, off, n) in ax:
        assert n_in >= 1 and full >= 1 and off >= 0 and n >= 1 and off + n <= full
    # windows: the whole resized frame, its first row / column only, its last only, an interior window with top != left and Ho != Wo
    assert any(a[2] == 0 and a[3] == a[1] for a in ax)
    assert any(a[2] == 0 and a[3] == 1 and a[1] > 1 for a in ax) and any(a[2] == a[1] - 1 and a[3] == 1 and a[1] > 1 for a in ax)
    inner = lambda a: a[2] > 0 and a[2] + a[3] < a[1]
    assert any(inner(R.AXES[h][1]) and inner(R.AXES[w][1]) and R.AXES[h][1][2] != R.AXES[w][1][2] and R.AXES[h][1][3] != R.AXES[w][1][3]
               for h, w in R.RESIZE_CASES)


def test_the_clamps_and_the_untapped_pixels_the_cases_were_chosen_for():
    for name in ("in1", "in1_mid", "in2"):                         # every tap clamps: i1 == i0 at the last pixel
        a = R.AXES[name][1]
        i0, i1, l = R.axis_taps(*a)
        assert ((i1 == i0) | (i0 == a[0] - 2)).all() and (i1 == i0).any(), name
    for name in ("up3", "up7"):                                    # many outputs at the max(., 0) clamp and at the last-pixel clamp
        a = R.AXES[name][1]
        i0, i1, l = R.axis_taps(*a)
        assert ((i0 == 0) & (l == 0)).sum() > 10 and (i1 == i0).sum() > 10, name
    for name in ("down509", "down509_mid", "down512"):             # source pixels no window pixel taps
        assert (R.axis_tap_counts(*R.AXES[name][1]) == 0).sum() > R.AXES[name][1][0] // 2, name
    for name in ("up2", "down2"):                                  # exact weights: quarters / halves
        assert set(np.unique(R.axis_matrix(*R.AXES[name][1]))) <= {0.0, 0.25, 0.5, 0.75, 1.0}, name
    assert np.array_equal(R.axis_matrix(9, 9, 0, 9), np.eye(9))
    for name in R.EXACT_INDEX_AXES:                                # ratio 1 or a power of two: held to torch float64 at 1e-12
        n_in, full = R.AXES[name][1][:2]
        assert max(n_in, full) % min(n_in, full) == 0 and (max(n_in, full) // min(n_in, full)) in (1, 2, 4, 8), name
    assert sum(h in R.EXACT_INDEX_AXES and w in R.EXACT_INDEX_AXES for h, w in R.RESIZE_CASES) >= 4
    assert R.RESIZE_CASES_WIDE_FULL and all(R.AXES[w][1][1] >= R.AXES[h][1][1] for h, w in R.RESIZE_CASES_WIDE_FULL)


def test_no_case_is_over_the_size_cap():
    for c in R.RESIZE_CASES:
        assert R.resize_case_pixels(c) <= R.SIZE_CAP, (c, R.resize_case_pixels(c))
    for c in R.CROP_CASES:
        assert max(c.N * c.C * c.Hi * c.Wi, c.N * c.C * c.Ho * c.Wo) <= R.SIZE_CAP, c.name
    for c in R.STEM_CROP_CASES:                                    # the output is the stem's 224 x 224 whatever the case
        assert c.F * 3 * c.Hi * c.Wi <= R.SIZE_CAP and c.F <= 11, c.name
    assert R.FWD_BOUND <= 2e-4 and R.FWD_ROUNDINGS == 8


def _boxes_inside(boxes, Hi, Wi):
    return all(t >= 0 and l >= 0 and h >= 1 and w >= 1 and t + h <= Hi and l + w <= Wi for (t, l, h, w) in boxes)


def test_crop_cases_hold_every_output_size_channel_count_and_box_kind():
    cs = R.CROP_CASES
    assert len({c.name for c in cs}) == len(cs)
    assert {(c.Ho, c.Wo) for c in cs} >= R.CROP_OUTPUT_SIZES
    assert {c.C for c in cs} >= {1, 3, 4} and {c.fpb for c in cs} >= {1, 3, 5}
    assert any(c.N == 7 and c.fpb == 3 and len(c.boxes) == 3 for c in cs)
    assert {c.N * c.C * c.Ho * c.Wo for c in cs} >= {1, 255, 256, 257}
    assert any(c.N == 1025 and (c.Ho, c.Wo) == (2, 3) for c in cs)
    for c in cs:
        assert len(c.boxes) == -(-c.N // c.fpb) and _boxes_inside(c.boxes, c.Hi, c.Wi), c.name
    kinds = {
        "whole": lambda c, b: b == (0, 0, c.Hi, c.Wi),
        "1x1": lambda c, b: b[2:] == (1, 1),
        "1xW": lambda c, b: b[2:] == (1, c.Wi),
        "Hx1": lambda c, b: b[2:] == (c.Hi, 1),
        "top": lambda c, b: b[0] == 0 and b[1] > 0 and b[1] + b[3] < c.Wi and b[2] < c.Hi,
        "bottom": lambda c, b: b[0] + b[2] == c.Hi and b[0] > 0 and b[1] > 0 and b[1] + b[3] < c.Wi,
        "left": lambda c, b: b[1] == 0 and b[0] > 0 and b[0] + b[2] < c.Hi and b[3] < c.Wi,
        "right": lambda c, b: b[1] + b[3] == c.Wi and b[1] > 0 and b[0] > 0 and b[0] + b[2] < c.Hi,
        "top-left": lambda c, b: b[:2] == (0, 0) and b[2] < c.Hi and b[3] < c.Wi,
        "top-right": lambda c, b: b[0] == 0 and b[1] + b[3] == c.Wi and b[2] < c.Hi and b[1] > 0,
        "bottom-left": lambda c, b: b[1] == 0 and b[0] + b[2] == c.Hi and b[0] > 0 and b[3] < c.Wi,
        "bottom-right": lambda c, b: b[0] + b[2] == c.Hi and b[1] + b[3] == c.Wi and b[0] > 0 and b[1] > 0,
        "identity": lambda c, b: b[2:] == (c.Ho, c.Wo) and (c.Ho, c.Wo) != (1, 1),
    }
    for kind, pred in kinds.items():
        assert any(pred(c, b) for c in cs for b in c.boxes), kind
    # every box kind but the identity at every output size the frame cannot hold as a box; all of them where it can
    for c in (c for c in cs if c.name in ("1x1_C1", "1x9_C4", "9x1_C4_fpb5", "5x7_C3", "3x300_C1")):
        for kind, pred in kinds.items():
            if kind != "identity" or (c.Ho <= c.Hi - 2 and c.Wo <= c.Wi - 3 and (c.Ho, c.Wo) != (1, 1)):
                assert any(pred(c, b) for b in c.boxes), (c.name, kind)


def test_stem_crop_cases_hold_what_the_uint8_kernel_branches_on():
    cs = R.STEM_CROP_CASES
    assert {c.F for c in cs} == {1, 2, 11} and {c.fpb for c in cs} == {1, 5}
    for c in cs:
        assert len(c.boxes) == -(-c.F // c.fpb) and _boxes_inside(c.boxes, c.Hi, c.Wi), c.name
    wide = [c for c in cs if c.Wi >= 500]
    assert {b[3] for c in wide for b in c.boxes} >= R.STEM_CROP_WIDTHS
    ratio = sorted({b[3] / 224.0 for c in wide for b in c.boxes})
    assert any(r < 1.5 for r in ratio if r > 1) and 1.5 in ratio and any(r > 1.5 for r in ratio) and 1.0 in ratio
    assert any(b[1] + b[3] == c.Wi and b[1] > 0 for c in wide for b in c.boxes) and any(b[1] == 0 for c in wide for b in c.boxes)
    assert {c.Wi for c in cs} >= {1, 3, 4}
    assert {b[2] for c in cs for b in c.boxes} >= {1, 2}
    for c in cs:
        if c.Wi >= 4:       # the last box (the last frame's) ends on the clip's last row, and on a wide clip on its last byte
            t, l, h, w = c.boxes[(c.F - 1) // c.fpb]
            assert t + h == c.Hi, c.name
    assert any(c.boxes[(c.F - 1) // c.fpb][1] + c.boxes[(c.F - 1) // c.fpb][3] == c.Wi for c in wide)


# ---- the references against torch float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_references_agree_with_torch_float64(case):
    N, C, ay, ax = R.resize_case(case)
    x_u8, x_f, dout, _ = R.resize_inputs(case)
    ref_u8, ref_f, adj = R.resize_refs(case)
    dy = 0.0 if case[0] in R.EXACT_INDEX_AXES else R.index_error(ay[0])
    dx = 0.0 if case[1] in R.EXACT_INDEX_AXES else R.index_error(ax[0])
    for x, ref in ((x_u8, ref_u8), (x_f, ref_f)):
        want = _torch_forward(x, ay, ax).numpy()
        assert ref.shape == want.shape == (N, C, ay[3], ax[3])
        bad = R.first_bad(np.abs(ref - want), (dy + dx) * 255.0 + 1e-12)
        assert bad is None, ("forward", case, bad)
    xr = torch.from_numpy(x_f.astype(np.float64)).requires_grad_(True)
    yr = F.interpolate(xr, size=(ay[1], ax[1]), mode="bilinear", align_corners=False)[:, :, ay[2]:ay[2] + ay[3], ax[2]:ax[2] + ax[3]]
    (yr * torch.from_numpy(dout.astype(np.float64))).sum().backward()
    tol = float(np.abs(dout).max()) * (dy + dx) * (adj.n_y[:, None] + 2) * (adj.n_x[None, :] + 2) + 1e-12
    bad = R.first_bad(np.abs(adj.din - xr.grad.numpy()), tol)
    assert bad is None, ("adjoint", case, bad)
    # S bounds |din|, and is zero exactly on the source pixels no window pixel taps
    assert (np.abs(adj.din) <= adj.S * (1 + 1e-12)).all()
    assert np.array_equal(adj.S == 0, np.broadcast_to((adj.n_y[:, None] == 0) | (adj.n_x[None, :] == 0), adj.S.shape))


def test_crop_reference_agrees_with_torch_float64():
    for c in R.CROP_CASES:
        if c.N > 70:
            continue
        x_u8, _ = R.crop_inputs(c.name)
        ref, _ = R.crop_refs(c.name)
        for n in range(c.N):
            t, l, h, w = c.boxes[n // c.fpb]
            want = F.interpolate(torch.from_numpy(x_u8[n:n + 1, :, t:t + h, l:l + w].astype(np.float64)) / 255.0, size=(c.Ho, c.Wo),
                                 mode="bilinear", align_corners=False).numpy() * 255.0
            bad = R.first_bad(np.abs(ref[n:n + 1] - want), (R.index_error(h) + R.index_error(w)) * 255.0 + 1e-12)
            assert bad is None, (c.name, n, bad)
