"""CPU: the case list of tests/test_gpu_bn.py (util.bn_cases) against the launch geometry the library reports (r3m_debug_bn_geometry,
which runs the launchers' own helpers): every boundary the BatchNorm launchers of csrc/bn.hip have is in the list for both dtypes, every
BatchNorm shape behind the stem of ResNet-18 / 34 / 50 at the sweep sizes of test_resolution_plan.py falls into a class some case
covers, and the inputs the GPU module will use stay clear of the ReLU kink."""
import pytest

from test_resolution_plan import SWEEP
from util import (BN_CHANNELS, BN_FRAME_SIZES, BN_LARGE, bn_cases, bn_class, bn_geometry, bn_inputs, bn_pair_cases, bn_plan_shapes,
                  bn_possible_tails, bn_span_tail)


@pytest.fixture(scope="module")
def L():
    from r3m_amd import _lib
    return _lib.lib()


def test_geometry_query_reports_what_the_header_says(L):
    g = bn_geometry(L, 2 * 56 * 56, 64, "fp32")
    assert (g["fwd_vec"], g["fwd_span"], g["fwd_grid"]) == (4, 256, 2 * 56 * 56 * 16 // 256)
    assert (g["red_vec"], g["rpb"], g["rpp"], g["col_blocks"], g["nblk"]) == (4, 512, 16, 1, -(-2 * 56 * 56 // 512))
    assert (g["app_span"], g["slice_cap"]) == (256, 256)
    assert bn_geometry(L, 100, 2048, "fp32")["col_blocks"] == 2 and bn_geometry(L, 100, 2048, "bf16")["col_blocks"] == 1
    assert bn_geometry(L, 100, 512, "fp32")["app_span"] == 1024 and bn_geometry(L, 100, 2048, "fp32")["app_span"] == 256
    assert all(bn_geometry(L, 100, C, "bf16")["app_span"] == 1024 for C in BN_CHANNELS)
    assert [bn_geometry(L, 100, C, "bf16")["fwd_span"] for C in BN_CHANNELS] == [256] * 5 + [1024]
    # the slice count on both sides of its cap: 256 slices at C = 64, 64 at C = 2048, one slice per 16 partial rows below it
    for C, cap in ((64, 256), (2048, 64)):
        assert bn_geometry(L, 1, C, "fp32")["slice_cap"] == cap
        assert [bn_geometry(L, r, C, "fp32")["slices_of_rows"] for r in (1, 16, 17, 16 * cap - 16, 16 * cap - 15, 16 * cap, 16 * cap + 1)] == \
            [1, 1, 2, cap - 1, cap, cap, cap]
    import ctypes
    buf = (ctypes.c_int * 16)()
    assert L.r3m_debug_bn_geometry(100, 64, 0, buf, 13) == -1          # buffer too short
    assert L.r3m_debug_bn_geometry(100, 96, 0, buf, 16) == -1          # C is not a power of two
    assert L.r3m_debug_bn_geometry(0, 64, 0, buf, 16) == -1
    assert L.r3m_debug_bn_geometry(100, 64, 2, buf, 16) == -1


def test_case_list_holds_the_plan_shapes_and_stays_small(L):
    cases = bn_cases()
    keys = {(r, c, d) for (r, c, d, _) in cases}
    assert len(keys) == len(cases)
    shapes = bn_plan_shapes(L, (18, 50), BN_FRAME_SIZES, (1, 3))
    for dtype in ("fp32", "bf16"):
        assert all((r, c, dtype) in keys for (r, c) in shapes)
        assert {1, 2, 3} <= {r for (r, c, d) in keys if d == dtype}                     # layer4 of one frame at 32 x 32, 33 x 47, ...
        assert (BN_LARGE[0], BN_LARGE[1], dtype) in keys
    assert any(r % 2 == 1 and r > 3 for (r, c, d) in keys if d == "bf16")               # odd row counts in bf16
    assert max(r * c * 4 for (r, c, d) in keys) <= 64 << 20                             # the largest tensor: 64 MiB


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_case_list_has_every_boundary(L, dtype):
    cases = [(r, c) for (r, c, d, _) in bn_cases() if d == dtype]
    geo = {(r, c): bn_geometry(L, r, c, dtype) for (r, c) in cases}
    for C in BN_CHANNELS:
        mine = [(r, g) for ((r, c), g) in geo.items() if c == C]
        rpp, rpb = mine[0][1]["rpp"], mine[0][1]["rpb"]
        if rpp > 1:
            assert any(r < rpp for r, g in mine), f"C={C}: no case with fewer rows than one pass ({rpp})"
        for rem in (0, 1, rpb - 1):
            assert any(r % rpb == rem and g["nblk"] > 1 for r, g in mine), f"C={C}: no multi-block case with rows % {rpb} == {rem}"
        assert any(g["nblk"] == 1 and r < rpb for r, g in mine)
        # the span-1024 launches: every tail kind of the last block
        for which in ("fwd", "app"):
            vec, span = mine[0][1][which + "_vec"], mine[0][1][which + "_span"]
            if span == 256:
                continue
            tails = {bn_span_tail(r, C, vec, span) for r, g in mine if g[which + "_grid"] > 1}
            assert {"full", "one", "all_but_one", "mid_walk"} <= tails, f"C={C} {which}: span {span} tails {tails}"
    if dtype == "fp32":
        assert any(g["col_blocks"] == 2 and g["nblk"] > 1 for g in geo.values())        # C = 2048: the second column block
    else:
        assert bn_span_tail(1025, 8, 8, 1024) == "one" and bn_span_tail(2047, 8, 8, 1024) == "all_but_one"   # literally one vector
        assert (1025, 8) in geo and (2047, 8) in geo and geo[(1025, 8)]["app_span"] == 1024
    assert any(g["slices"] > 4 for g in geo.values())                                   # several slices live (the large case)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pair_case_list_has_every_tail_of_the_paired_second_pass(L, dtype):
    """bn_bwd_apply_kernel's NB = 2 instantiations walk their span on their own: per channel count the multi-block cases of the pair list
    end in exactly the tail kinds that can exist for that (C, dtype) (util.bn_possible_tails: up to all five for span 1024; full, one,
    all_but_one and part for span 256, only full where one row already fills the span); one row fits one block unless it is longer
    than the span; rows 1..3 and the large case are there"""
    pairs = [(r, c) for (r, c, d) in bn_pair_cases() if d == dtype]
    assert all((r, c, dtype) in {(a, b, d) for (a, b, d, _) in bn_cases()} for (r, c) in pairs)
    for C in BN_CHANNELS:
        mine = [(r, bn_geometry(L, r, C, dtype)) for (r, c) in pairs if c == C]
        vec, span = mine[0][1]["app_vec"], mine[0][1]["app_span"]
        tails = {bn_span_tail(r, C, vec, span) for r, g in mine if g["app_grid"] > 1}
        assert tails == bn_possible_tails(C, vec, span), f"C={C}: span {span} tails {tails}"
        assert any(g["app_grid"] == 1 for r, g in mine) == (C // vec <= span)
    assert {1, 2, 3} <= {r for (r, c) in pairs} and (BN_LARGE[0], BN_LARGE[1]) in pairs


@pytest.mark.parametrize("size", [18, 34, 50])
def test_every_swept_batchnorm_shape_is_in_a_covered_class(L, size):
    covered = {bn_class(L, r, c, d) for (r, c, d, _) in bn_cases()}
    for (rows, C) in bn_plan_shapes(L, (size,), SWEEP, (1, 3)):
        for dtype in ("fp32", "bf16"):
            assert bn_class(L, rows, C, dtype) in covered, (size, rows, C, dtype, bn_class(L, rows, C, dtype))


def test_inputs_stay_clear_of_the_relu_kink():
    """the bf16 sign check and the recomputed masks leave out elements with |t| <= 1e-4: at most 0.1 % of a case may be left out, judged
    on the float64 reference alone, for the very inputs the GPU module builds (the construction moves them all away)"""
    for (rows, C, dtype, _) in bn_cases():
        for mode in ("plain", "identity", "downsample"):
            assert bn_inputs(rows, C, dtype, mode)["near"] <= 1e-3, (rows, C, dtype, mode)
