"""not gpu: the few-row Linear (r3m_linear_fwd_small) has no planner of its own: its plan IS small_conv_plan of the 1 x 1 geometry
(csrc/conv_small.hip). Checked here without a launch: the two debug entries agree for every case and flag set, the refusals carry
messages, the forced splits of every case, the float64 references of tests/test_gpu_linear_small.py meet the conditions that test
asserts, and the routing of the reward head's and distilbert-base's Linears."""
import ctypes as C

import pytest

from linear_small_cases import (B, BG, BR, GELU, GPU_CASES, LINEAR_FLAGS, RELU, geom, head_linears, linear_small_plan, reference,
                                text_linears)
from small_conv_cases import AR, conv_small_plan, forced_splits
from util import assert_range


@pytest.fixture(scope="module")
def L():
    from r3m_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("case,flag_sets", GPU_CASES)
def test_linear_plan_is_the_conv_plan_of_the_1x1_geometry(L, case, flag_sets):
    for fl in LINEAR_FLAGS:
        p = linear_small_plan(L, case, fl)
        assert p == conv_small_plan(L, geom(case), fl), (case, fl)
        assert p["grid"] > 0 and p["grid"] == p["tiles_m"] * p["tiles_n"] * p["S"], (case, fl, p)
    M, K, N = case
    p = linear_small_plan(L, case, flag_sets[0])
    assert p == conv_small_plan(L, geom(case), AR), "the store does not enter the plan"
    assert p["bm"] == (16 if M <= 16 else 32 if M <= 32 else 64) and p["tiles_m"] == -(-M // p["bm"]) and p["tiles_n"] * 64 == N
    assert p["nch"] == K // 32 and (p["S"] - 1) * p["cps"] < p["nch"] <= p["S"] * p["cps"]
    need = L.r3m_linear_small_workspace_bytes(M, K, N, 0)
    tickets = -(-p["tiles_m"] * p["tiles_n"] * 4 // 256) * 256
    assert need == p["S"] * p["tiles_m"] * p["bm"] * N * 4 + tickets
    assert need == L.r3m_conv2d_small_workspace_bytes(*geom(case), 0)


def test_pinned_tiles_and_slices(L):
    """the decomposition of the cases the list names for it"""
    pins = {(1, 4864, 1024): (16, 16), (17, 768, 768): (32, 6), (33, 768, 3072): (64, 5), (65, 256, 512): (64, 2), (130, 512, 256): (64, 4),
            (3, 32, 64): (16, 1)}
    for case, (bm, S) in pins.items():
        p = linear_small_plan(L, case, B)
        assert (p["bm"], p["S"]) == (bm, S), (case, p)
    p = linear_small_plan(L, (3, 32, 64), BR)
    assert p["nch"] == 1 and p["max_split"] == 1 and p["take"] == 0, "one chunk: S = 1 only, below the rule's four chunks"
    p = linear_small_plan(L, (2, 160, 64), BR)
    assert p["nch"] == 5 and p["max_split"] == 5


def test_refusals_carry_messages(L):
    buf = (C.c_int * 64)()
    p = C.addressof(buf)

    def lin(M, K, N, flags, split=0):
        return L.r3m_linear_fwd_small(p, p, p, p, M, K, N, flags, split, None, 0, None)

    assert lin(4, 48, 64, BR) != 0 and b"K must be a multiple of 32" in L.r3m_last_error()
    assert lin(4, 64, 96, BR) != 0 and b"N must be a multiple of 64" in L.r3m_last_error()
    assert lin(0, 64, 64, BR) != 0 and b"M must be" in L.r3m_last_error()
    assert lin(65537, 64, 64, BR) != 0 and b"more rows" in L.r3m_last_error()
    for fl in (0, RELU, GELU, B | 1, B | RELU | GELU, RELU | GELU):
        assert lin(4, 64, 64, fl) != 0 and b"flags" in L.r3m_last_error(), fl
    for fl in (128, 128 | 16, 128 | 2 | 16):                 # a convolution's store on the Linear entry
        assert lin(4, 64, 64, fl) != 0 and b"flags" in L.r3m_last_error() and b"r3m_conv2d_fwd_affine_small" in L.r3m_last_error(), fl
        out = (C.c_int * 10)(*([7] * 10))
        assert L.r3m_debug_linear_small_plan(4, 64, 64, fl, out, 10) == 10 and not any(out)
    for fl in LINEAR_FLAGS:                                  # ... and the reverse
        rc = L.r3m_conv2d_fwd_affine_small(p, p, p, p, p, 4, 1, 1, 64, 64, 1, 1, 0, fl, 0, None, 0, None)
        assert rc != 0 and b"flags" in L.r3m_last_error() and b"r3m_linear_fwd_small" in L.r3m_last_error(), fl
    assert lin(4, 256, 64, BR, 9) != 0 and b"split" in L.r3m_last_error()          # 8 chunks: at most 8 slices
    assert lin(4, 256, 64, BR, 2) != 0 and b"workspace" in L.r3m_last_error()      # S > 1 and no workspace
    assert L.r3m_linear_small_workspace_bytes(4, 48, 64, 0) == 0
    out = (C.c_int * 10)(*([7] * 10))
    assert L.r3m_debug_linear_small_plan(4, 48, 64, BR, out, 10) == 10 and not any(out)
    assert L.r3m_debug_linear_small_plan(4, 64, 64, BR, out, 9) == -1


@pytest.mark.parametrize("case,flag_sets", GPU_CASES)
def test_forced_splits(L, case, flag_sets):
    g = geom(case)
    p = linear_small_plan(L, case, flag_sets[0])
    splits, ragged, inside = forced_splits(L, g)
    assert splits[0] == 1 and p["max_split"] in splits and all(1 <= S <= p["max_split"] for S in splits)
    assert len(set(splits)) == len(splits)
    if p["nch"] > 2:
        assert ragged is not None and p["nch"] % ragged
    if p["nch"] == 1:
        assert splits == [1]
    for S in splits:
        assert L.r3m_linear_small_workspace_bytes(*case, S) >= S * p["tiles_m"] * p["bm"] * case[2] * 4


@pytest.mark.parametrize("case,flags", [(c, fl) for c, fls in GPU_CASES for fl in fls])
def test_references_meet_the_gpu_tests_conditions(case, flags):
    bias, pre, ref, terms = reference(case, flags)
    assert_range(ref, terms, f"linear {case} flags {flags}")
    assert float(bias.abs().max()) > 0
    if flags & RELU:
        zeros = float((ref == 0).double().mean())
        assert 0.2 <= zeros <= 0.8, (case, zeros)
    if flags & GELU:
        sd = float(pre.std())
        assert 0.3 <= sd <= 3.0, (case, sd)


@pytest.mark.parametrize("R", [1, 4, 16])
@pytest.mark.parametrize("D", [512, 2048])
def test_every_linear_of_the_head_is_taken(L, R, D):
    for case, fl in head_linears(R, D):
        p = linear_small_plan(L, case, fl)
        assert p["take"] == 1 and p["bm"] == 16 and p["grid"] <= 256, (case, p)


@pytest.mark.parametrize("R", [8, 256])
def test_every_linear_of_distilbert_base_is_taken(L, R):
    for case, fl in text_linears(R):
        p = linear_small_plan(L, case, fl)
        assert p["take"] == 1 and p["grid"] <= 256, (case, p)


def test_the_4096_row_text_case_stays_where_it_is(L):
    assert not any(linear_small_plan(L, case, fl)["take"] for case, fl in text_linears(4096))
