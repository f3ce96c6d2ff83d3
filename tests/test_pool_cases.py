"""CPU: the case lists of tests/test_gpu_pool_edges.py (tests/pool_cases.py) against the launch geometry the library reports
(r3m_debug_pool_geometry: the struct the launchers of csrc/bn_pool.hip launch from) -- every named condition has a case on each side of
its boundary in both dtypes, the reduce never writes more partial rows than r3m_bn_workspace_bytes lays out -- and the float64
references against F.max_pool2d(return_indices=True), with the inputs' exactness claims checked value by value."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_cases as pc

DTYPES = ("fp32", "bf16")
ALL_SHAPES = sorted({s for _, s in pc.FUSED_CASES} | {s for _, s in pc.MAXPOOL_CASES})


@pytest.fixture(scope="module")
def L():
    from r3m_amd import _lib
    return _lib.lib()


def test_geometry_query_reports_what_the_comments_say(L):
    """the 224 x 224 stem (y [N, 112, 112, 64]) of 32 frames: a reduce / apply block owns all Wo x CV items of a quad row with one thread
    each (896 in fp32, 448 in bf16: "all of them when they fit"), 8 quad rows per reduce block, one quad row per apply block; the bf16
    forward walks segments of POOL_SEG = 8 output rows, the fp32 forward gives every (pixel, 4 channels) output a thread of a 256-block"""
    g = pc.pool_geometry(L, 32, 112, 112, 64, "fp32")
    assert (g["Ho"], g["Wo"], g["V"]) == (56, 56, 4)
    assert (g["fwd_rows"], g["fwd_segs"], g["fwd_blocks"], g["fwd_threads"], g["fwd_items"]) == (0, 0, 32 * 56 * 56 * 16 // 256, 256, 256)
    assert (g["rq"], g["red_blocks"], g["red_threads"], g["red_items"], g["per_cv"], g["G"]) == (8, 32 * 56 // 8, 896, 896, 56, 8)
    assert g["red_lds"] == 2 * 896 * 16 and g["red_cap"] == -(-32 * 112 * 112 // 512)
    assert (g["app_blocks"], g["app_threads"]) == (32 * 56, 896)
    g = pc.pool_geometry(L, 32, 112, 112, 64, "bf16")
    assert (g["fwd_rows"], g["fwd_segs"], g["fwd_blocks"], g["fwd_threads"], g["fwd_items"], g["V"]) == (1, 7, 32 * 7, 448, 448, 8)
    assert (g["rq"], g["red_blocks"], g["red_threads"], g["red_items"], g["per_cv"], g["G"]) == (8, 32 * 56 // 8, 448, 448, 56, 8)
    assert g["red_lds"] == 2 * 2 * 448 * 16 and (g["app_blocks"], g["app_threads"]) == (32 * 56, 448)
    # "1024 (a multiple of CV <= 256)" once the items no longer fit, and the rounding up to 64 below that
    assert pc.pool_geometry(L, 1, 3, 400, 64, "fp32")["red_threads"] == 1024
    assert pc.pool_geometry(L, 1, 3, 5, 64, "fp32")["red_threads"] == 64 and pc.pool_geometry(L, 1, 3, 9, 64, "fp32")["red_threads"] == 128
    # "more [than 8 quad rows per block] when that would give more partial rows than the plain fp32 reduce of the same tensor writes"
    g = pc.pool_geometry(L, 3, 40, 16, 64, "fp32")
    assert (g["rq"], g["red_blocks"], g["red_cap"]) == (15, 4, 4)
    # (8 quad rows hold 16 Wi pixels against the 512 of a plain reduce block at C = 64: maps narrower than 32, up to the roundings)
    assert all(pc.pool_geometry(L, 3, 40, W, 64, "bf16")["rq"] > 8 for W in range(4, 30))
    assert all(pc.pool_geometry(L, 3, 40, W, 64, "bf16")["rq"] == 8 for W in range(32, 64))


def test_geometry_query_refusals(L):
    buf = (ctypes.c_int * 20)()
    assert L.r3m_debug_pool_geometry(2, 9, 7, 64, 0, buf, 18) == 18
    assert L.r3m_debug_pool_geometry(2, 9, 7, 64, 0, buf, 17) == -1 and b"18 ints" in L.r3m_last_error()      # buffer too short
    assert L.r3m_debug_pool_geometry(2, 9, 7, 64, 0, None, 18) == -1
    assert L.r3m_debug_pool_geometry(2, 9, 7, 64, 2, buf, 18) == -1 and b"dtype" in L.r3m_last_error()
    assert L.r3m_debug_pool_geometry(2, 9, 7, 64, -1, buf, 18) == -1
    for bad in ((0, 9, 7, 64), (2, 0, 7, 64), (2, 9, 0, 64), (2, 9, 7, 0), (2, 9, 7, 12), (2, 9, 7, -8)):
        assert L.r3m_debug_pool_geometry(*bad, 1, buf, 18) == -1, bad
    # channel counts the backward refuses still answer for the forward, with the backward's figures 0
    for C in (24, 2048):
        g = pc.pool_geometry(L, 2, 9, 7, C, "bf16")
        assert g["fwd_blocks"] >= 1 and all(g[k] == 0 for k in pc.GEOM_FIELDS[7:17]), g
    assert L.r3m_abi_version() == 1


def test_case_lists_are_distinct_and_tiny():
    for cases in (pc.FUSED_CASES, pc.MAXPOOL_CASES):
        assert len({n for n, _ in cases}) == len(cases) == len({s for _, s in cases})
        for _, (N, Hi, Wi, C) in cases:
            assert N * Hi * Wi * C <= pc.SIZE_CAP
    assert {N for _, (N, _, _, _) in pc.MAXPOOL_CASES} == {1, 2, 3} and {C for _, (_, _, _, C) in pc.MAXPOOL_CASES} == {4, 64}
    totals = [(N * Ho * Wo * C // 4, N * Hi * Wi * C // 4) for _, (N, Hi, Wi, C) in pc.MAXPOOL_CASES for Ho, Wo in [pc.out_hw(Hi, Wi)]]
    for side in (0, 1):          # forward / backward launch: one block, several with a ragged last one, several full ones
        assert any(t[side] < 256 for t in totals) and any(t[side] > 256 and t[side] % 256 for t in totals)
        assert any(t[side] > 256 and t[side] % 256 == 0 for t in totals)
    assert {(Hi, Wi) for _, (_, Hi, Wi, _) in pc.MAXPOOL_CASES} >= {(1, 1), (1, 7), (7, 1), (2, 2), (2, 9), (3, 3)}


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_backward_condition_has_a_case(L, dtype):
    cases = [(n, s, pc.pool_geometry(L, *s, dtype)) for n, s in pc.FUSED_CASES if pc.has_backward(s[3])]
    for name, pred in pc.BACKWARD_CONDITIONS.items():
        assert any(pred(g, s) for _, s, g in cases), f"{dtype}: no fused case with {name}"
    # the cases the issue names, at the figures it names
    by = {n: g for n, _, g in cases}
    assert (by["rq_15"]["rq"], by["rq_15"]["red_blocks"]) == (15, 4) and (by["rq_8_cap"]["rq"], by["rq_8_cap"]["red_blocks"]) == (8, 5)
    assert by["trips_1024_" + dtype]["red_items"] == 1024 and by["trips_1040_fp32" if dtype == "fp32" else "trips_1032_bf16"]["red_items"] > 1024
    assert [by[n]["per_cv"] for n in ("per_cv_1", "per_cv_2", "per_cv_3")] == [1, 2, 3]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_forward_condition_has_a_case(L, dtype):
    cases = [(s, pc.pool_geometry(L, *s, dtype)) for _, s in pc.FUSED_CASES]
    for name, pred in pc.FORWARD_CONDITIONS[dtype].items():
        assert any(pred(g, s) for s, g in cases), f"{dtype}: no fused case with {name}"
    for s, g in cases:          # which kernel: the row-walking one for bf16 and a power of two up to 2048, never for fp32
        assert g["fwd_rows"] == int(dtype == "bf16" and s[3] & (s[3] - 1) == 0 and s[3] <= 2048)
        assert g["fwd_segs"] == (-(-g["Ho"] // pc.POOL_SEG) if g["fwd_rows"] else 0)


def _check_launch_invariants(L, g, shape, dtype):
    N, Hi, Wi, C = shape
    CV = C // g["V"]
    assert (g["Ho"], g["Wo"]) == pc.out_hw(Hi, Wi) and g["V"] == (4 if dtype == "fp32" else 8)
    if g["fwd_rows"]:
        assert g["fwd_items"] == g["Wo"] * CV and g["fwd_blocks"] == N * g["fwd_segs"]
        assert CV <= g["fwd_threads"] <= 1024 and g["fwd_threads"] % CV == 0 and g["fwd_threads"] % 64 == 0
        assert g["fwd_threads"] >= min(g["fwd_items"], 1024)
    else:
        assert g["fwd_threads"] == 256 and g["fwd_blocks"] == -(-N * g["Ho"] * g["Wo"] * CV // 256)
    if not pc.has_backward(C):
        assert g["red_blocks"] == 0 and g["app_blocks"] == 0
        return
    # the reduce writes red_blocks partial rows [2][C] into the workspace laid out for red_cap of them
    assert 1 <= g["red_blocks"] <= g["red_cap"], (shape, g)
    assert L.r3m_bn_workspace_bytes(N * Hi * Wi, C) >= g["red_blocks"] * 2 * C * 4
    assert g["rq"] >= 8 and (g["red_blocks"] - 1) * g["rq"] < N * g["Ho"] <= g["red_blocks"] * g["rq"]
    # a thread's channel vector is loop-invariant: the block is a whole number of channel-vector groups, at least one
    for threads in (g["red_threads"], g["app_threads"]):
        assert CV <= threads <= 1024 and threads % CV == 0 and threads % 64 == 0 and threads >= min(g["red_items"], 1024)
    assert g["red_items"] == g["Wo"] * CV and g["per_cv"] == g["red_threads"] // CV and g["G"] == min(g["per_cv"], 8)
    assert g["red_lds"] == 2 * (g["V"] // 4) * g["red_threads"] * 16 <= 65536
    assert g["app_blocks"] == N * g["Ho"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_launches_fit_their_buffers(L, dtype):
    """every case, and a sweep of small shapes around them: blocks <= cap for the reduce (so the workspace r3m_bn_workspace_bytes sizes
    is enough), threads a multiple of CV and >= CV"""
    for _, s in pc.FUSED_CASES:
        _check_launch_invariants(L, pc.pool_geometry(L, *s, dtype), s, dtype)
    for C in (8, 16, 64, 512, 1024):
        for N in (1, 2, 5):
            for Hi in (1, 2, 3, 16, 17, 41, 112):
                for Wi in (1, 2, 3, 15, 31, 32, 64, 130, 258):
                    _check_launch_invariants(L, pc.pool_geometry(L, N, Hi, Wi, C, dtype), (N, Hi, Wi, C), dtype)


# ---- the references --------------------------------------------------------------------------------------------------------------------
def _codes_from_torch(z):
    """first-maximum window codes from F.max_pool2d(return_indices=True) in float64 on the CPU (flat input index -> 3 i + j)"""
    N, Hi, Wi, C = z.shape
    p, idx = F.max_pool2d(torch.tensor(z.transpose(0, 3, 1, 2)), 3, 2, 1, return_indices=True)
    Ho, Wo = p.shape[2], p.shape[3]
    yy, xx = idx // Wi, idx % Wi
    i = yy - (2 * torch.arange(Ho).view(1, 1, Ho, 1) - 1)
    j = xx - (2 * torch.arange(Wo).view(1, 1, 1, Wo) - 1)
    assert bool(((i >= 0) & (i < 3) & (j >= 0) & (j < 3)).all())
    return p.permute(0, 2, 3, 1).numpy(), (3 * i + j).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("name,shape", pc.FUSED_CASES + pc.MAXPOOL_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_references_agree_with_torch(name, shape):
    """pooled values, first-maximum codes and the scattered gradient against F.max_pool2d + autograd in float64, on the tied lattice
    inputs the GPU module uses"""
    N, Hi, Wi, C = shape
    fused = (name, shape) in pc.FUSED_CASES
    case = pc.fused_case(shape) if fused else pc.maxpool_case(shape)
    p_t, code_t = _codes_from_torch(case["z"])
    assert np.array_equal(case["p"], p_t) and np.array_equal(case["code"], code_t)
    zr = torch.tensor(case["z"].transpose(0, 3, 1, 2)).requires_grad_(True)
    F.max_pool2d(zr, 3, 2, 1).backward(torch.tensor(case["dp"].transpose(0, 3, 1, 2)))
    dz = pc.maxpool_bwd_ref(case["dp"], case["code"], Hi, Wi)
    assert np.array_equal(dz, zr.grad.permute(0, 2, 3, 1).numpy())
    if not fused:
        assert np.array_equal(dz, case["dz"])


def _bf16_exact(a):
    t = torch.tensor(a)
    return bool(torch.equal(t.to(torch.bfloat16).double(), t)) and not bool(np.signbit(a[a == 0]).any())


@pytest.mark.parametrize("name,shape", pc.FUSED_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_fused_lattice_is_exact_and_tied(name, shape):
    """every lattice tensor equals its own bf16 round trip and holds no negative zero; the eval-mode references equal their float32
    casts; the case holds tied positive windows, all-zero windows and pixels that are the maximum of 1, 2 and 4 windows"""
    N, Hi, Wi, C = shape
    c = pc.fused_case(shape)
    for k in ("y", "coef", "t", "z", "p", "dp", "g", "yhat", "dy"):
        assert _bf16_exact(c[k]), k
    b0, b1 = pc.lattice_bases(C)
    assert _bf16_exact(b0) and _bf16_exact(b1)
    for k in ("dy", "dbeta", "dgamma"):
        assert np.array_equal(c[k].astype(np.float32).astype(np.float64), c[k]), k
    assert np.array_equal((c["dgamma"] + b0).astype(np.float32).astype(np.float64), c["dgamma"] + b0)
    assert np.array_equal((c["dbeta"] + b1).astype(np.float32).astype(np.float64), c["dbeta"] + b1)
    Ho, Wo = pc.out_hw(Hi, Wi)
    s = pc.tie_stats(c["z"])
    assert s["all_zero"] > 0 and s["hit1"] > 0, s
    # pixels with t exactly 0 that a pooled gradient reaches (the first tap of an all-zero window): the mask's strict t > 0 drops it
    assert int(((c["t"] == 0) & (pc.maxpool_bwd_ref(c["dp"], c["code"], Hi, Wi) != 0)).sum()) > 0
    if Hi * Wi > 1:             # a window of a 1 x 1 map has one tap: nothing can tie
        assert s["tied_positive"] > 0, s
        assert s["tied"] > 0.5 * s["windows"] or min(Hi, Wi) < 5, s          # most windows of a map with full 3 x 3 windows
    if Ho * Wo >= 2:
        assert s["hit2"] > 0, s
    if Ho >= 2 and Wo >= 2:
        assert s["hit4"] > 0, s


@pytest.mark.parametrize("name,shape", pc.MAXPOOL_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_maxpool_lattice_is_exact_and_tied(name, shape):
    N, Hi, Wi, C = shape
    c = pc.maxpool_case(shape)
    for k in ("z", "p", "dp", "dz"):
        assert _bf16_exact(c[k]), k
    Ho, Wo = pc.out_hw(Hi, Wi)
    s = pc.tie_stats(c["z"])
    assert s["hit1"] > 0 and s["all_zero"] > 0, s
    if Hi * Wi > 1:
        assert s["tied_positive"] > 0 and s["tied"] > 0, s
    if Ho * Wo >= 2:
        assert s["hit2"] > 0, s
    if Ho >= 2 and Wo >= 2:
        assert s["hit4"] > 0, s
