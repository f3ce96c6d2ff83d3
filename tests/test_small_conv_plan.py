"""not gpu: the routing rule and the decomposition of the small-M split-K forward (csrc/conv_small.hip, small_conv_plan) through
r3m_debug_conv_small_plan and r3m_resnet_conv_info — a pure function of the launch geometry, nothing is launched. For every convolution
of ResNet-18/34/50 at 224 x 224 and 1, 8 and 16 frames: which launches the rule takes, their tile, S and grid (pinned in
tests/small_conv_cases.py), that the slices cover K exactly, and that the workspaces hold what the kernel writes."""
import pytest

from small_conv_cases import AR, GPU_CASES, PINNED, conv_small_plan, forced_splits, resnet_convs


@pytest.fixture(scope="module")
def L():
    from r3m_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("size,F", sorted(PINNED))
def test_rule_tile_split_and_grid_are_pinned(L, size, F):
    convs, plan_ws = resnet_convs(L, size, F)
    pins = PINNED[(size, F)]
    assert 0 not in pins, "the stem is not this kernel's"
    ctr_sum, slab_max = 0, 0
    for i, case in enumerate(convs):
        if i == 0:
            continue
        p = conv_small_plan(L, case)
        assert bool(p["take"]) == (i in pins), (i, case, p)
        if not p["take"]:
            continue
        assert (p["bm"], p["S"], p["grid"]) == pins[i], (i, case, p)
        N, Hi, Wi, Ci, Co, k, s, pad = case
        M = N * ((Hi + 2 * pad - k) // s + 1) * ((Wi + 2 * pad - k) // s + 1)
        assert p["bn"] == 64 and p["tiles_n"] * 64 == Co and p["tiles_m"] == -(-M // p["bm"]) and p["bm"] in (16, 32, 64)
        assert p["grid"] == p["tiles_m"] * p["tiles_n"] * p["S"]
        # the slices cover K exactly, none is empty
        assert p["nch"] == k * k * Ci // 32
        assert (p["S"] - 1) * p["cps"] < p["nch"] <= p["S"] * p["cps"], p
        # the decomposition rule: one round of blocks on 256 CUs, no slice shorter than 4 chunks, at most 32 slices
        assert p["grid"] <= 256 and p["S"] <= 32 and (p["S"] == 1 or p["cps"] >= 4), p
        # the workspace holds the slabs and a ticket per tile
        tickets = p["tiles_m"] * p["tiles_n"] * 4
        need = p["S"] * M * Co * 4 + tickets
        got = L.r3m_conv2d_small_workspace_bytes(*case, 0)
        assert need <= got, (case, need, got)
        padded = p["S"] * p["tiles_m"] * p["bm"] * Co * 4
        assert got == padded + -(-tickets // 256) * 256           # what the kernel really indexes: whole tiles of rows
        ctr_sum += -(-tickets // 256) * 256
        slab_max = max(slab_max, padded)
    assert plan_ws == ctr_sum + slab_max, "r3m_resnet_inference_workspace_bytes: every launch's tickets, then the largest slab area"


@pytest.mark.parametrize("size", [18, 34, 50])
def test_rule_takes_nothing_at_1280_frames(L, size):
    convs, plan_ws = resnet_convs(L, size, 1280)
    assert not any(conv_small_plan(L, c)["take"] for c in convs[1:])
    assert plan_ws == 0


def test_bf16_plans_need_no_workspace(L):
    h = L.r3m_resnet_create_dt(50, 1, 1)
    assert h and L.r3m_resnet_inference_workspace_bytes(h) == 0
    L.r3m_resnet_destroy(h)


@pytest.mark.parametrize("case,flag_sets", GPU_CASES)
def test_gpu_cases_are_taken_or_forced(L, case, flag_sets):
    """every case of tests/test_gpu_small_conv.py is a shape the kernel takes; its forced splits are accepted, differ, and contain a
    ragged last slice and a slice boundary inside a tap"""
    for fl in flag_sets:
        p = conv_small_plan(L, case, fl)
        assert p["grid"] > 0, (case, fl)
    p = conv_small_plan(L, case)
    splits, ragged, inside = forced_splits(L, case)
    assert splits[0] == 1 and p["max_split"] in splits and all(1 <= S <= p["max_split"] for S in splits)
    cpt = case[3] // 32
    if p["nch"] > 2:
        assert ragged is not None and p["nch"] % ragged
    if ragged is not None:
        cps = -(-p["nch"] // ragged)
        assert 0 < p["nch"] - (ragged - 1) * cps < cps or (ragged - 1) * cps >= p["nch"]   # the last non-empty slice is shorter
    if case[5] == 3:
        assert inside is not None and -(-p["nch"] // inside) % cpt, "no slice boundary inside a tap"
    for S in splits:
        assert L.r3m_conv2d_small_workspace_bytes(*case, S) >= S * p["tiles_m"] * p["bm"] * case[4] * 4


def test_shapes_the_kernel_does_not_take(L):
    for case, fl in [((1, 7, 7, 48, 64, 3, 1, 1), AR), ((1, 7, 7, 64, 96, 3, 1, 1), AR), ((1, 7, 7, 64, 64, 5, 1, 2), AR),
                     ((1, 7, 7, 64, 64, 3, 3, 1), AR), ((1, 7, 7, 64, 64, 3, 1, 1), 16), ((1, 7, 7, 64, 64, 3, 1, 1), 128 | 1)]:
        p = conv_small_plan(L, case, fl)
        assert not any(p.values()), (case, fl, p)
    assert L.r3m_conv2d_small_workspace_bytes(1, 7, 7, 48, 64, 3, 1, 1, 0) == 0
