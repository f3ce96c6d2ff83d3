"""not gpu: the split-K workspace of the few-row kernel (SmallLaunchSet, csrc/conv_small.hip) has five callers, and each reports its size
through an entry of its own; callers allocate exactly that much. The sizes are pinned here against literal tables.

How the tables were produced: from the library of the commit BEFORE the five callers were moved onto the one launch set (each then
laid its workspace out by hand), built with `tools/build_ab.sh HEAD` and loaded with R3M_HIP_LIB=r3m_amd/lib/libr3m_hip_base.so; a
script called the five `*_workspace_bytes` entries for the argument tuples below and printed the dictionaries. Never regenerate them
from the code under test: a change of the routing rule changes them on purpose, and then the new values come from reasoning about
the rule (ticket bytes: 4 per tile, padded to 256, per taken launch; slab bytes: the largest S * tiles_m * bm * Co * 4 of a call).

Covered: every case of small_conv_cases.py and linear_small_cases.py at split 0 and at its forced splits; the reward head at
R in {1, 5, 16, 17} for the sizes of test_gpu_reward_infer.py and a refused size; the text model at the small dims of test_text_plan.py
for (B, T) from every Linear taken to none taken; ResNet-18/34/50 fp32 at 1 and 8 frames, ResNet-18 at one 64 x 64 frame (the plan
of test_gpu_small_workspace.py), and a bf16 plan, which has no few-row launches."""
import ctypes as C

import pytest

import linear_small_cases as lc
import small_conv_cases as sc

# (N, Hi, Wi, Ci, Co, k, stride, pad) -> {split: r3m_conv2d_small_workspace_bytes}
CONV = {
    (1, 7, 7, 512, 512, 3, 1, 1): {0: 3801344, 1: 131328, 2: 262400, 32: 4194560, 5: 655616},
    (3, 1, 1, 512, 512, 3, 1, 1): {0: 950528, 1: 33024, 2: 65792, 32: 1048832, 5: 164096},
    (1, 7, 7, 512, 2048, 1, 1, 0): {0: 2097408, 1: 524544, 2: 1048832, 16: 8388864, 3: 1573120},
    (1, 7, 7, 2048, 512, 1, 1, 0): {0: 2097408, 1: 131328, 2: 262400, 32: 4194560, 3: 393472},
    (2, 14, 14, 256, 256, 3, 1, 1): {0: 4129024, 1: 459008, 2: 917760, 32: 14680320, 5: 2294016},
    (1, 13, 10, 256, 256, 3, 2, 1): {0: 1179904, 1: 65792, 2: 131328, 32: 2097408, 5: 327936},
    (1, 10, 13, 128, 128, 3, 2, 1): {0: 295168, 1: 33024, 2: 65792, 32: 1048832, 5: 164096},
    (2, 13, 11, 1024, 2048, 1, 2, 0): {0: 4194560, 1: 1048832, 2: 2097408, 32: 33554688, 3: 3145984},
    (1, 20, 12, 64, 128, 1, 2, 0): {0: 33024, 1: 33024, 2: 65792},
    (1, 56, 56, 64, 64, 3, 1, 1): {0: 3211520, 1: 803072, 2: 1605888, 18: 14450944, 4: 3211520},
    (1, 5, 5, 128, 64, 3, 1, 1): {0: 73984, 1: 8448, 2: 16640, 32: 262400, 5: 41216},
    (1, 7, 7, 48, 64, 1, 1, 0): {0: 0},               # refused: Ci no multiple of 32
    (1, 7, 7, 64, 64, 5, 1, 2): {0: 0},               # refused: k = 5
}
# (M, K, N) -> {split: r3m_linear_small_workspace_bytes}
LINEAR = {
    (1, 4864, 1024): {0: 1048832, 1: 65792, 2: 131328, 32: 2097408, 3: 196864},
    (1, 1024, 1024): {0: 524544, 1: 65792, 2: 131328, 32: 2097408, 3: 196864},
    (5, 1792, 64): {0: 57600, 1: 4352, 2: 8448, 32: 131328, 3: 12544},
    (16, 768, 2304): {0: 884992, 1: 147712, 2: 295168, 24: 3539200, 5: 737536},
    (17, 768, 768): {0: 590080, 1: 98560, 2: 196864, 24: 2359552, 5: 491776},
    (33, 768, 3072): {0: 3932416, 1: 786688, 2: 1573120, 24: 18874624, 5: 3932416},
    (8, 3072, 768): {0: 983296, 1: 49408, 2: 98560, 32: 1573120, 5: 246016},
    (65, 256, 512): {0: 524544, 1: 262400, 2: 524544, 8: 2097408, 3: 786688},
    (130, 512, 256): {0: 786688, 1: 196864, 2: 393472, 16: 3145984, 3: 590080},
    (3, 32, 64): {0: 4352, 1: 4352},
    (2, 160, 64): {0: 4352, 1: 4352, 2: 8448, 5: 20736, 3: 12544},
    (4, 48, 64): {0: 0},                              # refused: K no multiple of 32
    (0, 64, 64): {0: 0},                              # refused: no rows
}
# (D, hidden, lang_dim) -> {R: r3m_langrew_infer_workspace_bytes}
LANGREW = {
    (64, 64, 32): {1: 5632, 5: 10240, 16: 22784, 17: 28160},
    (512, 1024, 768): {1: 933888, 5: 995328, 16: 1164288, 17: 2097152},
    (2048, 1024, 768): {1: 1077248, 5: 1187840, 16: 1491968, 17: 2568192},
    (48, 64, 32): {5: 0},                             # refused: D no multiple of 32
}
# (vocab, max_pos, dim, n_layers, n_heads, ffn) -> {(B, T): r3m_text_small_workspace_bytes}
TEXT = {
    (64, 128, 256, 2, 4, 512): {(1, 1): 107520, (1, 2): 114688, (3, 5): 207872, (5, 17): 1397760, (8, 7): 796672, (16, 128): 18878464,
                                (33, 128): 30277632, (64, 128): 58720256},
    (59, 32, 768, 1, 4, 256): {(1, 1): 907264, (2, 8): 1229824, (8, 7): 4744192, (64, 32): 48235008, (512, 32): 352321536},
}
# r3m_resnet_create_hw's (size, frames, dtype, H, W) -> r3m_resnet_inference_workspace_bytes
RESNET = {
    (18, 1, 0, 224, 224): 3936768,
    (18, 8, 0, 224, 224): 3677952,
    (34, 1, 0, 224, 224): 3940864,
    (34, 8, 0, 224, 224): 3686656,
    (50, 1, 0, 224, 224): 4207872,
    (50, 8, 0, 224, 224): 3689216,
    (18, 1, 0, 64, 64): 954880,
    (18, 1, 1, 224, 224): 0,                          # bf16: no launch goes to the few-row kernel
}


@pytest.fixture(scope="module")
def L():
    from r3m_amd import _lib
    return _lib.lib()


def test_the_tables_cover_the_case_lists(L):
    for case, _ in sc.GPU_CASES:
        assert set(CONV[case]) == {0, *sc.forced_splits(L, case)[0]}, case
    for case, _ in lc.GPU_CASES:
        assert set(LINEAR[case]) == {0, *sc.forced_splits(L, lc.geom(case))[0]}, case


@pytest.mark.parametrize("case", list(CONV))
def test_conv2d_small_workspace_bytes(L, case):
    assert {s: L.r3m_conv2d_small_workspace_bytes(*case, s) for s in CONV[case]} == CONV[case]


@pytest.mark.parametrize("case", list(LINEAR))
def test_linear_small_workspace_bytes(L, case):
    assert {s: L.r3m_linear_small_workspace_bytes(*case, s) for s in LINEAR[case]} == LINEAR[case]


@pytest.mark.parametrize("size", list(LANGREW))
def test_langrew_infer_workspace_bytes(L, size):
    assert {R: L.r3m_langrew_infer_workspace_bytes(R, *size) for R in LANGREW[size]} == LANGREW[size]


@pytest.mark.parametrize("dims", list(TEXT))
def test_text_small_workspace_bytes(L, dims):
    d6 = (C.c_int * 6)(*dims)
    assert {bt: L.r3m_text_small_workspace_bytes(d6, *bt) for bt in TEXT[dims]} == TEXT[dims]
    # both sides of the take rule: every Linear of a layer taken at the fewest rows, none at the most, some in between
    taken = [sum(lc.linear_small_plan(L, case, fl)["take"] for case, fl in lc.text_linears(B * T, dims[2], dims[5])) for B, T in TEXT[dims]]
    assert taken[0] == 4 and taken[-1] == 0 and set(taken) - {0, 4}, taken
    B, T = list(TEXT[dims])[-1]
    assert TEXT[dims][(B, T)] == -(-L.r3m_text_workspace_bytes(d6, B, T) // 256) * 256, "nothing taken: the base workspace alone"


@pytest.mark.parametrize("key", list(RESNET))
def test_resnet_inference_workspace_bytes(L, key):
    h = L.r3m_resnet_create_hw(*key)
    assert h, L.r3m_last_error()
    try:
        assert L.r3m_resnet_inference_workspace_bytes(h) == RESNET[key]
    finally:
        L.r3m_resnet_destroy(h)
