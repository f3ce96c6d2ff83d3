"""Shared by tests/test_small_conv_plan.py (no GPU) and tests/test_gpu_small_conv.py: the case list of the small-M split-K forward
(csrc/conv_small.hip), the forced splits each case runs with, and the pinned plans of every ResNet convolution at 1, 8 and 16 frames.
Everything here goes through r3m_debug_conv_small_plan / r3m_resnet_conv_info: host-only, nothing is launched."""
import ctypes as C

AFFINE, ACCUM, RELU = 128, 2, 16
A, AR, AAR = AFFINE, AFFINE | RELU, AFFINE | ACCUM | RELU

# (N, Hi, Wi, Ci, Co, k, stride, pad) -> the flag sets run on it
GPU_CASES = [
    ((1, 7, 7, 512, 512, 3, 1, 1), (AR, AAR)),        # 49 ragged rows, 9 taps (layer4 of ResNet-18/34 at one frame)
    ((3, 1, 1, 512, 512, 3, 1, 1), (AR, AAR)),        # 3 rows (16-row tile), eight of nine taps all padding
    ((1, 7, 7, 512, 2048, 1, 1, 0), (A, AR, AAR)),    # all three flag sets; ACCUM reads the residual in the reducer
    ((1, 7, 7, 2048, 512, 1, 1, 0), (AR,)),           # long K, one tap
    ((2, 14, 14, 256, 256, 3, 1, 1), (AR, AAR)),      # 3x3 stride 1 on a 14 x 14 map, 392 rows: 7 row tiles, the last ragged
    ((1, 13, 10, 256, 256, 3, 2, 1), (AR,)),          # odd x even, stride 2
    ((1, 10, 13, 128, 128, 3, 2, 1), (AR,)),          # even x odd, stride 2 (35 rows: the 64-row tile; 32-row tile: the next case)
    ((2, 13, 11, 1024, 2048, 1, 2, 0), (A,)),         # downsample, flag A only
    ((1, 20, 12, 64, 128, 1, 2, 0), (A,)),            # 1x1 stride-2 downsample, even extents, two chunks of K
    ((1, 56, 56, 64, 64, 3, 1, 1), (AR, AAR)),        # 64-wide, 3136 rows: 49 row tiles
    ((1, 5, 5, 128, 64, 3, 1, 1), (AR,)),             # 25 rows: the 32-row tile
]


def conv_small_plan(L, case, flags=AR):
    """r3m_debug_conv_small_plan as a dict (take, bm, bn, S, grid, cps, tiles_m, tiles_n, nch, max_split)"""
    buf = (C.c_int * 10)()
    assert L.r3m_debug_conv_small_plan(*case, flags, buf, 10) == 10, L.r3m_last_error()
    return dict(zip(("take", "bm", "bn", "S", "grid", "cps", "tiles_m", "tiles_n", "nch", "max_split"), list(buf)))


def forced_splits(L, case):
    """the forced `split` values a case runs with: 1 (no ticket path), 2, the largest the entry accepts, one S that does not divide the
    chunk count (ragged last slice) and one S whose slice boundary falls inside a tap (chunks per slice no multiple of the chunks per
    tap; a 1 x 1 has one tap, so every boundary is inside it). Values the chunk count leaves no room for drop out."""
    p = conv_small_plan(L, case)
    nch, top = p["nch"], p["max_split"]
    cpt = case[3] // 32
    cps = lambda S: -(-nch // S)
    ragged = next((S for S in range(3, top + 1) if nch % S), None)
    inside = next((S for S in range(2, top + 1) if cps(S) % cpt and S != ragged), None)
    out = []
    for S in (1, 2, top, ragged, inside):
        if S is not None and 1 <= S <= top and S not in out:
            out.append(S)
    return out, ragged, inside


def resnet_convs(L, size, F, hw=(224, 224)):
    """[(N, Hi, Wi, Ci, Co, k, stride, pad)] of every convolution of the plan in r3m_resnet_conv_info order (index 0: the stem)"""
    h = L.r3m_resnet_create_hw(size, F, 0, hw[0], hw[1])
    assert h, L.r3m_last_error()
    try:
        out = []
        for i in range(L.r3m_resnet_num_convs(h)):
            v = [C.c_int() for _ in range(9)]
            assert L.r3m_resnet_conv_info(h, i, *[C.byref(x) for x in v]) == 0, L.r3m_last_error()
            Ci, Co, k, s, p, Hi, Wi, _, _ = [x.value for x in v]
            out.append((F, Hi, Wi, Ci, Co, k, s, p))
        return out, L.r3m_resnet_inference_workspace_bytes(h)
    finally:
        L.r3m_resnet_destroy(h)


# (size, frames) -> {convolution index: (tile rows, S, grid)} of the launches the routing rule takes at 224 x 224; every other
# convolution of the plan stays on the kernel it runs today
PINNED = {(18, 1): {1: (64, 4, 196),
           2: (64, 4, 196),
           3: (64, 4, 196),
           4: (64, 4, 196),
           5: (64, 4, 104),
           6: (64, 9, 234),
           8: (64, 9, 234),
           9: (64, 9, 234),
           10: (64, 9, 144),
           11: (64, 15, 240),
           12: (64, 1, 16),
           13: (64, 15, 240),
           14: (64, 15, 240),
           15: (64, 18, 144),
           16: (64, 29, 232),
           17: (64, 2, 16),
           18: (64, 29, 232),
           19: (64, 29, 232)},
 (18, 8): {5: (64, 1, 196),
           6: (64, 1, 196),
           8: (64, 1, 196),
           9: (64, 1, 196),
           10: (64, 2, 200),
           11: (64, 2, 200),
           12: (64, 1, 100),
           13: (64, 2, 200),
           14: (64, 2, 200),
           15: (64, 4, 224),
           16: (64, 4, 224),
           17: (64, 2, 112),
           18: (64, 4, 224),
           19: (64, 4, 224)},
 (18, 16): {10: (64, 1, 196),
            11: (64, 1, 196),
            12: (64, 1, 196),
            13: (64, 1, 196),
            14: (64, 1, 196),
            15: (64, 2, 208),
            16: (64, 2, 208),
            17: (64, 2, 208),
            18: (64, 2, 208),
            19: (64, 2, 208)},
 (34, 1): {1: (64, 4, 196),
           2: (64, 4, 196),
           3: (64, 4, 196),
           4: (64, 4, 196),
           5: (64, 4, 196),
           6: (64, 4, 196),
           7: (64, 4, 104),
           8: (64, 9, 234),
           10: (64, 9, 234),
           11: (64, 9, 234),
           12: (64, 9, 234),
           13: (64, 9, 234),
           14: (64, 9, 234),
           15: (64, 9, 234),
           16: (64, 9, 144),
           17: (64, 15, 240),
           18: (64, 1, 16),
           19: (64, 15, 240),
           20: (64, 15, 240),
           21: (64, 15, 240),
           22: (64, 15, 240),
           23: (64, 15, 240),
           24: (64, 15, 240),
           25: (64, 15, 240),
           26: (64, 15, 240),
           27: (64, 15, 240),
           28: (64, 15, 240),
           29: (64, 18, 144),
           30: (64, 29, 232),
           31: (64, 2, 16),
           32: (64, 29, 232),
           33: (64, 29, 232),
           34: (64, 29, 232),
           35: (64, 29, 232)},
 (34, 8): {7: (64, 1, 196),
           8: (64, 1, 196),
           10: (64, 1, 196),
           11: (64, 1, 196),
           12: (64, 1, 196),
           13: (64, 1, 196),
           14: (64, 1, 196),
           15: (64, 1, 196),
           16: (64, 2, 200),
           17: (64, 2, 200),
           18: (64, 1, 100),
           19: (64, 2, 200),
           20: (64, 2, 200),
           21: (64, 2, 200),
           22: (64, 2, 200),
           23: (64, 2, 200),
           24: (64, 2, 200),
           25: (64, 2, 200),
           26: (64, 2, 200),
           27: (64, 2, 200),
           28: (64, 2, 200),
           29: (64, 4, 224),
           30: (64, 4, 224),
           31: (64, 2, 112),
           32: (64, 4, 224),
           33: (64, 4, 224),
           34: (64, 4, 224),
           35: (64, 4, 224)},
 (34, 16): {16: (64, 1, 196),
            17: (64, 1, 196),
            18: (64, 1, 196),
            19: (64, 1, 196),
            20: (64, 1, 196),
            21: (64, 1, 196),
            22: (64, 1, 196),
            23: (64, 1, 196),
            24: (64, 1, 196),
            25: (64, 1, 196),
            26: (64, 1, 196),
            27: (64, 1, 196),
            28: (64, 1, 196),
            29: (64, 2, 208),
            30: (64, 2, 208),
            31: (64, 2, 208),
            32: (64, 2, 208),
            33: (64, 2, 208),
            34: (64, 2, 208),
            35: (64, 2, 208)},
 (50, 1): {2: (64, 4, 196),
           5: (64, 2, 98),
           6: (64, 4, 196),
           8: (64, 2, 98),
           9: (64, 4, 196),
           11: (64, 2, 196),
           12: (64, 9, 234),
           13: (64, 1, 104),
           14: (64, 2, 208),
           15: (64, 4, 104),
           16: (64, 9, 234),
           17: (64, 1, 104),
           18: (64, 4, 104),
           19: (64, 9, 234),
           20: (64, 1, 104),
           21: (64, 4, 104),
           22: (64, 9, 234),
           23: (64, 1, 104),
           24: (64, 4, 208),
           25: (64, 15, 240),
           26: (64, 2, 128),
           27: (64, 4, 256),
           28: (64, 8, 128),
           29: (64, 15, 240),
           30: (64, 2, 128),
           31: (64, 8, 128),
           32: (64, 15, 240),
           33: (64, 2, 128),
           34: (64, 8, 128),
           35: (64, 15, 240),
           36: (64, 2, 128),
           37: (64, 8, 128),
           38: (64, 15, 240),
           39: (64, 2, 128),
           40: (64, 8, 128),
           41: (64, 15, 240),
           42: (64, 2, 128),
           43: (64, 8, 256),
           44: (64, 29, 232),
           45: (64, 4, 128),
           46: (64, 8, 256),
           47: (64, 16, 128),
           48: (64, 29, 232),
           49: (64, 4, 128),
           50: (64, 16, 128),
           51: (64, 29, 232),
           52: (64, 4, 128)},
 (50, 8): {12: (64, 1, 196),
           15: (64, 1, 196),
           16: (64, 1, 196),
           18: (64, 1, 196),
           19: (64, 1, 196),
           21: (64, 1, 196),
           22: (64, 1, 196),
           25: (64, 2, 200),
           28: (64, 2, 200),
           29: (64, 2, 200),
           31: (64, 2, 200),
           32: (64, 2, 200),
           34: (64, 2, 200),
           35: (64, 2, 200),
           37: (64, 2, 200),
           38: (64, 2, 200),
           40: (64, 2, 200),
           41: (64, 2, 200),
           43: (64, 1, 200),
           44: (64, 4, 224),
           45: (64, 1, 224),
           46: (64, 1, 224),
           47: (64, 4, 224),
           48: (64, 4, 224),
           49: (64, 1, 224),
           50: (64, 4, 224),
           51: (64, 4, 224),
           52: (64, 1, 224)},
 (50, 16): {25: (64, 1, 196),
            28: (64, 1, 196),
            29: (64, 1, 196),
            31: (64, 1, 196),
            32: (64, 1, 196),
            34: (64, 1, 196),
            35: (64, 1, 196),
            37: (64, 1, 196),
            38: (64, 1, 196),
            40: (64, 1, 196),
            41: (64, 1, 196),
            44: (64, 2, 208),
            47: (64, 2, 208),
            48: (64, 2, 208),
            50: (64, 2, 208),
            51: (64, 2, 208)}}
