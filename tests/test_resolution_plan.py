"""CPU: native-resolution plans (r3m_resnet_create_hw). Every convolution's geometry matches torchvision's shapes for the same input
size (taken from the pinned oracle, oracle/resnet_ref.py, with forward hooks on a meta tensor), a 224 x 224 plan is the plan
r3m_resnet_create_dt makes, out-of-range sizes are refused with a message, and the general stem stays inside a CU's LDS."""
import ctypes as C

import pytest
import torch

import route_sig
from route_sig import ACCUM, AFFINE, BNRED, MASKED_ADD, RELU, STATS

SWEEP = [(s, s) for s in (32, 33, 47, 84, 96, 127, 128, 160, 223, 225, 256, 320, 511, 512)] + [(96, 160), (97, 131), (160, 96),
                                                                                              (33, 512), (512, 47)]


@pytest.fixture(scope="module")
def L():
    from r3m_amd import _lib
    return _lib.lib()


def _torch_convs(size, H, W):
    """[(Ci, Co, k, stride, pad, Hi, Wi, Ho, Wo)] of the oracle's convolutions in module order (= the engine's table order)"""
    from oracle import resnet_ref
    with torch.device("meta"):
        m = getattr(resnet_ref, f"resnet{size}")()
    m.eval()                     # eval BatchNorm: one frame at 32 x 32 leaves layer4 a single value per channel
    out = []

    def hook(mod, inp, res):
        x = inp[0]
        out.append((mod.in_channels, mod.out_channels, mod.kernel_size[0], mod.stride[0], mod.padding[0], x.shape[2], x.shape[3],
                    res.shape[2], res.shape[3]))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.register_forward_hook(hook)
    with torch.no_grad():
        m(torch.empty(1, 3, H, W, device="meta"))
    return out


_plan_convs = route_sig.plan_convs          # [(Ci, Co, k, stride, pad, Hi, Wi, Ho, Wo)], conv1 first (shared with tests/test_dispatch.py)


@pytest.mark.parametrize("size", [18, 34, 50])
def test_conv_geometry_matches_torchvision(L, size):
    for H, W in SWEEP:
        for dt in (0, 1):
            h = L.r3m_resnet_create_hw(size, 3, dt, H, W)
            assert h, L.r3m_last_error()
            try:
                hh, ww = C.c_int(), C.c_int()
                assert L.r3m_resnet_input_hw(h, C.byref(hh), C.byref(ww)) == 0 and (hh.value, ww.value) == (H, W)
                assert _plan_convs(L, h) == _torch_convs(size, H, W), (size, H, W)
                assert L.r3m_resnet_arena_bytes(h) > 0
            finally:
                L.r3m_resnet_destroy(h)


@pytest.mark.parametrize("size", [18, 34, 50])
@pytest.mark.parametrize("dt", [0, 1])
def test_create_hw_224_is_create_dt(L, size, dt):
    a = L.r3m_resnet_create_dt(size, 16, dt)
    b = L.r3m_resnet_create_hw(size, 16, dt, 224, 224)
    try:
        for q in ("r3m_resnet_num_params", "r3m_resnet_num_buffers", "r3m_resnet_arena_bytes", "r3m_resnet_num_tensors",
                  "r3m_resnet_out_dim", "r3m_resnet_num_convs"):
            assert getattr(L, q)(a) == getattr(L, q)(b), q
        name = C.create_string_buffer(128)
        kind, ndim, off = C.c_int(), C.c_int(), C.c_longlong()
        shape = (C.c_int * 4)()
        for i in range(L.r3m_resnet_num_tensors(a)):
            rows = []
            for h in (a, b):
                assert L.r3m_resnet_tensor_info(h, i, name, 128, C.byref(kind), C.byref(off), C.byref(ndim), shape) == 0
                rows.append((name.value, kind.value, off.value, ndim.value, tuple(shape)))
            assert rows[0] == rows[1]
        assert _plan_convs(L, a) == _plan_convs(L, b)
    finally:
        L.r3m_resnet_destroy(a)
        L.r3m_resnet_destroy(b)


def test_the_224_arena_is_unchanged(L):
    """the arena bytes of the 224 plans the benchmark and the pre-training configs use (recorded before native resolution)"""
    before = {(50, 1280, 0): 130016689152, (50, 1280, 1): 65723442432, (34, 2560, 1): 57598364672, (18, 16, 0): 632033024}
    for (size, F, dt), nbytes in before.items():
        h = L.r3m_resnet_create_dt(size, F, dt)
        g = L.r3m_resnet_create_hw(size, F, dt, 224, 224)
        assert h and g and L.r3m_resnet_arena_bytes(h) == L.r3m_resnet_arena_bytes(g) == nbytes
        L.r3m_resnet_destroy(h)
        L.r3m_resnet_destroy(g)


@pytest.mark.parametrize("H,W", [(31, 64), (64, 31), (16, 16), (513, 256), (256, 513), (1024, 1024), (0, 224), (-5, 224)])
def test_out_of_range_sizes_are_refused(L, H, W):
    assert not L.r3m_resnet_create_hw(50, 2, 0, H, W)
    msg = L.r3m_last_error().decode()
    assert "32..512" in msg and f"{H} x {W}" in msg, msg


def test_32bit_index_overflow_is_refused(L):
    assert not L.r3m_resnet_create_hw(50, 600, 0, 512, 512)
    msg = L.r3m_last_error().decode()
    assert "32-bit" in msg and "2^31" in msg, msg
    h = L.r3m_resnet_create_hw(50, 64, 0, 512, 512)
    assert h, L.r3m_last_error()
    L.r3m_resnet_destroy(h)


def test_general_stem_lds_fits_a_cu(L):
    f, w, d = C.c_int(), C.c_int(), C.c_int()
    worst = [0, 0, 0]
    for H in range(32, 513, 3):
        for W in list(range(32, 513, 1)):
            for F in (1, 3):
                assert L.r3m_stem_gen_lds_bytes(F, H, W, C.byref(f), C.byref(w), C.byref(d)) == 0
                worst = [max(a, b) for a, b in zip(worst, (f.value, w.value, d.value))]
    assert max(worst) <= 160 * 1024, worst
    assert L.r3m_stem_gen_lds_bytes(1, 31, 64, C.byref(f), C.byref(w), C.byref(d)) != 0


def test_forward_crop_needs_a_224_plan(L):
    """r3m_resnet_forward_crop refuses a plan that is not 224 x 224 before anything is launched (dummy non-null pointers)"""
    h = L.r3m_resnet_create_hw(18, 2, 0, 128, 128)
    try:
        boxes = (C.c_int * 8)()
        rc = L.r3m_resnet_forward_crop(h, 64, 1, C.addressof(boxes), 1, 240, 320, 64, 64, 64, 64, 1, None)
        assert rc != 0 and "224" in L.r3m_last_error().decode()
    finally:
        L.r3m_resnet_destroy(h)


def test_hip_resnet_refuses_out_of_range_frames_on_the_cpu():
    from r3m_amd.encoder import HipResNet
    with pytest.raises(ValueError, match="32..512"):
        HipResNet.check_input_hw(31, 224)
    HipResNet.check_input_hw(97, 131)


# ---- every launch of the swept plans runs a kernel built for the epilogue the engine asks of it -----------------------------------
_GG_SWITCH = {0, STATS, ACCUM, MASKED_ADD, 8, RELU, 8 | RELU, 32, BNRED, BNRED | MASKED_ADD}       # csrc/conv.hip GG_EPI_SWITCH
_PW = {0, STATS, ACCUM, BNRED, MASKED_ADD, BNRED | MASKED_ADD, AFFINE, AFFINE | RELU, AFFINE | ACCUM | RELU}   # conv_pw.hip pw_flags_ok
_BF16 = {0, STATS, ACCUM, MASKED_ADD, BNRED, BNRED | MASKED_ADD, AFFINE | RELU, AFFINE | ACCUM | RELU}
# route -> epilogue flag combinations its kernels are built with (the launchers' switches)
BUILT = {
    1: _GG_SWITCH | {AFFINE | RELU, AFFINE | ACCUM | RELU},     # 3x3 window kernel (LAUNCH_WIN cases + GG_EPI_SWITCH)
    11: _PW, 12: _PW, 13: _PW,                                  # persistent kernel, three forms
    20: _GG_SWITCH, 21: _GG_SWITCH, 22: _GG_SWITCH,             # 16-wide-K, gather, generic kernels
    30: _BF16 | {AFFINE},                                       # bf16 gather kernel (gg16_launch)
    31: _BF16, 32: _BF16,                                       # bf16 halo (halo_launch), kernel-row (row16_launch)
}


@pytest.mark.parametrize("size", [18, 34, 50])
@pytest.mark.parametrize("dt", [0, 1])
def test_every_launch_has_a_kernel_built_for_its_epilogue(L, size, dt):
    """forward (training: statistics; eval with a backward: plain), input gradients with the flags csrc/engine.hip plan_backward asks
    (fp32 plans fuse the BatchNorm-backward partials: 64; bf16 plans do not), and fused inference (r3m_debug_conv_fuses_affine: where
    it answers 1 the fused launch's route must build the flags; where 0 the engine runs the unfused sequence, plain forwards)."""
    for H, W in SWEEP:
        for F in (1, 3):
            # the launches and their flags: route_sig.engine_launches (one derivation, shared with the coverage test of test_dispatch.py)
            for (case, dgrad, flags, bits) in route_sig.engine_launches(L, size, dt, F, H, W):
                rs = route_sig.routes(L, case, dgrad, flags, bits, dt)
                assert len(rs) >= 1, (case, dgrad, flags, L.r3m_last_error())
                for r in rs:
                    assert r in BUILT and flags in BUILT[r], f"resnet{size} dt={dt} conv {case} dgrad={dgrad} flags={flags}: route {r}"


def test_bf16_fused_inference_answers_from_the_route(L):
    """r3m_debug_conv_fuses_affine for bf16 follows the route table (gg16_route + the epilogues each route builds), not the shape
    alone: a 3x3 stride-1 layer fuses affine + ReLU on the halo / kernel-row route; the plain affine store goes to the gather route,
    which builds it; a combination no bf16 kernel builds (affine + statistics) is refused even though the shape qualifies"""
    buf = (C.c_int * 8)()
    assert L.r3m_debug_conv_route(3, 28, 28, 128, 128, 3, 1, 1, 0, AFFINE | RELU, 0, 1, buf, 8) == 1 and buf[0] in (31, 32)
    assert L.r3m_debug_conv_fuses_affine(3, 28, 28, 128, 128, 3, 1, 1, AFFINE | RELU, 1) == 1
    assert L.r3m_debug_conv_route(3, 28, 28, 128, 128, 3, 1, 1, 0, AFFINE, 0, 1, buf, 8) == 1 and buf[0] == 30
    assert L.r3m_debug_conv_fuses_affine(3, 28, 28, 128, 128, 3, 1, 1, AFFINE, 1) == 1
    assert L.r3m_debug_conv_fuses_affine(3, 28, 28, 256, 512, 1, 2, 0, AFFINE, 1) == 1
    assert L.r3m_debug_conv_fuses_affine(3, 28, 28, 128, 128, 3, 1, 1, AFFINE | STATS, 1) == 0
    assert L.r3m_debug_conv_fuses_affine(3, 28, 28, 128, 128, 1, 1, 0, AFFINE | STATS, 1) == 0


# ---- the plan layout is pinned ---------------------------------------------------------------------------------------------------
def _plan_fingerprint(L, size, dt, F, H, W):
    """(arena bytes, hash of everything else the host-only queries tell), or ("refused", first five words of the message)"""
    import hashlib
    h = L.r3m_resnet_create_hw(size, F, dt, H, W)
    if not h:
        return ("refused", " ".join(L.r3m_last_error().decode().split()[:5]))
    try:
        rest = [L.r3m_resnet_num_params(h), L.r3m_resnet_num_buffers(h), _plan_convs(L, h)]
        name = C.create_string_buffer(128)
        kind, ndim, off = C.c_int(), C.c_int(), C.c_longlong()
        shape = (C.c_int * 4)()
        for i in range(L.r3m_resnet_num_tensors(h)):
            assert L.r3m_resnet_tensor_info(h, i, name, 128, C.byref(kind), C.byref(off), C.byref(ndim), shape) == 0
            rest.append((name.value.decode(), kind.value, off.value, ndim.value, tuple(shape)))
        cnt = C.c_longlong()
        for stage in range(4):
            assert L.r3m_resnet_stage_range(h, stage, C.byref(off), C.byref(cnt)) == 0
            rest.append((stage, off.value, cnt.value))
        return (L.r3m_resnet_arena_bytes(h), hashlib.sha256(repr(rest).encode()).hexdigest()[:16])
    finally:
        L.r3m_resnet_destroy(h)


_LAYOUT_HW = [(224, 224), (32, 32), (97, 161), (512, 512)]
_LAYOUT_F = [1, 5, 80, 1280]
# (size, dtype, F, H, W) -> _plan_fingerprint, recorded from the library built at the parent commit of the engine refactor
PLAN_LAYOUT = {
    (18, 0, 1, 224, 224): (102091008, 'db79de152c25154a'),
    (18, 0, 1, 32, 32): (68591872, '629a58ddb2775a4b'),
    (18, 0, 1, 97, 161): (79204352, 'bfda50e348010cf7'),
    (18, 0, 1, 512, 512): (246626048, '78720a51cbbead6b'),
    (18, 0, 5, 224, 224): (238946048, 'db79de152c25154a'),
    (18, 0, 5, 32, 32): (71376640, '629a58ddb2775a4b'),
    (18, 0, 5, 97, 161): (124506880, 'bfda50e348010cf7'),
    (18, 0, 5, 512, 512): (987797248, '78720a51cbbead6b'),
    (18, 0, 80, 224, 224): (2934959872, 'db79de152c25154a'),
    (18, 0, 80, 32, 32): (123735808, '629a58ddb2775a4b'),
    (18, 0, 80, 97, 161): (1028413184, 'bfda50e348010cf7'),
    (18, 0, 80, 512, 512): (14545000192, '78720a51cbbead6b'),
    (18, 0, 1280, 224, 224): (44041606912, 'db79de152c25154a'),
    (18, 0, 1280, 32, 32): (987797248, '629a58ddb2775a4b'),
    (18, 0, 1280, 97, 161): (14741859072, 'bfda50e348010cf7'),
    (18, 0, 1280, 512, 512): ('refused', 'resnet: 1280 frames of 512'),
    (18, 1, 1, 224, 224): (108330496, 'db79de152c25154a'),
    (18, 1, 1, 32, 32): (68284928, '629a58ddb2775a4b'),
    (18, 1, 1, 97, 161): (73646848, 'bfda50e348010cf7'),
    (18, 1, 1, 512, 512): (158321664, '78720a51cbbead6b'),
    (18, 1, 5, 224, 224): (177650688, 'db79de152c25154a'),
    (18, 1, 5, 32, 32): (69689344, '629a58ddb2775a4b'),
    (18, 1, 5, 97, 161): (96559104, 'bfda50e348010cf7'),
    (18, 1, 5, 512, 512): (546122752, '78720a51cbbead6b'),
    (18, 1, 80, 224, 224): (1533576192, 'db79de152c25154a'),
    (18, 1, 80, 32, 32): (96166912, '629a58ddb2775a4b'),
    (18, 1, 80, 97, 161): (580645376, 'bfda50e348010cf7'),
    (18, 1, 80, 512, 512): (7379725312, '78720a51cbbead6b'),
    (18, 1, 1280, 224, 224): (22329633792, 'db79de152c25154a'),
    (18, 1, 1280, 32, 32): (546122752, '629a58ddb2775a4b'),
    (18, 1, 1280, 97, 161): (7479091712, 'bfda50e348010cf7'),
    (18, 1, 1280, 512, 512): ('refused', 'resnet: 1280 frames of 512'),
    (34, 0, 1, 224, 224): (152699904, '3d65c5ab50d5a2c3'),
    (34, 0, 1, 32, 32): (109293568, 'b801d792f71b0ebc'),
    (34, 0, 1, 97, 161): (123354368, 'c4f89324cb5e2b76'),
    (34, 0, 1, 512, 512): (339959040, '81adb14a5a2a4a50'),
    (34, 0, 5, 224, 224): (330009344, '3d65c5ab50d5a2c3'),
    (34, 0, 5, 32, 32): (112903936, 'b801d792f71b0ebc'),
    (34, 0, 5, 97, 161): (183274496, 'c4f89324cb5e2b76'),
    (34, 0, 5, 512, 512): (1292483840, '81adb14a5a2a4a50'),
    (34, 0, 80, 224, 224): (3784542464, '3d65c5ab50d5a2c3'),
    (34, 0, 80, 32, 32): (180742400, 'b801d792f71b0ebc'),
    (34, 0, 80, 97, 161): (1361252864, 'c4f89324cb5e2b76'),
    (34, 0, 80, 512, 512): (18812566784, '81adb14a5a2a4a50'),
    (34, 0, 1280, 224, 224): (57027509504, '3d65c5ab50d5a2c3'),
    (34, 0, 1280, 32, 32): (1292483840, 'b801d792f71b0ebc'),
    (34, 0, 1280, 97, 161): (19459873024, 'c4f89324cb5e2b76'),
    (34, 0, 1280, 512, 512): ('refused', 'resnet: 1280 frames of 512'),
    (34, 1, 1, 224, 224): (153936640, '3d65c5ab50d5a2c3'),
    (34, 1, 1, 32, 32): (108899072, 'b801d792f71b0ebc'),
    (34, 1, 1, 97, 161): (115999232, 'c4f89324cb5e2b76'),
    (34, 1, 1, 512, 512): (225455104, '81adb14a5a2a4a50'),
    (34, 1, 5, 224, 224): (243640832, '3d65c5ab50d5a2c3'),
    (34, 1, 5, 32, 32): (110719488, 'b801d792f71b0ebc'),
    (34, 1, 5, 97, 161): (146277120, 'c4f89324cb5e2b76'),
    (34, 1, 5, 512, 512): (719752192, '81adb14a5a2a4a50'),
    (34, 1, 80, 224, 224): (1981765632, '3d65c5ab50d5a2c3'),
    (34, 1, 80, 32, 32): (144996352, 'b801d792f71b0ebc'),
    (34, 1, 80, 97, 161): (768460544, 'c4f89324cb5e2b76'),
    (34, 1, 80, 512, 512): (9550154752, '81adb14a5a2a4a50'),
    (34, 1, 1280, 224, 224): (28893023232, '3d65c5ab50d5a2c3'),
    (34, 1, 1280, 32, 32): (719752192, 'b801d792f71b0ebc'),
    (34, 1, 1280, 97, 161): (9876490752, 'c4f89324cb5e2b76'),
    (34, 1, 1280, 512, 512): ('refused', 'resnet: 1280 frames of 512'),
    (50, 0, 1, 224, 224): (218911488, '40ac808507dd3b5a'),
    (50, 0, 1, 32, 32): (119702272, 'a3790ff1911ae5a9'),
    (50, 0, 1, 97, 161): (152825088, '7bedf10d7a98a333'),
    (50, 0, 1, 512, 512): (647027712, '774c9b1c63c7d9af'),
    (50, 0, 5, 224, 224): (624277248, '40ac808507dd3b5a'),
    (50, 0, 5, 32, 32): (127966976, 'a3790ff1911ae5a9'),
    (50, 0, 5, 97, 161): (293701120, '7bedf10d7a98a333'),
    (50, 0, 5, 512, 512): (2791062528, '774c9b1c63c7d9af'),
    (50, 0, 80, 224, 224): (8354982912, '40ac808507dd3b5a'),
    (50, 0, 80, 32, 32): (283020288, 'a3790ff1911ae5a9'),
    (50, 0, 80, 97, 161): (2990109184, '7bedf10d7a98a333'),
    (50, 0, 80, 512, 512): (42651958272, '774c9b1c63c7d9af'),
    (50, 0, 1280, 224, 224): (130016689152, '40ac808507dd3b5a'),
    (50, 0, 1280, 32, 32): (2791062528, 'a3790ff1911ae5a9'),
    (50, 0, 1280, 97, 161): (45383710720, '7bedf10d7a98a333'),
    (50, 0, 1280, 512, 512): ('refused', 'resnet: 1280 frames of 512'),
    (50, 1, 1, 224, 224): (191965184, '40ac808507dd3b5a'),
    (50, 1, 1, 32, 32): (118803456, 'a3790ff1911ae5a9'),
    (50, 1, 1, 97, 161): (135514624, '7bedf10d7a98a333'),
    (50, 1, 1, 512, 512): (385008896, '774c9b1c63c7d9af'),
    (50, 1, 5, 224, 224): (396735488, '40ac808507dd3b5a'),
    (50, 1, 5, 32, 32): (122972160, 'a3790ff1911ae5a9'),
    (50, 1, 5, 97, 161): (206601984, '7bedf10d7a98a333'),
    (50, 1, 5, 512, 512): (1480467712, '774c9b1c63c7d9af'),
    (50, 1, 80, 224, 224): (4292351232, '40ac808507dd3b5a'),
    (50, 1, 80, 32, 32): (201225472, 'a3790ff1911ae5a9'),
    (50, 1, 80, 97, 161): (1594710272, '7bedf10d7a98a333'),
    (50, 1, 80, 512, 512): (21582652672, '774c9b1c63c7d9af'),
    (50, 1, 1280, 224, 224): (65723442432, '40ac808507dd3b5a'),
    (50, 1, 1280, 32, 32): (1480467712, 'a3790ff1911ae5a9'),
    (50, 1, 1280, 97, 161): (22957523712, '7bedf10d7a98a333'),
    (50, 1, 1280, 512, 512): ('refused', 'resnet: 1280 frames of 512'),
}


def test_plan_layout_is_unchanged(L):
    """Arena bytes, parameter / buffer counts, the conv table, the tensor table and the stage ranges of ResNet-18/34/50 x fp32/bf16 x
    F in {1, 5, 80, 1280} x four frame sizes equal what the library gave before the engine was refactored (and a combination it
    refused is still refused with the same opening words). PLAN_LAYOUT holds recorded results of that earlier library, not of the
    code under test."""
    assert len(PLAN_LAYOUT) == 3 * 2 * len(_LAYOUT_F) * len(_LAYOUT_HW)
    for (size, dt, F, H, W), want in PLAN_LAYOUT.items():
        assert _plan_fingerprint(L, size, dt, F, H, W) == want, (size, dt, F, H, W)
