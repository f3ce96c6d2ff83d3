"""CPU: which kernel family the convolution dispatch picks for every forward / input-gradient launch of the ResNet encoders at the
bench sizes — through r3m_debug_conv_route (csrc/conv.hip gg_route: a pure function of the launch parameters, nothing is launched).
DESIGN.md §4.1 claims that the whole ResNet-50 fp32 step runs the persistent kernel (conv_pw.hip, three forms) or the 3x3 window
kernel; a shape that silently fell back to the per-tile gather kernels would only show up as lost throughput on the GPU.
The layer table is torchvision's (the graph /root/reference/r3m/models/models_r3m.py:41-55 instantiates); the epilogue flags are
the ones csrc/engine.hip requests for each input gradient."""
import ctypes as C

import pytest

import route_sig
from route_sig import ACCUM, BNRED, MASKED_ADD, STATS

WIN, PW_POINT, PW_GATHER, PW_STRIDED, BF16, BF16_HALO, BF16_ROW = 1, 11, 12, 13, 30, 31, 32


@pytest.fixture(scope="module")
def route():
    from r3m_amd import _lib
    L = _lib.lib()

    def f(N, H, Ci, Co, k, s, p, dgrad=0, flags=0, bits=0, dt=0):
        buf = (C.c_int * 8)()
        n = L.r3m_debug_conv_route(N, H, H, Ci, Co, k, s, p, dgrad, flags, bits, dt, buf, 8)
        assert n >= 1, L.r3m_last_error()
        return list(buf[:n])
    return f


@pytest.fixture(scope="module")
def route_hw():
    """the non-square twin of `route`: Hi and Wi separate, () when the dispatch refuses the launch"""
    from r3m_amd import _lib
    L = _lib.lib()

    def f(N, Hi, Wi, Ci, Co, k, s, p, dgrad=0, flags=0, bits=0, dt=0):
        return route_sig.routes(L, (N, Hi, Wi, Ci, Co, k, s, p), dgrad, flags, bits, dt)
    return f


def _layers(size):
    """(name, H_in, Ci, Co, k, stride, pad, dgrad_flags, mask_bits) for every convolution behind the stem, dgrad flags as the engine sets
    them: inner BatchNorms get their backward partials from the producing dgrad with the mask recomputed (64); the first conv of a
    block joins the residual gradient and feeds the previous block's last BatchNorm, masked by that block's output bits (4 | 64,
    bits) unless the block has a downsample branch (plain store, then the downsample dgrad accumulates: 2)."""
    bottleneck = size == 50
    blocks = {18: [2, 2, 2, 2], 34: [3, 4, 6, 3], 50: [3, 4, 6, 3]}[size]
    out, H, cin = [], 56, 64
    for li, nb in enumerate(blocks):
        c = 64 << li
        for b in range(nb):
            s = 2 if (b == 0 and li > 0) else 1
            cout = 4 * c if bottleneck else c
            ds = b == 0 and (s != 1 or cin != cout)
            first = (0, 0) if ds else (MASKED_ADD | BNRED, 1)
            name = f"layer{li + 1}.{b}"
            if bottleneck:
                out.append((name + ".conv1", H, cin, c, 1, 1, 0) + first)
                out.append((name + ".conv2", H, c, c, 3, s, 1, BNRED, 0))
                out.append((name + ".conv3", H // s, c, cout, 1, 1, 0, BNRED, 0))
            else:
                out.append((name + ".conv1", H, cin, c, 3, s, 1) + first)
                out.append((name + ".conv2", H // s, c, c, 3, 1, 1, BNRED, 0))
            if ds:
                out.append((name + ".downsample", H, cin, cout, 1, s, 0, ACCUM, 0))
            H //= s
            cin = cout
    return out


@pytest.mark.parametrize("size,frames", [(50, 1280), (34, 2560), (18, 2560)])
def test_fp32_convolutions_run_the_persistent_or_the_window_kernel(route, size, frames):
    fast = {WIN, PW_POINT, PW_GATHER, PW_STRIDED}
    seen = {}
    for (name, H, Ci, Co, k, s, p, dflags, bits) in _layers(size):
        fwd = route(frames, H, Ci, Co, k, s, p, 0, STATS)
        assert len(fwd) == 1 and fwd[0] in fast, f"resnet{size} {name} forward -> {fwd}"
        if name == "layer1.0.conv1" or name == "layer1.0.downsample":
            continue                                   # their input is the stem's output: no input gradient is computed
        dg = route(frames, H, Ci, Co, k, s, p, 1, dflags, bits)
        assert all(r in fast for r in dg), f"resnet{size} {name} dgrad (flags {dflags}, bits {bits}) -> {dg}"
        # a stride-2 dgrad is one launch per output parity class that has taps: four for 3x3, one for 1x1
        assert len(dg) == (1 if s == 1 else (4 if k == 3 else 1)), (name, dg)
        if s == 2:
            assert set(dg) == {PW_STRIDED}, (name, dg)
        for r in fwd + dg:
            seen[r] = seen.get(r, 0) + 1
    assert PW_GATHER in seen and (size != 50 or PW_POINT in seen) and WIN in seen
    print(f"resnet{size}: launches by kernel family {dict(sorted(seen.items()))}")


def test_bf16_launches_take_the_bf16_path(route):
    assert route(1280, 56, 64, 256, 1, 1, 0, 0, STATS, 0, 1) == [BF16]


@pytest.mark.parametrize("size,frames", [(50, 1280), (34, 2560), (18, 2560), (18, 8)])
def test_bf16_3x3_stride1_launches_run_the_kernel_row_kernel(route, size, frames):
    """Round 6 (csrc/conv_row16.hip): every 3x3 / stride-1 forward and input-gradient launch of the bf16 plans — whatever the frame
    count, so that plans of different sizes accumulate in the same order — runs the persistent kernel-row kernel; everything else of
    the bf16 path stays on the gather kernel (30). A shape that fell back to the per-tile halo kernel (31) would only show as lost
    throughput and as a plan-size-dependent rounding."""
    n = 0
    for (name, H, Ci, Co, k, s, p, dflags, bits) in _layers(size):
        fwd = route(frames, H, Ci, Co, k, s, p, 0, STATS, 0, 1)
        want = [BF16_ROW] if (k == 3 and s == 1) else [BF16]
        assert fwd == want, f"resnet{size} {name} forward -> {fwd}"
        if name == "layer1.0.conv1" or name == "layer1.0.downsample":
            continue
        dg = route(frames, H, Ci, Co, k, s, p, 1, dflags, bits, 1)
        if k == 3 and s == 1:
            assert dg == [BF16_ROW], f"resnet{size} {name} dgrad (flags {dflags}) -> {dg}"
            n += 1
        else:
            assert all(r == BF16 for r in dg), (name, dg)
    assert n >= (12 if size == 50 else 7)
    assert route(1280, 56, 128, 128, 3, 2, 1, 1, BNRED, 0, 1) == [BF16] * 4


def test_shapes_outside_the_fast_forms_fall_back(route):
    # channel counts that are not multiples of 64 (the fuzz tests' geometries), mask bits on gathered 128-wide rows
    assert route(2, 13, 32, 96, 3, 2, 1, 0, STATS)[0] not in (WIN, PW_POINT, PW_GATHER, PW_STRIDED)
    assert route(64, 56, 128, 128, 3, 1, 1, 1, MASKED_ADD | BNRED, 1)[0] not in (PW_POINT, PW_GATHER, PW_STRIDED)


# ---- non-square frame sizes: every route the engine can take is run by an operator test ------------------------------------------------
def _non_square_sweep():
    from test_resolution_plan import SWEEP
    return [hw for hw in SWEEP if hw[0] != hw[1]] + [(96, 512), (512, 96)]


def _engine_launches(L):
    for size in (18, 34, 50):
        for dt in (0, 1):
            for F in (1, 3):
                for (H, W) in _non_square_sweep():
                    for launch in route_sig.engine_launches(L, size, dt, F, H, W):
                        yield (size, dt, F, H, W), launch


def test_every_engine_route_at_non_square_sizes_has_an_operator_case():
    """ResNet-18/34/50 x fp32/bf16 x F in {1, 3} x the non-square frame sizes of the sweep (+ 96 x 512, 512 x 96): the signature
    (dtype, dgrad, flags, mask_bits, routes, k, stride, Co % 128 == 0, wide / tall / square) of every forward and input-gradient launch,
    with the flags the engine asks, is the signature of a case of tests/test_gpu_ops_hw.py's lists -- a route the engine can take at a
    supported frame size and no operator test runs fails HERE, without a GPU, and names the geometry to add.

    Every epilogue the engine asks has an operator entry point (route_sig.OPERATOR_EPILOGUES): the downsample branch's accumulate, the
    masked join without partials and the eval-BatchNorm stores of inference are matched flag for flag against the lists of
    tests/test_gpu_conv_epilogues.py, like everything else. Nothing is matched by kernel family only any more."""
    from r3m_amd import _lib
    import test_gpu_conv_epilogues as E
    import test_gpu_ops_hw as T
    L = _lib.lib()
    have = {}
    have.update(route_sig.conv_case_signatures(L, T.HW_CONV_CASES, 0))
    have.update(route_sig.conv_case_signatures(L, T.HW_BF16_CASES + T.HW_ROW16_CASES, 1))
    have.update(route_sig.bnred_case_signatures(L, T.HW_BNRED_CASES))
    have.update(route_sig.affine_case_signatures(L, E.AFFINE_FP32_CASES, 0))
    have.update(route_sig.affine_case_signatures(L, E.AFFINE_BF16_CASES + E.AFFINE_BF16_3X3_CASES, 1))
    have.update(route_sig.join_case_signatures(L, E.JOIN_CASES, 0))
    have.update(route_sig.join_case_signatures(L, E.JOIN_CASES, 1))
    assert all(sig[4] for sig in have), [c for sig, c in have.items() if not sig[4]]      # no listed case is refused by the dispatch
    missing, n = {}, 0
    for plan, (case, dgrad, flags, bits) in _engine_launches(L):
        sig = route_sig.signature(L, case, dgrad, flags, bits, plan[1])
        assert sig[4], (plan, case, dgrad, flags, bits, L.r3m_last_error())
        assert (dgrad, flags, bits) in route_sig.OPERATOR_EPILOGUES, (plan, case, dgrad, flags, bits)
        n += 1
        if sig not in have:
            missing.setdefault(sig, (plan, case))
    assert n > 10000
    assert not missing, "no operator case in tests/test_gpu_ops_hw.py / tests/test_gpu_conv_epilogues.py for:\n" + "\n".join(
        f"  signature {k}: e.g. resnet{v[0][0]} dtype {v[0][1]} F={v[0][2]} at {v[0][3]} x {v[0][4]}, conv (N, Hi, Wi, Ci, Co, k, s, p) = {v[1]}"
        for k, v in missing.items())


def test_no_non_square_layer_is_refused_either_way_round(route_hw):
    """every layer geometry of those plans and its transpose (Hi <-> Wi) has a route for the forward and for the input gradient, and a
    stride-2 3x3 input gradient is four parity launches whenever both extents are >= 2"""
    from r3m_amd import _lib
    L = _lib.lib()
    seen = set()
    for plan, (case, dgrad, flags, bits) in _engine_launches(L):
        key = (plan[1], case, dgrad, flags, bits)
        if key in seen:
            continue
        seen.add(key)
        N, Hi, Wi, Ci, Co, k, s, p = case
        for (a, b) in ((Hi, Wi), (Wi, Hi)):
            r = route_hw(N, a, b, Ci, Co, k, s, p, dgrad, flags, bits, plan[1])
            assert len(r) >= 1, (plan, (N, a, b, Ci, Co, k, s, p), dgrad, flags, bits, L.r3m_last_error())
            if dgrad and k == 3 and s == 2 and a >= 2 and b >= 2:
                assert len(r) == 4, (plan, (N, a, b, Ci, Co, k, s, p), r)
    assert len(seen) > 500


def test_non_square_routes_go_by_the_extent_the_kernel_conditions_name(route_hw):
    """The conditions that treat height and width differently, pinned on both sides with the OTHER extent on the other side of the same
    number, so that a condition reading the wrong extent changes an answer here (it would otherwise only move launches to a slower
    kernel that computes the same values). fp32."""
    # conv.hip conv3x3_win_eligible: Wi <= 28, nothing of Hi
    assert route_hw(2, 40, 28, 128, 128, 3, 1, 1, 0, STATS) == (WIN,) and route_hw(2, 6, 28, 128, 128, 3, 1, 1, 1, BNRED) == (WIN,)
    assert route_hw(2, 6, 29, 128, 128, 3, 1, 1, 0, STATS) == (PW_GATHER,) and route_hw(2, 28, 40, 128, 128, 3, 1, 1, 1) == (PW_GATHER,)
    assert route_hw(1, 32, 6, 256, 256, 3, 1, 1, 0, STATS) == (WIN,) and route_hw(1, 6, 32, 256, 256, 3, 1, 1, 0, STATS) == (PW_GATHER,)
    # ... the masked join + partials on a map wider than the window kernel: the gather kernel
    assert route_hw(3, 6, 32, 256, 256, 3, 1, 1, 1, MASKED_ADD | BNRED, 1) == (21,)
    # conv_pw.hip pw_gemm_form: Wg < 4 || Hg < 2 per parity class of a stride-2 input gradient, classes in (py, px) order; and the
    # strided-output bounds (Hg - 1) os + ooy < Ho, (Wg - 1) os + oox < Wo, each against its own extent
    assert route_hw(3, 3, 32, 256, 512, 3, 2, 1, 1) == (PW_STRIDED, PW_STRIDED, 21, 21)          # odd rows: Hg = 1
    assert route_hw(3, 9, 7, 128, 256, 3, 2, 1, 1) == (PW_STRIDED, 21, PW_STRIDED, 21)           # odd columns: Wg = 3
    assert route_hw(3, 16, 7, 256, 512, 3, 2, 1, 1, BNRED) == (PW_STRIDED, 21, PW_STRIDED, 21)
    assert route_hw(3, 7, 9, 128, 256, 3, 2, 1, 1) == (PW_STRIDED,) * 4
    assert route_hw(2, 13, 10, 128, 128, 3, 2, 1, 1) == (PW_STRIDED,) * 4 and route_hw(2, 10, 13, 128, 128, 3, 2, 1, 1) == (PW_STRIDED,) * 4
    assert route_hw(1, 20, 12, 256, 256, 3, 2, 1, 1, BNRED) == (PW_STRIDED,) * 4 and route_hw(1, 6, 32, 512, 512, 3, 2, 1, 1, BNRED) == (PW_STRIDED,) * 4
    # gather form: Wg 3 / 4 with Hg 9, Hg 1 / 2 with Wg 9
    assert route_hw(2, 9, 3, 64, 64, 3, 1, 1, 0, STATS) == (21,) and route_hw(2, 9, 4, 64, 64, 3, 1, 1, 0, STATS) == (PW_GATHER,)
    assert route_hw(2, 1, 9, 64, 64, 3, 1, 1, 0, STATS) == (21,) and route_hw(2, 2, 9, 64, 64, 3, 1, 1, 0, STATS) == (PW_GATHER,)


def test_operator_case_groups_hold_what_they_are_there_for():
    """The signature of the coverage test does not see sizes or weight-gradient paths, so it does not need the threshold groups of
    tests/test_gpu_ops_hw.py: this pins, per group, the routes / extents the group's comment promises, so that a group cannot be
    emptied or drift off its condition unnoticed."""
    from r3m_amd import _lib
    import test_gpu_ops_hw as T
    L = _lib.lib()
    G, B, H16 = T.HW_CONV_GROUPS, T.HW_BNRED_GROUPS, T.HW_BF16_GROUPS
    fwd = lambda c, dt=0: route_sig.routes(L, c, 0, STATS, 0, dt)
    dgr = lambda c, fl=0, dt=0: route_sig.routes(L, c, 1, fl, 0, dt)
    maps = lambda g: {(c[1], c[2]) for c in g}
    mixed = {(PW_STRIDED, PW_STRIDED, 21, 21), (PW_STRIDED, 21, PW_STRIDED, 21)}
    assert mixed <= {dgr(c) for c in G["mixed_dgrad"]} and {(3, 32), (32, 3), (9, 7), (7, 9), (16, 7)} <= maps(G["mixed_dgrad"])
    assert mixed <= {dgr(c, BNRED) for (c, modes) in B["mixed_dgrad"] if "recompute" in modes}
    assert len(H16["mixed_dgrad"]) >= 4 and all(dgr(c, 0, 1) == (BF16,) * 4 for c in H16["mixed_dgrad"])
    assert {(6, 32), (32, 6), (3, 16), (16, 3), (3, 32), (32, 3), (2, 16), (16, 2)} <= maps(G["extremes"])
    assert {fwd(c) for c in G["extremes"] if (c[1], c[2]) == (32, 6) and c[5] == 3 and c[6] == 1} == {(WIN,)}
    assert {fwd(c) for c in G["extremes"] if (c[1], c[2]) == (6, 32) and c[5] == 3 and c[6] == 1} == {(PW_GATHER,)}
    assert {(20,), (21,)} <= {fwd(c) for c in G["extremes"]} and max(c[4] for c in G["extremes"]) == 2048
    assert maps(H16["extremes"]) == maps(G["extremes"])
    for k in (1, 3):
        assert any(c[1] == 1 and c[5] == k for c in G["one_pixel"]) and any(c[2] == 1 and c[5] == k for c in G["one_pixel"])
    assert [fwd(c) for c in G["window_width"]] == [(WIN,), (PW_GATHER,), (WIN,), (PW_GATHER,)]
    assert [(c[1], c[2]) for c in G["window_width"]] == [(40, 28), (40, 29), (6, 28), (6, 29)]
    assert [fwd(c) for c in G["persistent_extent"]] == [(21,), (PW_GATHER,), (PW_GATHER,), (21,), (PW_GATHER,), (21,), (PW_GATHER,)]
    assert {(9, 2), (33, 5), (5, 33)} <= maps(G["wgrad_window_width"]) and all(c[5:] == (3, 1, 1) for c in G["wgrad_window_width"])
    for k in (1, 3):           # (odd, even), (even, odd), (odd, odd) at stride 2
        par = {(c[1] % 2, c[2] % 2) for c in G["stride2_parity"] if c[5] == k and c[6] == 2}
        assert {(1, 0), (0, 1)} <= par and (k == 1 or (1, 1) in par), (k, par)
    assert any(c[5] == 1 and c[1] % 2 and c[2] % 2 for c in G["stride2_parity"])
    assert set(G["stride2_parity"]) <= set(H16["stride2_parity"])
    # more 128-row tiles than the persistent kernel has workers (two four-wave blocks on each of 256 CUs) and a partial last tile
    assert {shape for shape in maps(G["many_tiles"])} == {(28, 56), (56, 28)}
    for (N, Hi, Wi, Ci, Co, k, s, p) in G["many_tiles"]:
        M = N * ((Hi + 2 * p - k) // s + 1) * ((Wi + 2 * p - k) // s + 1)
        assert -(-M // 128) * (Co // 128) > 512 and M % 128, (N, Hi, Wi, M)
        assert fwd((N, Hi, Wi, Ci, Co, k, s, p))[0] in (PW_POINT, PW_GATHER)
    # bf16: all-taps weight gradient needs (Wi & 7) == 0, Wi >= 8, Hi >= 4: both answers on the wide maps (Hi = 3 against 4, 5), and the
    # transposes (Wi = 3, 4, 5 with Hi = 8, 16, 24) must all stay off it; FAST K steps need Ho Wo > 32 -- the library's own answers
    wg = lambda c, dt=1: route_sig.wgrad_plan(L, c, dt)
    ok = lambda c: wg(c).route == route_sig.WG16_ALL_TAPS
    assert {ok(c) for c in H16["wgrad_all_taps"] if c[2] > c[1]} == {True, False}
    assert {ok(c) for c in H16["wgrad_all_taps"] if c[1] > c[2]} == {False} and len(H16["wgrad_all_taps"]) == 18
    assert all(wg(c).route == route_sig.WG16_ROWS for c in H16["wgrad_fast_path"])
    assert {wg(c).fast for c in H16["wgrad_fast_path"]} == {1, 0} and all(c[3] % 128 == 0 and c[4] % 128 == 0 for c in H16["wgrad_fast_path"])
    # fp32 shared-window weight gradient: Wo = 2 is on it, the 9 x 1 maps of one_pixel are not
    assert all(wg(c, 0).route == route_sig.WG_WINDOW for c in G["wgrad_window_width"])
    assert {wg(c, 0).route for c in G["one_pixel"] if c[2] == 1 and c[5:] == (3, 1, 1)} == {route_sig.WG_ROWS}
    # kernel-row and halo kernel, wide and tall, 64- and 128-wide outputs, all on the kernel-row route by default
    assert all(fwd(c, 1) == (BF16_ROW,) for c in T.HW_ROW16_CASES)
    assert {(c[2] > c[1], c[4] % 128 == 0) for c in T.HW_ROW16_CASES} == {(a, b) for a in (True, False) for b in (True, False)}
    assert all(fwd(c, 1) == (BF16_HALO,) for c in H16["row16_too_wide"]) and {c[4] for c in H16["row16_too_wide"]} == {64, 128}


# ---- the engine-only epilogues and the tile queues (tests/test_gpu_conv_epilogues.py) -------------------------------------------------------
def test_conv_epilogue_case_groups_hold_what_they_are_there_for():
    """per group of tests/test_gpu_conv_epilogues.py the routes, tiles, flag sets and extents its comment promises, and that the engine
    would really make every listed launch (r3m_debug_conv_fuses_affine) and none of the refused ones"""
    from r3m_amd import _lib
    import test_gpu_conv_epilogues as E
    L = _lib.lib()
    A, AR, AAR = route_sig.AFFINE, route_sig.AFFINE | route_sig.RELU, route_sig.AFFINE | ACCUM | route_sig.RELU
    fwd = lambda c, fl, dt=0: route_sig.routes(L, c, 0, fl, 0, dt)
    dgr = lambda c, fl, dt=0: route_sig.routes(L, c, 1, fl, 0, dt)
    fuses = lambda c, fl, dt: L.r3m_debug_conv_fuses_affine(*c, fl, dt)
    rows = lambda c: c[0] * ((c[1] + 2 * c[7] - c[5]) // c[6] + 1) * ((c[2] + 2 * c[7] - c[5]) // c[6] + 1)
    orient = lambda g: {route_sig.shape_class(c[1], c[2]) for (c, _) in g}
    G = E.AFFINE_FP32_GROUPS
    assert all(fuses(c, fl, 0) == 1 for (c, fl) in E.AFFINE_FP32_CASES)
    assert all(fuses(c, fl, 1) == 1 for (c, fl) in E.AFFINE_BF16_CASES + E.AFFINE_BF16_3X3_CASES)
    assert all(fuses(c, fl, dt) == 0 for (c, fl, dt) in E.AFFINE_REFUSED) and {dt for (_, _, dt) in E.AFFINE_REFUSED} == {0, 1}
    assert any(fwd(c, fl) == (WIN,) and fl == A for (c, fl, dt) in E.AFFINE_REFUSED if dt == 0)
    assert all(fwd(c, fl) == (WIN,) for (c, fls) in G["window"] for fl in fls) and all(set(fls) == {AR, AAR} for (_, fls) in G["window"])
    assert {"wide", "tall"} <= orient(G["window"]) and any(rows(c) % 128 for (c, _) in G["window"])
    for name, route in (("pointwise_128", PW_POINT), ("gather_128", PW_GATHER)):
        assert all(fwd(c, fl) == (route,) and c[4] % 128 == 0 for (c, fls) in G[name] for fl in fls), name
        assert all(set(fls) == {A, AR, AAR} for (_, fls) in G[name]) and {"wide", "tall"} <= orient(G[name])
        assert any(rows(c) % 128 and rows(c) > 128 for (c, _) in G[name]), name
    assert {c[6] for (c, _) in G["gather_128"]} == {1, 2}
    # 64-wide outputs: the burst launches take the 512 x 64 tile (half the row panels of the 256 x 64 one), the others the 256 x 64 tile
    t64 = {(fwd(c, fl)[0], fl, route_sig.pw_queue_grids(L, c, 0, fl)[0][0] == -(-rows(c) // 512)) for (c, fls) in G["tile_64"] for fl in fls}
    assert all(c[4] == 64 and rows(c) % 512 and rows(c) > 512 for (c, _) in G["tile_64"])
    assert {(PW_GATHER, AR, True), (PW_GATHER, AAR, False), (PW_GATHER, A, False), (PW_POINT, AR, True), (PW_POINT, AAR, False),
            (PW_POINT, AR, False), (PW_POINT, A, False)} <= t64, t64
    assert all(fwd(c, A) == (PW_GATHER,) and c[5:] == (1, 2, 0) and fls == (A,) for (c, fls) in G["downsample"])
    assert {(c[1] % 2, c[2] % 2) for (c, _) in G["downsample"]} == {(1, 0), (0, 1), (1, 1), (0, 0)}
    assert {fwd(c, AR)[0] for (c, _) in G["one_pixel"]} == {WIN, PW_POINT} and all(c[1:3] == (1, 1) for (c, _) in G["one_pixel"])
    # bf16: route 30 with all three flag sets, Co = 64 and 128 and more, ragged M, wide and tall; 32 by default and 31 when switched for the
    # 3x3 list; 31 in the default mode on the maps too wide for the kernel-row kernel
    H = E.AFFINE_BF16_GROUPS
    assert all(fwd(c, fl, 1) == (BF16,) for (c, fls) in H["gather"] for fl in fls)
    assert {fl for (_, fls) in H["gather"] for fl in fls} == {A, AR, AAR} and {64, 128} <= {c[4] for (c, _) in H["gather"]}
    assert {"wide", "tall"} <= orient(H["gather"]) and any(rows(c) % 256 for (c, _) in H["gather"])
    assert all(fwd(c, fl, 1) == (BF16_HALO,) for (c, fls) in H["row16_too_wide"] for fl in fls)
    assert all(fwd(c, fl, 1) == (BF16_ROW,) and set(fls) == {AR, AAR} for (c, fls) in H["conv3x3"] for fl in fls)
    old = L.r3m_debug_set_conv3x3_bf16(0)
    try:
        assert all(fwd(c, fl, 1) == (BF16_HALO,) for (c, fls) in H["conv3x3"] for fl in fls)
    finally:
        L.r3m_debug_set_conv3x3_bf16(old)
    assert {(route_sig.shape_class(c[1], c[2]), c[4]) for (c, _) in H["conv3x3"]} >= {(o, co) for o in ("wide", "tall") for co in (64, 128)}
    assert any(rows(c) % 128 for (c, _) in H["conv3x3"] if c[4] == 128) and any(rows(c) % 256 for (c, _) in H["conv3x3"] if c[4] == 64)
    # input gradients
    J = E.JOIN_GROUPS
    s2 = [c for (c, m) in J["accumulate_stride2"]]
    assert all(m == "accumulate" and c[5:] == (1, 2, 0) for (c, m) in J["accumulate_stride2"])
    assert {(c[1] % 2, c[2] % 2) for c in s2} == {(1, 0), (0, 1), (1, 1), (0, 0)}
    assert {dgr(c, ACCUM) for c in s2} == {(PW_STRIDED,), (21,)} and all(dgr(c, ACCUM, 1) == (BF16,) for c in s2)     # ONE launch: three classes skipped
    assert all(c[3:] == (64, 256, 1, 1, 0) and dgr(c, ACCUM) == (PW_POINT,) for (c, m) in J["accumulate_stride1"])
    jn = [c for (c, m) in J["join"]]
    assert all(m == "join" and c[6] == 1 for (c, m) in J["join"])
    assert {dgr(c, MASKED_ADD)[0] for c in jn} == {WIN, PW_POINT, PW_GATHER} and {dgr(c, MASKED_ADD, 1)[0] for c in jn} == {BF16, BF16_HALO, BF16_ROW}
    assert any(c[3:] == (64, 64, 3, 1, 1) and dgr(c, MASKED_ADD) == (PW_GATHER,) for c in jn)                         # the first-block form
    assert {c[3] for c in jn if c[5] == 3} >= {64, 128, 256}


def test_tile_queue_cases_pass_the_launchers_threshold():
    """conv_pw.hip launch_pw_shape hands the queues on when gridM >= 64 (and at least 64 blocks, which that implies): every queue case
    marked `used` has every launch at or above it on the persistent kernel, the others have every launch below; gridM covers 64, 74
    (= 9 x 8 + 2: a ragged last group of panels) against 63, gridN 1 and more, both tile widths, and a four-launch stride-2 input gradient"""
    from r3m_amd import _lib
    import test_gpu_conv_epilogues as E
    L = _lib.lib()
    seen, kinds = set(), set()
    for (kind, case, flags, used) in E.QUEUE_CASES:
        dgrad, fl = {"fwd_stats": (0, STATS), "affine": (0, flags), "dgrad": (1, 0), "accumulate": (1, ACCUM)}[kind]
        grids = route_sig.pw_queue_grids(L, case, dgrad, fl)
        assert grids, (kind, case, "not on the persistent kernel")
        assert all((gm >= 64) == used for (gm, gn) in grids), (kind, case, grids)
        seen |= {(gm, min(gn, 2), case[3 if dgrad else 4] % 128 == 0) for (gm, gn) in grids}
        kinds.add((kind, used, len(grids)))
    assert {(64, 1, True), (74, 1, True), (74, 2, True), (63, 1, True), (74, 1, False)} <= seen, seen
    assert {("fwd_stats", True, 1), ("fwd_stats", False, 1), ("affine", True, 1), ("affine", False, 1), ("dgrad", True, 1), ("dgrad", True, 4),
            ("accumulate", True, 1)} <= kinds, kinds
    # the burst launches of 64-wide outputs run the 512 x 64 tile: 6 x 56 x 56 rows are 37 panels there, NOT a queue case
    assert route_sig.pw_queue_grids(L, (6, 56, 56, 64, 64, 3, 1, 1), 0, STATS) == ((37, 1),)


# ---- the language-reward head's Linear layers (csrc/lang.hip through the conv GEMMs; tests/test_gpu_langrew_edges.py) -----------------------
def test_head_launches_of_the_workload_have_an_operator_case():
    """The head's Linear layers are conv launches with epilogues nothing else asks (forward 8 | 16 = bias + ReLU, input gradient 32 = ReLU
    mask on the store). The workload runs them at R = 15 x 256 and 15 x 512 rows, K1 = 2 x 512 + 768 and 2 x 2048 + 768, H = 1024, in
    both dtypes: every signature (dtype, dgrad, flags, routes, Co % 128 == 0) of those launches is the signature of a launch of a case
    of tests/test_gpu_langrew_edges.py (batched and single-call lists), and the dispatch refuses none of either."""
    from r3m_amd import _lib
    import test_gpu_langrew_edges as T
    L = _lib.lib()
    have = {}
    for (B, D, H, LD) in T.FP32_CASES:
        for (case, dgrad, flags) in route_sig.head_launches(15 * B, 2 * D + LD, H, 0):
            have.setdefault(route_sig.head_signature(L, case, dgrad, flags, 0), (B, D, H, LD))
    for (B, D, H, LD) in T.BF16_CASES:
        assert LD % 64 == 0
        for (case, dgrad, flags) in route_sig.head_launches(15 * B, 2 * D + LD, H, 1):
            have.setdefault(route_sig.head_signature(L, case, dgrad, flags, 1), (B, D, H, LD))
    for R in T.CALL_ROWS:
        D, H, LD = T.CALL_DIMS
        for (case, dgrad, flags) in route_sig.head_launches(R, 2 * D + LD, H, 0):
            have.setdefault(route_sig.head_signature(L, case, dgrad, flags, 0), ("call", R))
    assert all(sig[3] for sig in have), [c for sig, c in have.items() if not sig[3]]
    missing, seen = {}, set()
    for R in (15 * 256, 15 * 512):
        for K1 in (2 * 512 + 768, 2 * 2048 + 768):
            for dt in (0, 1):
                for (case, dgrad, flags) in route_sig.head_launches(R, K1, 1024, dt):
                    sig = route_sig.head_signature(L, case, dgrad, flags, dt)
                    assert sig[3], (case, dgrad, flags, dt, L.r3m_last_error())
                    assert (dgrad, flags, 0) in route_sig.OPERATOR_EPILOGUES, (case, dgrad, flags)
                    seen.add(sig)
                    if sig not in have:
                        missing.setdefault(sig, case)
    assert not missing, "no case in tests/test_gpu_langrew_edges.py for:\n" + "\n".join(f"  signature {k}: e.g. {v}" for k, v in missing.items())
    # what the workload's head runs today: gather GEMM with and without the LDS-direct loads forward, the persistent pointwise kernel and
    # the gather GEMM for the input gradients; the bf16 gather kernel throughout
    assert {s[3] for s in seen if s[0] == 0 and s[1] == 0} == {(21,), (22,)} and {s[3] for s in seen if s[0] == 0 and s[1] == 1} == {(PW_POINT,), (21,)}
    assert {s[3] for s in seen if s[0] == 1} == {(BF16,)}


# ---- the weight gradients behind the stem (csrc/wgrad.hip wgrad_plan through r3m_debug_wgrad_route) -----------------------------------------
def _wgrad_want(dt, Hin, Ci, Co, k, s):
    """(route, tile) the weight gradient of a ResNet layer at a 224 x 224 frame must run -- as profiles/wgrad_unify_routes.txt lists them.
    A layer that fell off the window kernel or the all-taps kernel would only show as lost throughput on the GPU."""
    R = route_sig
    wide = Ci % 128 == 0 and Co % 128 == 0
    if dt == 0:
        tile = 128 if wide else 64
        if k == 1:
            return (R.WG_TAPS_SIMPLE if s == 1 else R.WG_TAPS_GATHER), tile
        return (R.WG_WINDOW if s == 1 else R.WG_ROWS), tile
    if k == 3 and s == 1 and Hin % 8 == 0:          # 56 x 56 and 28 x 28 (and 14 x 14 has no multiple of 8: kernel rows / taps)
        return R.WG16_ALL_TAPS, 64
    if k == 3 and wide:
        return R.WG16_ROWS, 128
    return R.WG16_TAPS, (128 if wide else 64)


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size,frames", [(50, 1280), (34, 2560), (18, 2560), (18, 8)])
def test_weight_gradient_route_of_every_layer(size, frames, dt):
    """per network and precision the route and tile of every layer's weight gradient: fp32 3x3 / stride-1 layers on the shared-window
    kernel, 3x3 / stride 2 on kernel rows, 1x1 / stride 1 on simple rows, strided 1x1 on gathered rows; bf16 3x3 / stride-1 layers at widths
    that are multiples of 8 on the all-taps kernel, the other 3x3 layers of 128-multiple channel counts on kernel rows (the division-free
    walk everywhere), the rest per tap with K steps of 32 rows on the 128-wide tile and 64 on the 64-wide one. And the grid and the
    workspace follow from the plan: gx = tiles x tap groups, workspace = split x Co x k^2 x Ci floats, the splits cover M."""
    from r3m_amd import _lib
    L = _lib.lib()
    R = route_sig
    seen = set()
    for (name, H, Ci, Co, k, s, p, _, _) in _layers(size):
        case = (frames, H, H, Ci, Co, k, s, p)
        r = R.wgrad_plan(L, case, dt)
        assert (r.route, r.tile) == _wgrad_want(dt, H, Ci, Co, k, s), (size, name, r)
        assert r.bk == {R.WG_ROWS: 16, R.WG16_ALL_TAPS: 64, R.WG16_TAPS: 32 if r.tile == 128 else 64}.get(r.route, 32), (name, r)
        assert r.fast == (r.route == R.WG16_ROWS), (name, r)
        groups = {R.WG_TAPS_SIMPLE: k * k, R.WG_TAPS_GATHER: k * k, R.WG16_TAPS: k * k, R.WG16_ALL_TAPS: 1}.get(r.route, k)
        assert r.tilesN == -(-Ci // r.tile) and r.gx == -(-Co // r.tile) * r.tilesN * groups, (name, r)
        assert (r.lds_bytes > 0) == (r.route in (R.WG_WINDOW, R.WG16_ALL_TAPS)) and r.lds_bytes <= 160 * 1024, (name, r)
        Ho = (H + 2 * p - k) // s + 1
        M = frames * Ho * Ho
        assert r.split >= 1 and r.rows_per_split % (64 if dt else 32) == 0 and r.split * r.rows_per_split >= M, (name, r)
        assert dt == 1 or (r.split - 1) * r.rows_per_split < M, (name, r)                      # fp32: no empty split
        assert L.r3m_conv2d_wgrad_workspace_bytes_dt(*case, dt) == 4 * r.split * Co * k * k * Ci, (name, r)
        seen.add(r.route)
    want = {0: {R.WG_WINDOW, R.WG_ROWS} | ({R.WG_TAPS_SIMPLE, R.WG_TAPS_GATHER} if size == 50 else {R.WG_TAPS_GATHER}),
            1: {R.WG16_ALL_TAPS, R.WG16_TAPS, R.WG16_ROWS}}[dt]
    assert seen == want, (size, dt, seen)


def test_every_weight_gradient_route_and_variant_has_an_operator_case():
    """every route value, and inside a route every kernel instantiation (tile 128 / 64, K step, FAST) that a layer of the networks, the
    reward head or ANY listed case takes, is run by a case of the GPU operator lists, which compare dW with autograd / float64; each
    precision has a case of more than one split whose last split is shorter than the others, and workspace = split x |dW| throughout"""
    from r3m_amd import _lib
    L = _lib.lib()
    R = route_sig
    ops = R.wgrad_operator_cases()
    have = {}
    for (origin, case, dt) in ops:
        r = R.wgrad_plan(L, case, dt)
        have.setdefault(R.wgrad_variant(r), (origin, case))
        N, Hi, Wi, Ci, Co, k, s, p = case
        assert L.r3m_conv2d_wgrad_workspace_bytes_dt(*case, dt) == 4 * r.split * Co * k * k * Ci, (case, dt, r)
    for dt in (0, 1):
        assert {v[0] for v in have if v[0] in R.WG_ROUTES[dt]} == set(R.WG_ROUTES[dt]), (dt, sorted(have))
    assert set(have) == {(40, 128, 32, 0), (40, 64, 32, 0), (41, 128, 32, 0), (41, 64, 32, 0), (42, 128, 16, 0), (42, 64, 16, 0),
                         (43, 128, 32, 0), (43, 64, 32, 0), (50, 128, 32, 0), (50, 64, 64, 0), (51, 128, 32, 0), (51, 128, 32, 1),
                         (52, 64, 64, 0)}, sorted(have)
    engine = set()
    for (size, frames) in ((50, 1280), (34, 2560), (18, 2560), (18, 8)):
        for (name, H, Ci, Co, k, s, p, _, _) in _layers(size):
            engine |= {R.wgrad_variant(R.wgrad_plan(L, (frames, H, H, Ci, Co, k, s, p), dt)) for dt in (0, 1)}
    for Rows in (15 * 256, 15 * 512):
        for K in (2 * 512 + 768, 2 * 2048 + 768, 1024):
            engine |= {R.wgrad_variant(R.wgrad_plan(L, (Rows, 1, 1, K, 1024, 1, 1, 0), dt)) for dt in (0, 1)}
    assert engine <= set(have), engine - set(have)
    rows = lambda c: c[0] * ((c[1] + 2 * c[7] - c[5]) // c[6] + 1) * ((c[2] + 2 * c[7] - c[5]) // c[6] + 1)
    for dt in (0, 1):
        ragged = [(c, r) for (_, c, d) in ops if d == dt for r in [R.wgrad_plan(L, c, dt)]
                  if r.split > 1 and 0 < rows(c) - (r.split - 1) * r.rows_per_split < r.rows_per_split]
        assert ragged, dt
        assert {r.route for (_, r) in ragged} >= ({R.WG_TAPS_SIMPLE, R.WG_ROWS, R.WG_WINDOW} if dt == 0 else {R.WG16_TAPS, R.WG16_ALL_TAPS}), dt


def test_debug_wgrad_route_refuses_a_short_buffer():
    from r3m_amd import _lib
    L = _lib.lib()
    buf = (C.c_int * 9)()
    assert L.r3m_debug_wgrad_route(2, 9, 7, 64, 64, 3, 1, 1, 0, buf, 8) == -1
    assert L.r3m_debug_wgrad_route(2, 9, 7, 64, 64, 3, 1, 1, 0, buf, 9) == 9 and buf[0] == route_sig.WG_WINDOW
