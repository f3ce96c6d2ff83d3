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

    Epilogues no operator entry point can ask for (route_sig.OPERATOR_EPILOGUES: the downsample branch's accumulate, the masked join
    without partials, the eval-BatchNorm forwards of inference) cannot be matched flag for flag: for those, every kernel family of the
    launch must be run by an operator case of the same (dtype, direction, k, stride, width class, map orientation)."""
    from r3m_amd import _lib
    import test_gpu_ops_hw as T
    L = _lib.lib()
    have = {}
    have.update(route_sig.conv_case_signatures(L, T.HW_CONV_CASES, 0))
    have.update(route_sig.conv_case_signatures(L, T.HW_BF16_CASES + T.HW_ROW16_CASES, 1))
    have.update(route_sig.bnred_case_signatures(L, T.HW_BNRED_CASES))
    assert all(sig[4] for sig in have), [c for sig, c in have.items() if not sig[4]]      # no listed case is refused by the dispatch
    families = {(sig[0], sig[1], r) + sig[5:] for sig in have for r in sig[4]}
    missing, missing_family = {}, {}
    for plan, (case, dgrad, flags, bits) in _engine_launches(L):
        sig = route_sig.signature(L, case, dgrad, flags, bits, plan[1])
        assert sig[4], (plan, case, dgrad, flags, bits, L.r3m_last_error())
        if (dgrad, flags, bits) in route_sig.OPERATOR_EPILOGUES:
            if sig not in have:
                missing.setdefault(sig, (plan, case))
        else:
            for r in sig[4]:
                if (sig[0], sig[1], r) + sig[5:] not in families:
                    missing_family.setdefault((sig[0], sig[1], r) + sig[5:], (plan, case, flags, bits))
    assert not missing and not missing_family, "no operator case in tests/test_gpu_ops_hw.py for:\n" + "\n".join(
        f"  signature {k}: e.g. resnet{v[0][0]} dtype {v[0][1]} F={v[0][2]} at {v[0][3]} x {v[0][4]}, conv (N, Hi, Wi, Ci, Co, k, s, p) = {v[1]}"
        for k, v in list(missing.items()) + list(missing_family.items()))


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
    # transposes (Wi = 3, 4, 5 with Hi = 8, 16, 24) must all stay off it; FAST K steps need Ho Wo > 32
    ok = lambda c: c[2] % 8 == 0 and c[2] >= 8 and c[1] >= 4
    assert {ok(c) for c in H16["wgrad_all_taps"] if c[2] > c[1]} == {True, False}
    assert {ok(c) for c in H16["wgrad_all_taps"] if c[1] > c[2]} == {False} and len(H16["wgrad_all_taps"]) == 18
    assert {c[1] * c[2] > 32 for c in H16["wgrad_fast_path"]} == {True, False} and all(c[3] % 128 == 0 and c[4] % 128 == 0 for c in H16["wgrad_fast_path"])
    # kernel-row and halo kernel, wide and tall, 64- and 128-wide outputs, all on the kernel-row route by default
    assert all(fwd(c, 1) == (BF16_ROW,) for c in T.HW_ROW16_CASES)
    assert {(c[2] > c[1], c[4] % 128 == 0) for c in T.HW_ROW16_CASES} == {(a, b) for a in (True, False) for b in (True, False)}
    assert all(fwd(c, 1) == (BF16_HALO,) for c in H16["row16_too_wide"]) and {c[4] for c in H16["row16_too_wide"]} == {64, 128}
