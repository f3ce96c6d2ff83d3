"""tests/profile_model.py against itself, against the survey's FLOP counts and against the case list of tests/test_gpu_profile.py. No GPU."""
import itertools
import os
import re

import pytest

import profile_cases as pc
import profile_model as pm
import route_sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURVEY_FWD = {18: 3.6271, 34: 7.3265, 50: 8.1743}           # SURVEY.md §8(d), GFLOP per 224 x 224 frame, forward
SURVEY_FWD_BWD = {18: 10.6453, 34: 21.7435, 50: 24.2868}    # forward + input gradients (none for conv1) + weight gradients

SHAPES = [(N, Hi, Wi, Ci, Co, k, s, p) for N in (1, 3) for (Hi, Wi) in ((1, 9), (7, 9), (10, 13), (33, 5)) for (Ci, Co) in ((64, 128),)
          for (k, p) in ((1, 0), (3, 1), (7, 3)) for s in (1, 2, 3)]


def brute_pairs(case):
    """every (input pixel, tap) pair with a compatible tap, pixel by pixel: what dgrad_pairs counts class by class"""
    N, Hi, Wi, Ci, Co, k, s, p = case
    return sum(1 for iy, ix, ky, kx in itertools.product(range(Hi), range(Wi), range(k), range(k))
               if (iy + p - ky) % s == 0 and (ix + p - kx) % s == 0)


@pytest.fixture(scope="module")
def L():
    from r3m_amd import _lib
    return _lib.lib()


def test_enumeration_is_the_closed_form_at_stride_1():
    for c in SHAPES:
        N, Hi, Wi, Ci, Co, k, s, p = c
        if s == 1:
            assert pm.dgrad_pairs(c) == Hi * Wi * k * k
            assert pm.dgrad_flops(c) == 2 * N * Hi * Wi * Ci * k * k * Co
            one = pm.dgrad_launches(c, 0)
            assert len(one) == 1 and one[0].flops == pm.dgrad_flops(c) and (one[0].M, one[0].N, one[0].K, one[0].taps) == (N * Hi * Wi, Ci, Co, k * k)


def test_enumeration_by_class_is_the_enumeration_by_pixel():
    for c in SHAPES:
        assert pm.dgrad_pairs(c) == brute_pairs(c), c
        launches = pm.dgrad_launches(c, 0)
        assert sum(l.flops for l in launches) == pm.dgrad_flops(c), c
        assert sum(l.M * l.taps for l in launches) == c[0] * pm.dgrad_pairs(c), c


def test_strided_1x1_touches_one_pixel_in_s_squared_with_one_tap():
    for c in SHAPES:
        N, Hi, Wi, Ci, Co, k, s, p = c
        if k == 1 and s > 1:
            assert pm.dgrad_pairs(c) == -(-Hi // s) * -(-Wi // s)
            with_taps = [l for l in pm.dgrad_launches(c, 0) if l.taps]
            assert len(with_taps) == 1 and with_taps[0].taps == 1 and with_taps[0].M == N * -(-Hi // s) * -(-Wi // s)
            # a class without taps writes zeros and reads nothing; it is skipped when the launch would only add
            assert all(l.bytes == 4 * l.M * Ci for l in pm.dgrad_launches(c, 0) if not l.taps)
            assert len(pm.dgrad_launches(c, 0, pm.ACCUM)) == 1
            # the forward reads the same quarter (ninth) of the input
            f = pm.forward_launches(c, 0)[0]
            assert f.bytes == 4 * (N * -(-Hi // s) * -(-Wi // s) * Ci + Co * Ci + f.M * Co)


def test_bytes_of_a_dense_launch_are_input_weights_and_result():
    c = (2, 9, 7, 64, 128, 3, 1, 1)
    f, = pm.forward_launches(c, 1, pm.STATS, stats_rows=5)
    assert f.bytes == 2 * (2 * 9 * 7 * 64 + 128 * 9 * 64 + 2 * 9 * 7 * 128) + 8 * 5 * 128
    w, = pm.wgrad_launches(c, 1, split=3)
    assert w.bytes == 2 * (2 * 9 * 7 * 128 + 2 * 9 * 7 * 64) + 4 * 3 * 128 * 9 * 64 and w.flops == f.flops
    assert pm.stem_launches(2, 34, 32, 0, "fwd")[0].flops == 2 * 2 * 17 * 16 * 64 * 147


def bench_constant():
    src = open(os.path.join(ROOT, "bench.py")).read()
    m = re.search(r"FWD_GFLOP_PER_FRAME = \{18: ([0-9.]+), 34: ([0-9.]+), 50: ([0-9.]+)\}", src)
    return {18: float(m.group(1)), 34: float(m.group(2)), 50: float(m.group(3))} if m else {}


def resnet_gflop(L, size):
    """(forward, forward + backward) GFLOP per 224 x 224 frame from the plan's own convolution table"""
    h = L.r3m_resnet_create_hw(size, 1, 0, 224, 224)
    assert h, L.r3m_last_error()
    try:
        convs = [(1, c[5], c[6], c[0], c[1], c[2], c[3], c[4]) for c in route_sig.plan_convs(L, h)]
    finally:
        L.r3m_resnet_destroy(h)
    fwd = sum(pm.forward_flops(c) for c in convs)
    bwd = sum(pm.dgrad_flops(c) for c in convs[1:]) + sum(pm.wgrad_flops(c) for c in convs)
    return fwd * 1e-9, (fwd + bwd) * 1e-9


@pytest.mark.parametrize("size", [18, 34, 50])
def test_resnet_flops_per_frame_are_the_surveys(L, size):
    """The model's sums over r3m_resnet_conv_info equal SURVEY.md's to its four decimals. bench.py's FWD_GFLOP_PER_FRAME is printed next to
    them and not asserted (it is not this test's to change): it is 3.6286 / 7.3407 for ResNet-18 / -34 where both others say 3.6271 /
    7.3265; ResNet-50 agrees."""
    fwd, both = resnet_gflop(L, size)
    print(f"ResNet-{size}: forward GFLOP per frame: model {fwd:.4f}, bench.py {bench_constant().get(size)}, survey {SURVEY_FWD[size]}; "
          f"forward + backward: model {both:.4f}, survey {SURVEY_FWD_BWD[size]}")
    assert round(fwd, 4) == SURVEY_FWD[size]
    assert round(both, 4) == SURVEY_FWD_BWD[size]


def test_gpu_cases_cover_every_class_operation_dtype_and_route(L):
    classes, families, wg = set(), {0: set(), 1: set()}, {0: set(), 1: set()}
    for c, dt in pc.conv_cases():
        r_f, r_d = route_sig.routes(L, c, 0, 0, 0, dt), route_sig.routes(L, c, 1, 0, 0, dt)
        families[dt] |= set(r_f) | set(r_d) | set(route_sig.routes(L, c, 0, route_sig.STATS, 0, dt))
        wg[dt].add(route_sig.wgrad_plan(L, c, dt).route)
        classes.add((dt, "fwd", pm.forward_launches(c, dt, 0, r_f)[0].kclass))
        d = pm.dgrad_launches(c, dt, 0, 0, r_d)
        assert len(d) == len(r_d), (c, dt)                       # the model's parity classes are the dispatch's launches
        classes |= {(dt, "dgrad", l.kclass) for l in d}
        classes.add((dt, "wgrad", pm.wgrad_class(c)))
    assert classes == {(dt, op, k) for dt in (0, 1) for (op, ks) in (("fwd", (0, 1)), ("dgrad", (0, 1)), ("wgrad", (2, 3))) for k in ks}
    # every kernel family a ResNet layer can reach (include/r3m_hip.h r3m_debug_conv_route; 22, the generic kernel, serves no layer of a
    # network: channel counts that are no multiple of 64) and every weight-gradient route route_sig names
    assert families[0] == {1, 11, 12, 13, 20, 21} and families[1] == {30, 31, 32}
    assert wg[0] == set(route_sig.WG_ROUTES[0]) and wg[1] == set(route_sig.WG_ROUTES[1])
    # a wide class reached only through the bf16 kernel-row route (64 output channels), and split-K factors of 1 and more
    assert any(dt == 1 and c[4] % 128 and pm.forward_launches(c, dt, 0, route_sig.routes(L, c, 0, 0, 0, dt))[0].kclass == pm.GEMM_WIDE
               for c, dt in pc.conv_cases())
    splits = {route_sig.wgrad_plan(L, c, dt).split > 1 for c, dt in pc.conv_cases()}
    assert splits == {False, True}
    assert len(pc.conv_cases()) <= 64 and max(pc.work(c) for c, _ in pc.conv_cases()) < 5e8      # small: the whole file takes seconds
