"""The launch profiler (csrc/capi.hip prof_begin / prof_bytes / prof_end, r3m_profile_*) against tests/profile_model.py: every figure
bench.py derives per kernel class -- launches, FLOPs, algorithmic bytes, times -- the CSV of r3m_profile_dump_to, the switches bench.py
uses between its probe and its timed steps, and that bracketing changes no result bit. Operator level on the smallest members of the
operator tests' case lists (tests/profile_cases.py), then the engine under autograd (the backward runs on autograd's thread).

Every comparison of counts, FLOPs and bytes is exact: both sides are integers (or multiples of 1/8) far below 2^53 held in doubles."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import torch

import profile_cases as pc
import profile_model as pm
import route_sig
from util import DEV, _st

pytestmark = pytest.mark.gpu

HEADER = "class,M,N,K,taps,ms,gflop,alg_mbytes"
OPS = ("fwd", "fwd_stats", "dgrad", "wgrad")


# ---- the instrument ---------------------------------------------------------------------------------------------------------------------
def collect(hip):
    ms, n, fl, by = (C.c_double * 4)(), (C.c_longlong * 4)(), (C.c_double * 4)(), (C.c_double * 4)()
    assert hip.r3m_profile_collect(ms, n, fl) == 0, hip.r3m_last_error()
    assert hip.r3m_profile_collect_bytes(by) == 0, hip.r3m_last_error()
    return dict(ms=list(ms), launches=list(n), flops=list(fl), bytes=list(by))


class profiled:
    """`with profiled(hip) as p: ...` then p.got = what collect returned and p.outer_ms = the time between two events recorded on the
    current stream around the body; profiling is off again afterwards whatever happened"""

    def __init__(self, hip, csv=None):
        self.hip, self.csv = hip, csv

    def __enter__(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if self.csv is not None:
            assert self.hip.r3m_profile_dump_to(str(self.csv).encode()) == 0, self.hip.r3m_last_error()
        self.hip.r3m_profile_enable(1)
        self.e0.record()
        return self

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                self.e1.record()
                torch.cuda.synchronize()
                self.got = collect(self.hip)
                self.outer_ms = self.e0.elapsed_time(self.e1)
        finally:
            self.hip.r3m_profile_enable(0)
            self.hip.r3m_profile_dump_to(None)
        return False


@functools.lru_cache(maxsize=None)
def event_granularity_ms():
    """the largest elapsed_time between back-to-back event pairs on an idle stream: what two timestamps of the same instant can differ by"""
    torch.cuda.synchronize()
    worst = 0.0
    for _ in range(200):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        b.record()
        b.synchronize()
        worst = max(worst, a.elapsed_time(b))
    print(f"ACCT event granularity: largest elapsed_time of 200 back-to-back event pairs on an idle stream = {worst * 1e3:.2f} us")
    return worst


def assert_accounting(got, model, what, outer_ms=None):
    """collected figures against the model's launches, class by class; times finite, positive and inside the outer pair of events"""
    want = pm.totals(model)
    print(f"ACCT {what}: collected launches {got['launches']} flops {[int(f) for f in got['flops']]} bytes {got['bytes']} | model "
          f"launches {[t[0] for t in want]} flops {[t[1] for t in want]} bytes {[float(t[2]) for t in want]}")
    assert got["launches"] == [t[0] for t in want], f"{what}: launches per class"
    assert got["flops"] == [float(t[1]) for t in want], f"{what}: FLOPs per class"
    assert got["bytes"] == [float(t[2]) for t in want], f"{what}: algorithmic bytes per class"
    for k in range(4):
        if want[k][0]:
            assert np.isfinite(got["ms"][k]) and got["ms"][k] > 0, f"{what}: class {k} took {got['ms'][k]} ms"
        else:
            assert got["ms"][k] == 0.0
    if outer_ms is not None:
        allow = 2 * event_granularity_ms() * len(model)
        print(f"ACCT {what}: bracketed {sum(got['ms']):.4f} ms inside {outer_ms:.4f} ms (+ {allow:.4f} allowed)")
        assert sum(got["ms"]) <= outer_ms + allow, f"{what}: the brackets sum to {sum(got['ms'])} ms, the call took {outer_ms} ms"


def read_csv(path):
    lines = open(path).read().split("\n")
    assert lines[0] == HEADER and lines[-1] == "", lines[:1]
    return [ln.split(",") for ln in lines[1:-1]]


def assert_csv(rows, model, got, what):
    assert len(rows) == len(model), f"{what}: {len(rows)} CSV rows for {len(model)} launches"
    for r, l in zip(rows, model):
        assert [int(v) for v in r[:5]] == [l.kclass, l.M, l.N, l.K, l.taps], f"{what}: CSV row {r} against {l}"
        assert float(r[5]) >= 0
    # the file prints three decimals: each row is within half a unit of the last place of its launch
    assert abs(sum(float(r[6]) for r in rows) - sum(got["flops"]) * 1e-9) <= 0.5e-3 * len(rows) + 1e-9, what
    assert abs(sum(float(r[7]) for r in rows) - sum(got["bytes"]) * 1e-6) <= 0.5e-3 * len(rows) + 1e-9, what


# ---- operator level ---------------------------------------------------------------------------------------------------------------------
def dev_rand(shape, seed, dt, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = (torch.rand(shape, generator=g) * 2 - 1) * scale
    return t.to(DEV).to(torch.bfloat16 if dt else torch.float32).contiguous()


def operator(hip, case, dt, op):
    """(call, model): call() runs the stand-alone entry point of `op` into NaN-filled outputs and returns them; model: its launches"""
    N, Hi, Wi, Ci, Co, k, s, p = case
    Ho, Wo = pm.out_hw(case)
    tdt = torch.bfloat16 if dt else torch.float32
    x, dy = dev_rand((N, Hi, Wi, Ci), 1, dt), dev_rand((N, Ho, Wo, Co), 3, dt)
    w32 = dev_rand((Co, k, k, Ci), 2, 0, 0.2)
    nan = lambda shape, t=tdt: torch.full(shape, float("nan"), dtype=t, device=DEV)
    L = hip
    if op in ("fwd", "fwd_stats"):
        w = w32.to(tdt)
        rows = hip.r3m_conv2d_stats_rows(N, Hi, Wi, Co, k, s, p) if op == "fwd_stats" else 0
        flags = route_sig.STATS if rows else 0

        def call():
            y, st = nan((N, Ho, Wo, Co)), (nan((rows, 2, Co), torch.float32) if rows else None)
            rc = hip.r3m_conv2d_fwd_dt(x.data_ptr(), w.data_ptr(), y.data_ptr(), None if st is None else st.data_ptr(), N, Hi, Wi, Ci, Co, k, s, p,
                                       dt, _st())
            assert rc == 0, hip.r3m_last_error()
            return [y] + ([st] if rows else [])
        return call, pm.forward_launches(case, dt, flags, route_sig.routes(L, case, 0, flags, 0, dt), rows)
    if op == "dgrad":
        wsb = hip.r3m_conv2d_dgrad_workspace_bytes(Ci, Co, k)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)

        def call():
            dx = nan((N, Hi, Wi, Ci))
            rc = hip.r3m_conv2d_dgrad_dt(dy.data_ptr(), w32.data_ptr(), dx.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, dt, _st())
            assert rc == 0, hip.r3m_last_error()
            return [dx]
        routes = route_sig.routes(L, case, 1, 0, 0, dt)
        model = pm.dgrad_launches(case, dt, 0, 0, routes)
        assert len(model) == len(routes), (case, routes)
        return call, model
    assert op == "wgrad"
    wsb = hip.r3m_conv2d_wgrad_workspace_bytes_dt(N, Hi, Wi, Ci, Co, k, s, p, dt)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)

    def call():
        dw = nan((Co, k, k, Ci), torch.float32)
        rc = hip.r3m_conv2d_wgrad_dt(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb, N, Hi, Wi, Ci, Co, k, s, p, 0, dt, _st())
        assert rc == 0, hip.r3m_last_error()
        return [dw]
    return call, pm.wgrad_launches(case, dt, route_sig.wgrad_plan(L, case, dt).split)


def assert_same_bits(plain, bracketed, what):
    for a, b in zip(plain, bracketed):
        assert not bool(torch.isnan(a.float()).any()), f"{what}: an output element was not written"
        assert torch.equal(a, b), f"{what}: bracketing changed a result"


def check_operator(hip, tmp_path, call, model, what):
    plain = call()
    torch.cuda.synchronize()
    assert collect(hip)["launches"] == [0, 0, 0, 0], f"{what}: launches counted with profiling off"
    csv = tmp_path / "launches.csv"
    with profiled(hip, csv) as p:
        bracketed = call()
    assert_same_bits(plain, bracketed, what)
    assert_accounting(p.got, model, what, p.outer_ms)
    assert_csv(read_csv(csv), model, p.got, what)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("case,dt", pc.conv_cases(), ids=pc.case_id)
def test_operator_accounting(hip, tmp_path, case, dt, op):
    call, model = operator(hip, case, dt, op)
    check_operator(hip, tmp_path, call, model, f"{op} {pc.case_id(dt)} {case}")
    if op == "dgrad" and case[6] > 1:
        rows = read_csv(tmp_path / "launches.csv")
        assert sum(int(r[1]) * int(r[4]) for r in rows) == case[0] * pm.dgrad_pairs(case)      # sum of M x taps = the enumerated pairs


@pytest.mark.parametrize("dt", [0, 1], ids=pc.case_id)
@pytest.mark.parametrize("stats", [0, 1], ids=["plain", "stats"])
@pytest.mark.parametrize("case", pc.STEM_CASES, ids=lambda c: "F{}_{}x{}".format(*c))
def test_stem_accounting(hip, tmp_path, case, dt, stats):
    """the general stem's forward and weight gradient: narrow launches of M = F Ho Wo rows, 64 columns, K = 147"""
    F, H, W = case
    Ho, Wo = pm.stem_hw(H, W)
    tdt = torch.bfloat16 if dt else torch.float32
    assert hip.r3m_stem_gen_image_bytes(F, H, W, dt) == F * H * W * 3 * pm.esize(dt)
    xn, dy, w = dev_rand((F, H, W * 3), 1, dt), dev_rand((F, Ho, Wo, 64), 3, dt), dev_rand((64, 7, 7, 3), 2, 0, 0.2)
    rows = -(-F * Ho * Wo // 256) if stats else 0

    def fwd():
        y = torch.full((F, Ho, Wo, 64), float("nan"), dtype=tdt, device=DEV)
        st = torch.full((rows, 2, 64), float("nan"), device=DEV) if rows else None
        rc = hip.r3m_stem_gen_fwd(xn.data_ptr(), w.data_ptr(), y.data_ptr(), None if st is None else st.data_ptr(), F, H, W, dt, _st())
        assert rc == 0, hip.r3m_last_error()
        return [y] + ([st] if rows else [])
    check_operator(hip, tmp_path, fwd, pm.stem_launches(F, H, W, dt, "fwd", rows), f"stem forward {pc.case_id(dt)} {case} stats={stats}")
    if stats:
        return
    wsb = hip.r3m_stem_gen_wgrad_ws_bytes()
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)

    def wgrad():
        dw = torch.full((64, 7, 7, 3), float("nan"), device=DEV)
        rc = hip.r3m_stem_gen_wgrad(xn.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), F, H, W, 0, dt, _st())
        assert rc == 0, hip.r3m_last_error()
        return [dw]
    check_operator(hip, tmp_path, wgrad, pm.stem_launches(F, H, W, dt, "wgrad"), f"stem weight gradient {pc.case_id(dt)} {case}")


# ---- the switches bench.py uses -------------------------------------------------------------------------------------------------------------
def switch_ops(hip):
    """[(call, model)] of forward, input gradient and weight gradient of the two fp32 switch cases: launches of all four classes"""
    out = [operator(hip, c, 0, op) for c in pc.SWITCH_CASES for op in ("fwd", "dgrad", "wgrad")]
    assert {l.kclass for _, m in out for l in m} == {0, 1, 2, 3}
    return out


def run_all(ops):
    for call, _ in ops:
        call()


def test_csv_stops_at_null_and_a_bad_path_is_an_error(hip, tmp_path):
    ops = switch_ops(hip)
    csv = tmp_path / "launches.csv"
    assert hip.r3m_profile_dump_to(str(csv).encode()) == 0
    hip.r3m_profile_enable(1)
    try:
        run_all(ops)
        first = collect(hip)
        rows = read_csv(csv)
        assert len(rows) == sum(first["launches"]) == sum(len(m) for _, m in ops)
        assert hip.r3m_profile_dump_to(None) == 0
        run_all(ops)
        assert collect(hip)["launches"] == first["launches"]
        assert read_csv(csv) == rows, "a collect after r3m_profile_dump_to(NULL) appended to the file"
        bad = tmp_path / "no_such_directory" / "launches.csv"
        assert hip.r3m_profile_dump_to(str(bad).encode()) != 0
        assert "no_such_directory" in hip.r3m_last_error().decode()
        run_all(ops)
        assert collect(hip)["launches"] == first["launches"]           # and profiling goes on without a file
    finally:
        hip.r3m_profile_enable(0)
        hip.r3m_profile_dump_to(None)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_class_mask_counts_only_its_class(hip, k):
    ops = switch_ops(hip)
    want = pm.totals([l for _, m in ops for l in m])
    old = hip.r3m_profile_classes(1 << k)
    try:
        assert old & 0xF == 0xF                                     # every class is bracketed by default
        assert hip.r3m_profile_classes(1 << k) == 1 << k          # returns the previous mask
        with profiled(hip) as p:
            run_all(ops)
        for j in range(4):
            assert p.got["launches"][j] == (want[j][0] if j == k else 0), (k, p.got)
            assert p.got["flops"][j] == (float(want[j][1]) if j == k else 0.0)
            assert p.got["bytes"][j] == (float(want[j][2]) if j == k else 0.0)
    finally:
        hip.r3m_profile_classes(0xF)
    with profiled(hip) as p:
        run_all(ops)
    assert p.got["launches"] == [t[0] for t in want]


def test_second_collect_returns_zeros(hip):
    ops = switch_ops(hip)
    hip.r3m_profile_enable(1)
    try:
        run_all(ops)
        first = collect(hip)
        second = collect(hip)
    finally:
        hip.r3m_profile_enable(0)
    assert sum(first["launches"]) == sum(len(m) for _, m in ops)
    assert second == dict(ms=[0.0] * 4, launches=[0] * 4, flops=[0.0] * 4, bytes=[0.0] * 4)


def test_disable_drops_what_was_recorded_and_off_counts_nothing(hip):
    ops = switch_ops(hip)
    hip.r3m_profile_enable(1)
    run_all(ops)
    hip.r3m_profile_enable(0)                    # what bench.py does between its probe and its timed steps
    assert collect(hip)["launches"] == [0, 0, 0, 0]
    run_all(ops)                                 # profiling off
    assert collect(hip)["launches"] == [0, 0, 0, 0]
    with profiled(hip) as p:                     # nothing stale is added to the next measurement
        run_all(ops)
    assert_accounting(p.got, [l for _, m in ops for l in m], "after a dropped measurement")


def test_a_refused_launch_leaves_nothing_behind(hip):
    """fp32 weight gradient with Ci = 6 (no multiple of 4) is refused; the good launches after it are counted alone, also when the next
    launch is of a class the mask leaves out (it must not close a bracket the refused launch left open)"""
    N, Hi, Wi, Ci, Co = 2, 9, 7, 6, 64
    x, dy = dev_rand((N, Hi, Wi, Ci), 1, 0), dev_rand((N, Hi, Wi, Co), 3, 0)
    dw = torch.zeros((Co, 1, 1, Ci), device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    ops = switch_ops(hip)

    def refused():
        rc = hip.r3m_conv2d_wgrad_dt(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(), N, Hi, Wi, Ci, Co, 1, 1, 0, 0, 0, _st())
        assert rc != 0 and b"multiples of 4" in hip.r3m_last_error()

    with profiled(hip) as p:
        refused()
        run_all(ops)
    assert_accounting(p.got, [l for _, m in ops for l in m], "after a refused launch", p.outer_ms)
    old = hip.r3m_profile_classes(1 << 0)
    try:
        with profiled(hip) as p:
            refused()
            run_all(ops)
        assert_accounting(p.got, [l for _, m in ops for l in m if l.kclass == 0], "after a refused launch, class 0 only", p.outer_ms)
    finally:
        hip.r3m_profile_classes(old)


# ---- engine level -------------------------------------------------------------------------------------------------------------------------
F_ENGINE, HW_ENGINE = 2, (64, 96)


def _encoder(size, precision, train):
    from test_gpu_inference_session import _encoder as make
    return make(size, precision, train=train)


def _frames(tag):
    from test_gpu_inference_session import _frames as make
    return make(tag, F_ENGINE, *HW_ENGINE)


def engine_model(L, size, dt):
    """the bracketed launches of one training forward, its backward, and one inference forward of a plan at F_ENGINE x HW_ENGINE"""
    F, (H, W) = F_ENGINE, HW_ENGINE
    h = L.r3m_resnet_create_hw(size, F, dt, H, W)
    assert h, L.r3m_last_error()
    try:
        table = route_sig.plan_convs(L, h)
        convs = [(F, c[5], c[6], c[0], c[1], c[2], c[3], c[4]) for c in table]
    finally:
        L.r3m_resnet_destroy(h)
    Ho, Wo = pm.stem_hw(H, W)
    assert convs[0] == (F, H, W, 3, 64, 7, 2, 3)
    launches = route_sig.engine_launches(L, size, dt, F, H, W)
    fwd_train = pm.stem_launches(F, H, W, dt, "fwd", -(-F * Ho * Wo // 256))
    bwd = pm.stem_launches(F, H, W, dt, "wgrad")
    infer = pm.stem_launches(F, H, W, dt, "fwd", 0)
    fused = [False]            # per inference launch: the convolution stores the activated output itself
    # engine_launches lists per block: (statistics, plain) forward of each of its n convolutions, its input gradients, then the n
    # forwards of inference (fused stores where the whole block fuses, else plain ones followed by stand-alone BatchNorm passes)
    it = iter(launches)
    for body, ds in route_sig.plan_blocks(table, size):
        n = len(body) + (1 if ds else 0)
        seen_fwd = 0
        while seen_fwd < 3 * n:
            c, dgrad, flags, bits = next(it)
            r = route_sig.routes(L, c, dgrad, flags, bits, dt)
            assert r, (c, dgrad, flags, bits)
            if dgrad:
                m = pm.dgrad_launches(c, dt, flags, bits, r)
                assert len(m) == len(r), (c, flags, r)
                bwd += m
                continue
            seen_fwd += 1
            if seen_fwd > 2 * n:
                infer += pm.forward_launches(c, dt, flags, r)
                fused.append(bool(flags & route_sig.AFFINE))
            elif flags == route_sig.STATS:
                fwd_train += pm.forward_launches(c, dt, flags, r, L.r3m_conv2d_stats_rows(*c[:3], c[4], *c[5:]))
    assert next(it, None) is None
    for c in convs[1:]:
        bwd += pm.wgrad_launches(c, dt, route_sig.wgrad_plan(L, c, dt).split)
    assert len(fwd_train) == len(infer) == len(convs)
    # total FLOPs: forward, the input gradient of every convolution but conv1, every weight gradient
    assert sum(l.flops for l in fwd_train) == pm.stem_flops(F, Ho, Wo) + sum(pm.forward_flops(c) for c in convs[1:])
    assert sum(l.flops for l in bwd) == pm.stem_flops(F, Ho, Wo) + sum(pm.dgrad_flops(c) + pm.wgrad_flops(c) for c in convs[1:])
    return fwd_train, bwd, infer, fused


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [18, 50])
def test_engine_training_step_accounting(hip, size, precision):
    """One training forward and backward through HipResNet under autograd with all four classes bracketed: the backward's launches come
    from autograd's thread and are counted like the forward's; with obs.requires_grad the stem's input gradient adds no launch (it is
    outside the four classes); the results are the bits of an unbracketed step."""
    dt = 0 if precision == "fp32" else 1
    fwd, bwd, _, _ = engine_model(hip, size, dt)
    x = _frames("prof")
    threads = []

    def step(want_dx):
        m = _encoder(size, precision, train=True)
        xs = x.clone().requires_grad_(want_dx)
        hh = m(xs)
        hh.register_hook(lambda g: threads.append(threading.get_ident()))
        (hh * torch.linspace(-1.0, 1.0, hh.numel(), device=DEV).view_as(hh)).sum().backward()
        torch.cuda.synchronize()
        return hh.detach().clone(), m.flat_grads().detach().clone(), (xs.grad.clone() if want_dx else None)

    plain = step(False)
    with profiled(hip) as p:
        got = step(False)
    assert threads and all(t != threading.get_ident() for t in threads), "the backward did not run on autograd's thread"
    assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1]), "bracketing changed the step's results"
    assert_accounting(p.got, fwd + bwd, f"ResNet-{size} {precision} training step")
    with profiled(hip) as p:
        got = step(True)
    assert got[2] is not None and bool(torch.isfinite(got[2]).all()) and torch.equal(plain[1], got[1])
    assert_accounting(p.got, fwd + bwd, f"ResNet-{size} {precision} training step with obs.requires_grad")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [18, 50])
def test_engine_inference_accounting(hip, size, precision):
    """eval forward under no_grad (fused epilogues): one bracketed launch per convolution; through an InferenceSession exactly the
    convolutions that r3m_debug_conv_small_plan does not take or whose block does not run the fused sequence (the few-row kernel of
    csrc/conv_small.hip, which only stores fused epilogues, is outside the four classes)"""
    dt = 0 if precision == "fp32" else 1
    _, _, infer, fused = engine_model(hip, size, dt)
    m = _encoder(size, precision, train=False)
    for q in m.parameters():
        q.requires_grad_(False)
    x = _frames("prof")
    with torch.no_grad():
        plain = m(x).clone()
        with profiled(hip) as p:
            got = m(x).clone()
    assert torch.equal(plain, got)
    assert_accounting(p.got, infer, f"ResNet-{size} {precision} inference forward")
    assert sum(p.got["launches"]) == len(infer)

    sess = m.inference_session()
    with torch.no_grad():
        sess(x)                                     # prepares
        with profiled(hip) as p:
            sess(x)
    plan = sess._plans[(F_ENGINE,) + HW_ENGINE]
    convs = route_sig.plan_convs(hip, plan)
    taken, buf = [], (C.c_int * 10)()
    for (Ci, Co, k, s, pad, Hi, Wi, Ho, Wo), fuses in zip(convs[1:], fused[1:]):
        assert hip.r3m_debug_conv_small_plan(F_ENGINE, Hi, Wi, Ci, Co, k, s, pad, 128 | 16, buf, 10) == 10
        taken.append(bool(buf[0]) and dt == 0 and fuses)       # fp32 plans only, and only where the block runs the fused sequence
    assert any(taken) == (dt == 0), "fp32 plans of two 64 x 96 frames have few-row launches, bf16 plans none"
    left = [infer[0]] + [l for l, t in zip(infer[1:], taken) if not t]
    assert_accounting(p.got, left, f"ResNet-{size} {precision} prepared forward")


@pytest.mark.parametrize("dt", [0, 1], ids=pc.case_id)
def test_head_linears_are_in_the_gemm_classes(hip, tmp_path, dt):
    """one r3m_langrew_forward at the smallest head shape: its four hidden Linears are bracketed as GEMM launches with taps = 1 and
    M, N, K = rows, outputs, inputs (the final Linear to one output is a reduction kernel outside the classes)"""
    B, D, H, LD = pc.HEAD_SHAPE_BF16 if dt else pc.HEAD_SHAPE
    R, K1 = 15 * B, 2 * D + LD
    n = hip.r3m_langrew_num_params(D, H, LD)
    params = dev_rand((n + (-n) % 4,), 5, 0, 0.1)
    alle, feats = dev_rand((B, 5, D), 6, 0), dev_rand((B, LD), 7, 0)
    perm = torch.arange(B, dtype=torch.int32, device=DEV).repeat(9, 1).contiguous()
    wsb = hip.r3m_langrew_workspace_bytes(B, D, H, LD)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)

    def call():
        scores = torch.full((15, B), float("nan"), device=DEV)
        rc = hip.r3m_langrew_forward_dt(alle.data_ptr(), feats.data_ptr(), perm.data_ptr(), params.data_ptr(), scores.data_ptr(), ws.data_ptr(), wsb,
                                        B, D, H, LD, dt, _st())
        assert rc == 0, hip.r3m_last_error()
        return [scores]
    flags = 0 if dt else pm.BIAS | pm.RELU
    model = [pm.forward_launches((R, 1, 1, K, H, 1, 1, 0), dt, flags)[0] for K in (K1, H, H, H)]
    assert [(l.M, l.N, l.K, l.taps) for l in model] == [(R, H, K1, 1)] + [(R, H, H, 1)] * 3
    check_operator(hip, tmp_path, call, model, f"language-reward head forward {pc.case_id(dt)} {(B, D, H, LD)}")
