"""-m gpu: the max-pool and the fused stem tail of csrc/bn_pool.hip element by element at their launch edges, through the C ABI, in fp32
and bf16. The case lists, the lattice inputs and the float64 references are tests/pool_cases.py; tests/test_pool_cases.py checks on the
CPU (r3m_debug_pool_geometry) that the lists hold a case on each side of every launch condition and that the references agree with
F.max_pool2d(return_indices=True).

What is compared, and how:
  r3m_maxpool_fwd_dt            pooled values and argmax bytes EQUAL the reference: first maximum in row-major scan order, ties included
  r3m_maxpool_bwd_dt            on the reference's codes: dz EQUALS the scatter
  r3m_bn_relu_maxpool_fwd_dt    pooled values and argmax bytes EQUAL the reference (the bf16 row-walking kernel and, at C = 24, the
                                one-output-per-thread kernel in bf16 too)
  r3m_bn_maxpool_bwd_dt         use_batch_stats = 0 (fine-tuning with frozen statistics): dy = scale g, dbeta = sum g, dgamma = sum g yhat
                                EQUAL the float64 reference, accumulate = 1 gives base + sum. use_batch_stats = 1, accumulate 0 / 1: the
                                ceilings of tests/test_gpu_bn.py (TOL, util.rel_err against float64 on the same coefficients, its witness
                                rule for 1..3 rows), guarded by util.assert_range; plus the continuous-valued body of
                                test_gpu_ops_hw.py::test_stem_tail_fused_vs_torch_hw at two of the edge shapes.
The equalities hold because every input lies on a lattice on which the kernels' arithmetic is exact (tests/pool_cases.py).

Every output is filled with NaN (argmax bytes: 255) and sits between two guards of 64 sentinel elements inside its own allocation, which
are checked after the call; refusals must return non-zero before any launch and leave the fill as it was.

profiles/pool_edges_mutants.txt: five value mutants of csrc/bn_pool.hip (each in bounds, reasons there) and which of these tests fails
each."""
import numpy as np
import pytest
import torch

import pool_cases as pc
from test_gpu_bn import TOL, check_bwd
from util import DEV, assert_guard_intact, assert_range, check_stem_tail_fused_vs_torch, guarded_bytes

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16")
G = pc.GUARD
SENTINEL = -7.0e30              # guard value of the floating-point buffers (finite in bf16); argmax guards hold 0xA5
FUSED = [(n, s, d) for (n, s) in pc.FUSED_CASES for d in DTYPES]
FUSED_BWD = [(n, s, d) for (n, s, d) in FUSED if pc.has_backward(s[3])]
PLAIN = [(n, s, d) for (n, s) in pc.MAXPOOL_CASES for d in DTYPES]
ids = lambda v: v if isinstance(v, str) else "x".join(map(str, v))


def st():
    return torch.cuda.current_stream().cuda_stream


def tdt(dtype):
    return torch.float32 if dtype == "fp32" else torch.bfloat16


def dti(dtype):
    return 0 if dtype == "fp32" else 1


def dev(a, dtype=None):
    """numpy float64 -> device tensor of the case's storage type (fp32 when dtype is None), uint8 stays uint8"""
    t = torch.tensor(a)
    return t.to(DEV) if t.dtype == torch.uint8 else t.to(torch.float32).to(DEV).to(torch.float32 if dtype is None else tdt(dtype))


class Out:
    """an output of n elements, pre-filled, between two guards of G sentinel elements inside the same allocation"""

    def __init__(self, n, dt, fill=float("nan"), init=None):
        self.n, self.sent = n, (0xA5 if dt == torch.uint8 else SENTINEL)
        self.buf = torch.full((n + 2 * G,), self.sent, dtype=dt, device=DEV)
        self.body = self.buf[G:G + n]
        if init is None:
            self.body.fill_(fill)
        else:
            self.body.copy_(init)
        self.ptr = self.body.data_ptr()
        assert self.ptr % 16 == 0

    def check_guards(self, what):
        want = torch.tensor(self.sent, dtype=self.buf.dtype)
        for side, g in (("before", self.buf[:G]), ("behind", self.buf[G + self.n:])):
            bad = torch.nonzero(g.cpu() != want).flatten()
            assert bad.numel() == 0, f"{what}: {bad.numel()} guard elements {side} the buffer were overwritten (first at {bad[:4].tolist()})"

    def values(self):
        b = self.body.cpu()
        return b.numpy() if b.dtype == torch.uint8 else b.double().numpy()

    def untouched(self):
        b = self.body.cpu()
        return bool((b == 255).all()) if b.dtype == torch.uint8 else bool(torch.isnan(b.float()).all())


def assert_equal(what, got, ref):
    """element by element, nothing masked or left out"""
    ref = np.asarray(ref).reshape(-1)
    assert got.shape == ref.shape
    bad = np.nonzero(~(got == ref))[0]
    if bad.size:
        i = bad[:6]
        pytest.fail(f"{what}: {bad.size} of {ref.size} elements differ, first at {i.tolist()}: got {got[i].tolist()} reference {ref[i].tolist()}")


# ---- the plain max-pool ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,dtype", PLAIN, ids=ids)
def test_maxpool_forward_and_backward(hip, name, shape, dtype):
    N, Hi, Wi, C = shape
    c = pc.maxpool_case(shape)
    zd = dev(c["z"], dtype)
    p, am = Out(c["p"].size, tdt(dtype)), Out(c["code"].size, torch.uint8, 255)
    assert hip.r3m_maxpool_fwd_dt(zd.data_ptr(), p.ptr, am.ptr, N, Hi, Wi, C, dti(dtype), st()) == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    p.check_guards("pooled values"), am.check_guards("argmax bytes")
    assert_equal("pooled values", p.values(), c["p"])
    assert_equal("argmax bytes (first maximum in scan order)", am.values(), c["code"])
    dpd, coded = dev(c["dp"], dtype), dev(c["code"])
    dz = Out(c["dz"].size, tdt(dtype))
    assert hip.r3m_maxpool_bwd_dt(dpd.data_ptr(), coded.data_ptr(), dz.ptr, N, Hi, Wi, C, dti(dtype), st()) == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    dz.check_guards("dz")
    assert_equal("dz", dz.values(), c["dz"])


# ---- the fused stem tail ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,dtype", FUSED, ids=ids)
def test_fused_forward(hip, name, shape, dtype):
    N, Hi, Wi, C = shape
    c = pc.fused_case(shape)
    yd, coefd = dev(c["y"], dtype), dev(c["coef"])
    p, am = Out(c["p"].size, tdt(dtype)), Out(c["code"].size, torch.uint8, 255)
    rc = hip.r3m_bn_relu_maxpool_fwd_dt(yd.data_ptr(), coefd.data_ptr(), p.ptr, am.ptr, N, Hi, Wi, C, dti(dtype), st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    p.check_guards("pooled values"), am.check_guards("argmax bytes")
    assert_equal("pooled values", p.values(), c["p"])
    assert_equal("argmax bytes (first maximum in scan order)", am.values(), c["code"])


def run_fused_bwd(hip, c, shape, dtype, ubs, acc, bases):
    """r3m_bn_maxpool_bwd_dt on the reference's codes -> (dgamma, dbeta, dy) as Out buffers, guards checked"""
    N, Hi, Wi, C = shape
    yd, coefd, dpd, coded = dev(c["y"], dtype), dev(c["coef"]), dev(c["dp"], dtype), dev(c["code"])
    wsb = hip.r3m_bn_workspace_bytes(N * Hi * Wi, C)
    ws = guarded_bytes(wsb)
    dg = Out(C, torch.float32, init=dev(bases[0]) if acc else None)
    db = Out(C, torch.float32, init=dev(bases[1]) if acc else None)
    dy = Out(c["y"].size, tdt(dtype))
    rc = hip.r3m_bn_maxpool_bwd_dt(dpd.data_ptr(), coded.data_ptr(), yd.data_ptr(), coefd.data_ptr(), dg.ptr, db.ptr, dy.ptr, ws.data_ptr(), wsb,
                                   N, Hi, Wi, C, ubs, acc, dti(dtype), st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    for what, o in (("dgamma", dg), ("dbeta", db), ("dy", dy)):
        o.check_guards(what)
    assert_guard_intact(ws, wsb, "r3m_bn_maxpool_bwd_dt")
    return dg, db, dy


@pytest.mark.parametrize("name,shape,dtype", FUSED_BWD, ids=ids)
def test_fused_backward_frozen_statistics(hip, name, shape, dtype):
    """use_batch_stats = 0, what fine-tuning with frozen statistics runs: every output EQUALS the float64 reference, and accumulate = 1
    onto lattice bases gives base + sum"""
    C = shape[3]
    c = pc.fused_case(shape)
    bases = pc.lattice_bases(C)
    for acc in (0, 1):
        dg, db, dy = run_fused_bwd(hip, c, shape, dtype, 0, acc, bases)
        assert_equal(f"accumulate={acc} dy", dy.values(), c["dy"])
        assert_equal(f"accumulate={acc} dbeta", db.values(), c["dbeta"] + (bases[1] if acc else 0.0))
        assert_equal(f"accumulate={acc} dgamma", dg.values(), c["dgamma"] + (bases[0] if acc else 0.0))


@pytest.mark.parametrize("name,shape,dtype", FUSED_BWD, ids=ids)
def test_fused_backward_batch_statistics(hip, name, shape, dtype):
    """use_batch_stats = 1, accumulate 0 / 1, under the ceilings of tests/test_gpu_bn.py (and its witness rule for 1..3 rows) against
    float64 on the same coefficients"""
    N, Hi, Wi, C = shape
    rows = N * Hi * Wi
    c = pc.fused_case(shape)
    bases = pc.lattice_bases(C)
    ref = tuple(torch.tensor(a) for a in pc.train_bwd_ref(c))
    wit = tuple(torch.tensor(a) for a in pc.train_bwd_ref(c, np.float32))
    g, yhat, scale = torch.tensor(c["g"]).reshape(rows, C), torch.tensor(c["yhat"]).reshape(rows, C), torch.tensor(c["coef"][2])
    if rows > 1:          # one row: dy = scale (g - g - yhat g yhat) is an exact zero on both sides when yhat = +-1, tiny otherwise
        assert_range(ref[2], [scale * g, scale * g.mean(0), scale * yhat * (g * yhat).mean(0)], "dy")
    assert TOL[dtype]["dy"] == (2e-4 if dtype == "fp32" else 2.0 ** -8) and TOL[dtype]["dg"] == (1e-4 if dtype == "fp32" else 2e-4)
    b0 = tuple(torch.tensor(b).float() for b in bases)
    for acc in (0, 1):
        dg, db, dy = run_fused_bwd(hip, c, shape, dtype, 1, acc, bases)
        got = (dg.body, db.body, dy.body.reshape(rows, C))
        assert all(bool(torch.isfinite(t.float()).all()) for t in got)
        check_bwd(f"{name} use_batch_stats=1 accumulate={acc}", rows, dtype, got, ref, wit, b0 if acc else (None, None))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 40, 16, 64), (1, 3, 258, 64)], ids=lambda s: "{}x{}x{}x{}".format(*s))
def test_fused_continuous_values(hip, shape, dtype):
    """the body of test_gpu_ops_hw.py::test_stem_tail_fused_vs_torch_hw (continuous coefficients, batch statistics of y) where the reduce
    runs 15 quad rows per block and where the thread loops take a second trip"""
    N, Hi, Wi, C = shape
    check_stem_tail_fused_vs_torch(hip, N, Hi, Wi, C, dtype)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_the_outputs_alone(hip, dtype):
    """a backward with C = 24 or C = 2048, a workspace that is too small, a null argument, an unknown dtype, a forward with C no multiple
    of 8: non-zero before any launch, the NaN fill intact"""
    N, Hi, Wi = 2, 5, 6
    Ho, Wo = pc.out_hw(Hi, Wi)

    def attempt(C, what, ws_short=0, null=None, dt=dti(dtype)):
        rows = N * Hi * Wi
        yd = torch.zeros((rows, C), dtype=tdt(dtype), device=DEV)
        dpd = torch.ones((N * Ho * Wo, C), dtype=tdt(dtype), device=DEV)
        am = torch.full((N * Ho * Wo, C), 4, dtype=torch.uint8, device=DEV)
        coefd = torch.ones((4, C), device=DEV)
        wsb = hip.r3m_bn_workspace_bytes(rows, C)
        ws = guarded_bytes(wsb)
        dg, db, dy = Out(C, torch.float32), Out(C, torch.float32), Out(rows * C, tdt(dtype))
        a = dict(dp=dpd.data_ptr(), am=am.data_ptr(), y=yd.data_ptr(), coef=coefd.data_ptr(), dg=dg.ptr, db=db.ptr, dy=dy.ptr, ws=ws.data_ptr())
        if null:
            a[null] = None
        rc = hip.r3m_bn_maxpool_bwd_dt(a["dp"], a["am"], a["y"], a["coef"], a["dg"], a["db"], a["dy"], a["ws"], wsb - ws_short, N, Hi, Wi, C, 1, 0,
                                       dt, st())
        torch.cuda.synchronize()
        assert rc != 0 and hip.r3m_last_error(), what
        for o in (dg, db, dy):
            assert o.untouched(), what
            o.check_guards(what)
        assert_guard_intact(ws, wsb, what)

    attempt(24, "backward with C = 24")
    attempt(2048, "backward with C = 2048")
    attempt(64, "workspace one byte short", ws_short=1)
    for null in ("dp", "am", "y", "coef", "dg", "db", "dy", "ws"):
        attempt(64, f"null {null}", null=null)
    attempt(64, "unknown dtype", dt=2)

    for C, null, dt, what in ((12, None, dti(dtype), "forward with C = 12"), (64, "p", dti(dtype), "forward, null p"), (64, "am", dti(dtype), "forward, null argmax"),
                              (64, None, 2, "forward, unknown dtype")):
        yd = torch.zeros((N * Hi * Wi, C), dtype=tdt(dtype), device=DEV)
        coefd = torch.ones((4, C), device=DEV)
        p, am = Out(N * Ho * Wo * C, tdt(dtype)), Out(N * Ho * Wo * C, torch.uint8, 255)
        rc = hip.r3m_bn_relu_maxpool_fwd_dt(yd.data_ptr(), coefd.data_ptr(), None if null == "p" else p.ptr, None if null == "am" else am.ptr,
                                            N, Hi, Wi, C, dt, st())
        torch.cuda.synchronize()
        assert rc != 0 and hip.r3m_last_error(), what
        assert p.untouched() and am.untouched(), what
        p.check_guards(what), am.check_guards(what)
