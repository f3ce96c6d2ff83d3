"""-m gpu: the small-M split-K forward (csrc/conv_small.hip) through r3m_conv2d_fwd_affine_small, one launch at a time against float64
[relu](conv * scale + shift [+ residual]) on the CPU, built as util.check_conv_affine builds it: the same generators, assert_range, the
0.2 - 0.8 zero share under ReLU, and assert_close_store(..., "fp32") — the ceiling the other fp32 kernels meet for this very store.

Every launch: outputs (where no residual lives there) and the WHOLE workspace pre-filled with NaN, run twice, torch.equal. Every case
runs with the rule's S where the rule takes it and with forced splits: 1 (no ticket, no slab), 2, the largest accepted, one that leaves
a ragged last slice and one whose slice boundary falls inside a tap (tests/small_conv_cases.py; tests/test_small_conv_plan.py checks
the list without a GPU)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from small_conv_cases import A, ACCUM, AR, GPU_CASES, RELU, conv_small_plan, forced_splits
from util import DEV, _st, assert_close_store, assert_range, nchw, nhwc, rnd

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _operands(case):
    """x, w (NCHW / OIHW, CPU) and the float64 convolution: once per case, shared by its flag sets, never written"""
    N, Hi, Wi, Ci, Co, k, s, p = case
    x = rnd((N, Ci, Hi, Wi), 1)
    w = rnd((Co, Ci, k, k), 2, -0.2, 0.2)
    y = F.conv2d(x.double(), w.double(), stride=s, padding=p)
    return x, w, y


def _launch(hip, case, flags, split, xd, wd, sc, sh, res_d, shape):
    need = hip.r3m_conv2d_small_workspace_bytes(*case, split)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), float("nan"), device=DEV)
    out = res_d.clone() if res_d is not None else torch.full(shape, float("nan"), device=DEV)
    rc = hip.r3m_conv2d_fwd_affine_small(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), sc.data_ptr(), sh.data_ptr(), *case, flags, split,
                                         ws.data_ptr(), need, _st())
    assert rc == 0, hip.r3m_last_error()
    return out


@pytest.mark.parametrize("case,flags", [(c, fl) for c, fls in GPU_CASES for fl in fls])
def test_small_conv_against_float64(hip, case, flags):
    N, Hi, Wi, Ci, Co, k, s, p = case
    x, w, y = _operands(case)
    Ho, Wo = y.shape[2], y.shape[3]
    sd = float(y.pow(2).mean().sqrt())
    scale = rnd((Co,), 21, 0.5, 1.5)
    shift = rnd((Co,), 22, -0.6, 0.6) * sd
    res = rnd(tuple(y.shape), 23) * sd if flags & ACCUM else None
    terms = [y * scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1).expand_as(y)] + ([res.double()] if res is not None else [])
    t = sum(terms[1:], terms[0])
    ref = torch.relu(t) if flags & RELU else t
    what = f"small conv flags {flags} {case}"
    assert_range(ref, terms, what)
    if flags & RELU:
        zeros = float((ref == 0).double().mean())
        assert 0.2 <= zeros <= 0.8, f"{what}: {zeros:.2f} of the reference outputs are zero"
    if res is not None:
        assert float(res.abs().max()) > 0

    xd = nhwc(x).to(DEV)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    sc, sh = scale.to(DEV), shift.to(DEV)
    res_d = nhwc(res).to(DEV) if res is not None else None
    splits, _, _ = forced_splits(hip, case)
    if conv_small_plan(hip, case, flags)["take"]:
        splits = [0] + splits
    for split in splits:
        out = _launch(hip, case, flags, split, xd, wd, sc, sh, res_d, (N, Ho, Wo, Co))
        assert_close_store(f"{what} split {split}", nchw(out.cpu()), ref, "fp32")
        again = _launch(hip, case, flags, split, xd, wd, sc, sh, res_d, (N, Ho, Wo, Co))
        assert torch.equal(out, again), f"{what} split {split}: two launches differ"


def test_small_conv_refusals(hip):
    """a shape, a flag set, a split and a workspace the entry does not take: non-zero with a message, nothing launched"""
    t, o, ws = (torch.zeros(1 << 16, device=DEV) for _ in range(3))     # operands (read only), the output, the workspace
    ptr = t.data_ptr()

    def call(case, flags, split, ws_bytes):
        return hip.r3m_conv2d_fwd_affine_small(ptr, ptr, o.data_ptr(), ptr, ptr, *case, flags, split, ws.data_ptr(), ws_bytes, _st())

    ok = (1, 4, 4, 64, 64, 3, 1, 1)
    need = hip.r3m_conv2d_small_workspace_bytes(*ok, 2)
    assert 0 < need <= t.numel() * 4
    assert call(ok, AR, 2, need) == 0, hip.r3m_last_error()
    assert call((1, 4, 4, 48, 64, 3, 1, 1), AR, 0, need) != 0 and b"Ci must be a multiple of 32" in hip.r3m_last_error()
    assert call(ok, AR, 2, need - 1) != 0 and b"workspace" in hip.r3m_last_error()
    assert call(ok, RELU, 2, need) != 0 and b"flags" in hip.r3m_last_error()
    assert call(ok, A | 1, 2, need) != 0 and b"flags" in hip.r3m_last_error()
    top = conv_small_plan(hip, ok)["max_split"]
    assert call(ok, AR, top + 1, 1 << 18) != 0 and b"split" in hip.r3m_last_error()
    torch.cuda.synchronize()
