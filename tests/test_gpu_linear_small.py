"""-m gpu: the few-row Linear r3m_linear_fwd_small (the split-K kernel of csrc/conv_small.hip with the Linear stores bias, bias + ReLU,
bias + exact GELU), one launch at a time against float64 on the CPU. Operands as tests/test_gpu_small_conv.py generates them, the bias
+-0.6 of the product's rms; assert_range, the 0.2 - 0.8 zero share under ReLU and a pre-activation standard deviation of 0.3 - 3 under
GELU hold for the references (tests/test_linear_small_plan.py checks them without a GPU); the ceiling is assert_close_store(..., "fp32").

Every launch: the output and the WHOLE workspace pre-filled with NaN, the output inside a guarded buffer whose guard is checked, run
twice, torch.equal. Every case runs with the rule's S where the rule takes it and with the forced splits of tests/small_conv_cases.py."""
import pytest
import torch

from linear_small_cases import BR, GELU, GPU_CASES, RELU, geom, linear_small_plan, operands, reference
from small_conv_cases import forced_splits
from util import DEV, _st, assert_close_store, assert_guard_intact, assert_range, guarded_bytes

pytestmark = pytest.mark.gpu


def _launch(hip, case, flags, split, xd, wd, bd):
    M, K, N = case
    need = hip.r3m_linear_small_workspace_bytes(M, K, N, split)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), float("nan"), device=DEV)
    nbytes = M * N * 4
    buf = guarded_bytes(nbytes)
    out = buf[:nbytes].view(torch.float32).view(M, N)
    out.fill_(float("nan"))
    rc = hip.r3m_linear_fwd_small(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), M, K, N, flags, split, ws.data_ptr(), need,
                                  _st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    assert_guard_intact(buf, nbytes, f"linear {case} flags {flags} split {split}")
    return out.clone()


@pytest.mark.parametrize("case,flags", [(c, fl) for c, fls in GPU_CASES for fl in fls])
def test_linear_small_against_float64(hip, case, flags):
    M, K, N = case
    x, w, _ = operands(case)
    bias, pre, ref, terms = reference(case, flags)
    what = f"linear small flags {flags} {case}"
    assert_range(ref, terms, what)
    if flags & RELU:
        zeros = float((ref == 0).double().mean())
        assert 0.2 <= zeros <= 0.8, f"{what}: {zeros:.2f} of the reference outputs are zero"
    if flags & GELU:
        assert 0.3 <= float(pre.std()) <= 3.0, f"{what}: pre-activation standard deviation {float(pre.std()):.2f}"
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    splits, _, _ = forced_splits(hip, geom(case))
    if linear_small_plan(hip, case, flags)["take"]:
        splits = [0] + splits
    for split in splits:
        out = _launch(hip, case, flags, split, xd, wd, bd)
        assert_close_store(f"{what} split {split}", out.cpu().view(M, N, 1, 1), ref.view(M, N, 1, 1), "fp32")
        again = _launch(hip, case, flags, split, xd, wd, bd)
        assert torch.equal(out, again), f"{what} split {split}: two launches differ"


def test_linear_small_refusals(hip):
    """a short workspace, a split above the maximum and a null workspace with S > 1: non-zero with a message, nothing launched"""
    t, o, ws = (torch.zeros(1 << 16, device=DEV) for _ in range(3))     # operands (read only), the output, the workspace
    ptr = t.data_ptr()
    M, K, N = 4, 256, 64

    def call(split, ws_ptr, ws_bytes, flags=BR):
        return hip.r3m_linear_fwd_small(ptr, ptr, ptr, o.data_ptr(), M, K, N, flags, split, ws_ptr, ws_bytes, _st())

    need = hip.r3m_linear_small_workspace_bytes(M, K, N, 2)
    assert 0 < need <= ws.numel() * 4
    assert call(2, ws.data_ptr(), need) == 0, hip.r3m_last_error()
    assert call(2, ws.data_ptr(), need - 1) != 0 and b"workspace" in hip.r3m_last_error()
    top = linear_small_plan(hip, (M, K, N), BR)["max_split"]
    assert call(top + 1, ws.data_ptr(), 1 << 18) != 0 and b"split" in hip.r3m_last_error()
    assert call(2, None, 0) != 0 and b"workspace" in hip.r3m_last_error()
    assert call(1, None, 0) == 0, hip.r3m_last_error()                  # one slice: neither ticket nor slab
    assert call(2, ws.data_ptr(), need, 128 | 16) != 0 and b"flags" in hip.r3m_last_error()
    torch.cuda.synchronize()
