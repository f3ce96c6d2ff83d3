"""r3m_langrew_infer (csrc/lang.hip): the reward head's forward without a backward — concat (with the R0 == 1 broadcast), one ticket
memset, four Linear + ReLU on the few-row split-K kernel where its plan takes them, the final GEMV — against the float64 MLP on the CPU.

One 17-row input set per size; R in {1, 5, 16, 17} takes its first R rows, R0 in {1, R}. The ceiling is the one of
test_langrew_c_abi_vs_torch (tests/test_gpu_lang.py): max|d| <= 2e-5 of the reference's range, here the range of the 17-row reference.
That range is first asserted to be at least a quarter of the largest summand of the last layer (h4[r, k] w5[k], b5), so the relative
ceiling is not loosened by cancellation; the same assertion runs without a GPU below. The workspace is pre-filled with NaN, two calls
give equal bits."""
import functools

import pytest
import torch

from util import DEV, _st, langrew_layers, rnd

SIZES = [(64, 64, 32), (512, 1024, 768), (2048, 1024, 768)]
ROWS = 17
SEED = 0
CEIL = 2e-5


@functools.lru_cache(maxsize=None)
def _setup(size):
    """layers, inputs and the two float64 references (one row per frame; row 0 of e0 / le for every frame) of one size: built once"""
    D, H, LD = size
    layers = langrew_layers(D, H, LD, seed=SEED)
    e0 = torch.relu(rnd((ROWS, D), 1, -0.5, 1.0))
    eg = torch.relu(rnd((ROWS, D), 5, -0.5, 1.0))
    le = rnd((ROWS, LD), 2, -0.6, 0.6)
    flat = torch.cat([t.detach().reshape(-1) for l in layers for t in (l.weight, l.bias)])
    flat = torch.cat([flat, torch.zeros((-flat.numel()) % 4)])

    def mlp(a, b, c):
        x = torch.cat([a, b, c], -1).double()
        for l in layers[:-1]:
            x = torch.relu(x @ l.weight.detach().double().t() + l.bias.detach().double())
        w5, b5 = layers[-1].weight.detach().double().view(-1), layers[-1].bias.detach().double()
        top = max(float((x * w5).abs().max()), float(b5.abs().max()))
        return x @ w5 + b5, top

    per_row = mlp(e0, eg, le)
    one_first = mlp(e0[:1].expand(ROWS, -1), eg, le[:1].expand(ROWS, -1))
    return flat, e0, eg, le, {False: per_row, True: one_first}


def _range(size, one_first):
    ref, top = _setup(size)[4][one_first]
    rng = float(ref.abs().max())
    assert rng >= 0.25 * top > 0, f"{size}: score range {rng} against last-layer summands up to {top}"
    return ref, rng


@pytest.mark.parametrize("size", SIZES)
def test_reference_range_is_no_cancellation(size):
    """not gpu: what the GPU test asserts first, for the seed it uses"""
    for one_first in (False, True):
        _range(size, one_first)


def _call(hip, size, flat_d, e0, eg, le, R, R0, ws_bytes=None):
    D, H, LD = size
    need = hip.r3m_langrew_infer_workspace_bytes(R, D, H, LD)
    assert need > 0 and need % 4 == 0, hip.r3m_last_error()
    ws = torch.full((need // 4,), float("nan"), device=DEV)
    score = torch.full((R,), float("nan"), device=DEV)
    rc = hip.r3m_langrew_infer(e0.data_ptr(), eg.data_ptr(), le.data_ptr(), flat_d.data_ptr(), score.data_ptr(), ws.data_ptr(),
                               need if ws_bytes is None else ws_bytes, R, R0, D, H, LD, _st())
    return rc, score


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 5, 16, 17])
@pytest.mark.parametrize("size", SIZES)
def test_langrew_infer_against_float64(hip, size, R):
    flat, e0, eg, le, _ = _setup(size)
    flat_d, e0d, egd, led = flat.to(DEV), e0.to(DEV), eg.to(DEV), le.to(DEV)
    for R0 in sorted({1, R}):
        one_first = R0 == 1 and R > 1
        refs = [_range(size, one_first)] if R > 1 else [_range(size, False), _range(size, True)]   # R = 1: both readings agree in row 0
        a0, l0 = (e0d[:1].contiguous(), led[:1].contiguous()) if R0 == 1 else (e0d[:R].contiguous(), led[:R].contiguous())
        rc, score = _call(hip, size, flat_d, a0, egd[:R].contiguous(), l0, R, R0)
        assert rc == 0, hip.r3m_last_error()
        rc, again = _call(hip, size, flat_d, a0, egd[:R].contiguous(), l0, R, R0)
        assert rc == 0, hip.r3m_last_error()
        torch.cuda.synchronize()
        for ref, rng in refs:
            err = float((score.cpu().double() - ref[:R]).abs().max()) / rng
            print(f"langrew_infer {size} R {R} R0 {R0}: max|d| / range {err:.3e}")
            assert err <= CEIL, (size, R, R0, err)
        assert torch.equal(score, again), (size, R, R0)


@pytest.mark.gpu
def test_langrew_infer_refusals(hip):
    size = SIZES[0]
    D, H, LD = size
    flat, e0, eg, le, _ = _setup(size)
    flat_d, e0d, egd, led = flat.to(DEV), e0.to(DEV), eg.to(DEV), le.to(DEV)
    rc, _ = _call(hip, size, flat_d, e0d, egd, led, 5, 5)
    assert rc == 0, hip.r3m_last_error()
    for R0 in (0, 2, 4, 6):
        rc, _ = _call(hip, size, flat_d, e0d, egd, led, 5, R0)
        assert rc != 0 and b"R0" in hip.r3m_last_error(), R0
    need = hip.r3m_langrew_infer_workspace_bytes(5, D, H, LD)
    rc, _ = _call(hip, size, flat_d, e0d, egd, led, 5, 5, ws_bytes=need - 1)
    assert rc != 0 and b"workspace" in hip.r3m_last_error()
    for bad in ((48, 64, 32), (64, 96, 32), (64, 64, 48), (0, 64, 32)):
        assert hip.r3m_langrew_infer_workspace_bytes(5, *bad) == 0 and b"langrew" in hip.r3m_last_error(), bad
        ws = torch.zeros(1 << 16, device=DEV)
        rc = hip.r3m_langrew_infer(e0d.data_ptr(), egd.data_ptr(), led.data_ptr(), flat_d.data_ptr(), ws.data_ptr(), ws.data_ptr(),
                                   1 << 18, 5, 5, *bad, _st())
        assert rc != 0 and b"langrew" in hip.r3m_last_error(), bad
    assert hip.r3m_langrew_infer_workspace_bytes(0, D, H, LD) == 0
    torch.cuda.synchronize()
