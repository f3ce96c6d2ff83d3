"""gpu: the kernels of csrc/text.hip one by one through their stand-alone entry points, every element against float64 on the same fp32
inputs. Outputs are pre-filled with NaN (an element nobody wrote fails); the ceiling is the project's fp32 store ceiling, 2e-5 of the
output range. Inputs are O(1); attention logits stay within +-8."""
import math

import numpy as np
import pytest
import torch

import text_ref
from util import DEV, _st, rnd

pytestmark = pytest.mark.gpu

CEIL = 2e-5
EPS = 1e-12


def _close(got, ref, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements are not finite"
    err = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))
    print(f"{what}: max error {err:.3e} of the output range")
    assert err < CEIL, f"{what}: max error {err:.3e} of the output range (ceiling {CEIL})"


def _dev(*tensors):
    """device copies, held by the caller for as long as the kernel may read them"""
    return [None if t is None else t.to(DEV) for t in tensors]


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


# ---- LayerNorm, embed ----
@pytest.mark.parametrize("C", [64, 256, 768])
@pytest.mark.parametrize("rows", [1, 3, 255, 256, 257])
def test_layernorm_with_and_without_residual(hip, rows, C):
    x = rnd((rows, C), 1, -2, 2)
    res = rnd((rows, C), 2, -2, 2)
    gamma, beta = rnd((C,), 3, 0.5, 1.5), rnd((C,), 4, -1, 1)
    for r in (None, res):
        y = _nan(rows, C)
        xd, rd, gd, bd = _dev(x, r, gamma, beta)
        rc = hip.r3m_layernorm_fwd(xd.data_ptr(), None if rd is None else rd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), rows,
                                   C, EPS, _st())
        assert rc == 0, hip.r3m_last_error()
        xin = x.double().numpy() + (0 if r is None else r.double().numpy())
        _close(y, text_ref.layernorm(xin, gamma.double().numpy(), beta.double().numpy(), EPS), f"layernorm {rows}x{C} res={r is not None}")


@pytest.mark.parametrize("C", [64, 768])
def test_layernorm_of_a_constant_row(hip, C):
    """variance exactly 0: eps alone keeps 1 / sqrt(var + eps) finite (1e6), and the row comes out as beta. The constant is a dyadic
    fraction, so its fp32 row mean is exact in any summation order; for other constants ANY fp32 LayerNorm (torch's too) multiplies the
    mean's last-bit rounding by that 1e6."""
    x = rnd((5, C), 5, -2, 2)
    x[2] = 0.75
    res = torch.zeros(5, C)
    res[2] = 0.5
    gamma, beta = rnd((C,), 6, 0.5, 1.5), rnd((C,), 7, -1, 1)
    for r in (None, res):
        y = _nan(5, C)
        xd, rd, gd, bd = _dev(x, r, gamma, beta)
        assert hip.r3m_layernorm_fwd(xd.data_ptr(), None if rd is None else rd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), 5, C,
                                     EPS, _st()) == 0, hip.r3m_last_error()
        assert torch.equal(y[2].cpu(), beta)
        xin = x.double().numpy() + (0 if r is None else r.double().numpy())
        _close(y, text_ref.layernorm(xin, gamma.double().numpy(), beta.double().numpy(), EPS), f"layernorm constant row C={C}")


@pytest.mark.parametrize("B,T,C", [(1, 1, 64), (3, 1, 256), (5, 51, 768), (2, 128, 64), (257, 1, 256)])
def test_embed(hip, B, T, C):
    vocab = 37
    word, pos = rnd((vocab, C), 8, -1, 1), rnd((T + 3, C), 9, -1, 1)
    gamma, beta = rnd((C,), 10, 0.5, 1.5), rnd((C,), 11, -1, 1)
    g = torch.Generator().manual_seed(12)
    ids = torch.randint(0, vocab, (B, T), generator=g, dtype=torch.int32)
    ids.view(-1)[0] = vocab - 1
    y = _nan(B, T, C)
    d = _dev(ids, word, pos, gamma, beta)
    assert hip.r3m_text_embed(*(t.data_ptr() for t in d), y.data_ptr(), B, T, C, vocab, EPS, _st()) == 0, hip.r3m_last_error()
    xin = word.double().numpy()[ids.numpy()] + pos.double().numpy()[None, :T]
    _close(y, text_ref.layernorm(xin, gamma.double().numpy(), beta.double().numpy(), EPS), f"embed {B}x{T}x{C}")


def test_embed_clamps_ids_outside_the_table(hip):
    vocab, T, C = 11, 4, 64
    word, pos = rnd((vocab, C), 13, -1, 1), rnd((T, C), 14, -1, 1)
    gamma, beta = rnd((C,), 15, 0.5, 1.5), rnd((C,), 16, -1, 1)
    ids = torch.tensor([[-5, 0, 3, 10], [11, 2 ** 31 - 1, -2 ** 31, 7]], dtype=torch.int32)
    y = _nan(2, T, C)
    d = _dev(ids, word, pos, gamma, beta)
    assert hip.r3m_text_embed(*(t.data_ptr() for t in d), y.data_ptr(), 2, T, C, vocab, EPS, _st()) == 0, hip.r3m_last_error()
    xin = word.double().numpy()[ids.numpy().clip(0, vocab - 1)] + pos.double().numpy()[None]
    _close(y, text_ref.layernorm(xin, gamma.double().numpy(), beta.double().numpy(), EPS), "embed with clamped ids")


# ---- bias + GELU ----
@pytest.mark.parametrize("rows,C", [(1, 4), (1, 1020), (1, 1024), (1, 1028), (3, 340), (257, 4), (7, 3072)])
def test_bias_gelu(hip, rows, C):
    """one block is 256 threads x 4 floats = 1024 elements: sizes below, at and above it, and a last vector alone in its block"""
    x, bias = rnd((rows, C), 17, -5, 5), rnd((C,), 18, -1, 1)
    x.view(-1)[0] = 6.0 - float(bias[0])
    x.view(-1)[-1] = -6.0 - float(bias[-1])
    xd, bd = _dev(x, bias)
    assert hip.r3m_bias_gelu(xd.data_ptr(), bd.data_ptr(), rows, C, _st()) == 0, hip.r3m_last_error()
    _close(xd, text_ref.gelu(x.double().numpy() + bias.double().numpy()), f"bias_gelu {rows}x{C}")


# ---- attention ----
ATTN_SHAPES = [(1, 1, 1, 64), (1, 2, 12, 64), (3, 5, 4, 192), (2, 9, 4, 192), (5, 17, 12, 64), (2, 33, 2, 64), (1, 64, 12, 64),
               (3, 128, 12, 64), (2, 32, 4, 192)]


def _masks(B, T):
    full = np.ones((B, T), dtype=np.int64)
    one = np.zeros((B, T), dtype=np.int64)
    one[:, 0] = 1
    if T > 1:
        one[B - 1, 0], one[B - 1, T - 1] = 0, 1          # the one real token need not be the first
    dead = text_ref.ragged_mask(B, T, 1)
    dead[0] = 0                                          # a sentence without a single real key
    return {"full": full, "ragged": text_ref.ragged_mask(B, T, 0), "one real token": one, "one sentence fully masked": dead}


@pytest.mark.parametrize("B,T,heads,hd", ATTN_SHAPES)
def test_attention(hip, B, T, heads, hd):
    dim = heads * hd
    # |q . k| / sqrt(hd) <= hd * a^2 / sqrt(hd) = 8 with a = sqrt(8 / sqrt(hd))
    a = math.sqrt(8.0 / math.sqrt(hd))
    qkv = rnd((B, T, 3 * dim), 19, -a, a)
    qkv[..., 2 * dim:] = rnd((B, T, dim), 20, -1, 1)
    q, k, v = (qkv[..., i * dim:(i + 1) * dim].double().numpy() for i in range(3))
    qd = qkv.to(DEV)
    for name, mask in _masks(B, T).items():
        out = _nan(B, T, dim)
        md = torch.from_numpy(mask).to(torch.int32).to(DEV)
        assert hip.r3m_attention_fwd(qd.data_ptr(), md.data_ptr(), out.data_ptr(), B, T, heads, hd, _st()) == 0, hip.r3m_last_error()
        ref = text_ref.attention(q, k, v, mask, heads)            # every query row, padded ones too
        _close(out, ref, f"attention {(B, T, heads, hd)} mask: {name}")
        if name == "one sentence fully masked":
            # the finite fill: a row without real keys is the plain average of V over all T keys
            uniform = v[0].mean(0)
            assert np.abs(out[0].cpu().numpy() - uniform[None]).max() < CEIL * np.abs(ref).max()


# ---- pool ----
@pytest.mark.parametrize("B,T,C", [(1, 1, 64), (3, 7, 768), (5, 33, 256), (2, 128, 320)])
def test_pool_both_modes(hip, B, T, C):
    hidden = rnd((B, T, C), 21, -2, 2)
    mask = text_ref.ragged_mask(B, T, 2)
    mask[0] = 0                                          # pool 1: zeros, not 0 / 0
    hd, md = hidden.to(DEV), torch.from_numpy(mask).to(torch.int32).to(DEV)
    for mode in (0, 1):
        feats = _nan(B, C)
        assert hip.r3m_text_pool(hd.data_ptr(), md.data_ptr(), feats.data_ptr(), B, T, C, mode, _st()) == 0, hip.r3m_last_error()
        _close(feats, text_ref.pool(hidden.double().numpy(), mask, mode), f"pool {B}x{T}x{C} mode {mode}")
        if mode == 1:
            assert not feats[0].any()
