"""Shared by tests/test_linear_small_plan.py (no GPU) and tests/test_gpu_linear_small.py: the case list of the few-row Linear
(r3m_linear_fwd_small: the split-K kernel of csrc/conv_small.hip on the 1 x 1 geometry (M, 1, 1, K, N, 1, 1, 0) with a Linear store), its
operands and float64 references, and the Linear shapes of the reward head and of distilbert-base whose routing is pinned.
The plan queries go through r3m_debug_linear_small_plan / r3m_debug_conv_small_plan: host-only, nothing is launched."""
import ctypes as C
import functools

import torch

from util import rnd

BIAS, RELU, GELU = 8, 16, 256
B, BR, BG = BIAS, BIAS | RELU, BIAS | GELU
LINEAR_FLAGS = (B, BR, BG)
PLAN_FIELDS = ("take", "bm", "bn", "S", "grid", "cps", "tiles_m", "tiles_n", "nch", "max_split")

# (M, K, N) -> the flag sets run on it
GPU_CASES = [
    ((1, 4864, 1024), (BR,)),        # head layer 0 of ResNet-50; one live row in a 16-row tile
    ((1, 1024, 1024), (BR,)),
    ((5, 1792, 64), (BR,)),          # ResNet-18 K1; one column tile
    ((16, 768, 2304), (B,)),         # a full 16-row tile
    ((17, 768, 768), (B,)),          # the 32-row tile with 15 dead rows
    ((33, 768, 3072), (BG,)),        # the 64-row tile, ragged
    ((8, 3072, 768), (B,)),          # lin2's K
    ((65, 256, 512), (BG,)),         # two row tiles, the second holds one row
    ((130, 512, 256), (B,)),         # three row tiles
    ((3, 32, 64), (B, BR, BG)),      # one chunk: S = 1 only
    ((2, 160, 64), (BR,)),           # five chunks: a ragged last slice
]


def geom(case):
    """the 1 x 1 convolution geometry of a Linear (M, K, N)"""
    M, K, N = case
    return (M, 1, 1, K, N, 1, 1, 0)


def linear_small_plan(L, case, flags):
    buf = (C.c_int * 10)()
    assert L.r3m_debug_linear_small_plan(*case, flags, buf, 10) == 10, L.r3m_last_error()
    return dict(zip(PLAN_FIELDS, list(buf)))


@functools.lru_cache(maxsize=None)
def operands(case):
    """x [M,K], w [N,K] (CPU, fp32) and the float64 product, generated as tests/test_gpu_small_conv.py generates a convolution's: once
    per case, shared by its flag sets, never written"""
    M, K, N = case
    x = rnd((M, K), 1)
    w = rnd((N, K), 2, -0.2, 0.2)
    return x, w, x.double() @ w.double().t()


def reference(case, flags):
    """(bias fp32 [N], pre-activation float64, float64 reference, its summands): the bias is +-0.6 of the product's rms"""
    _, _, y = operands(case)
    sd = float(y.pow(2).mean().sqrt())
    bias = rnd((case[2],), 22, -0.6, 0.6) * sd
    terms = [y, bias.double().view(1, -1).expand_as(y)]
    pre = terms[0] + terms[1]
    if flags & GELU:
        ref = 0.5 * pre * (1.0 + torch.erf(pre / 2.0 ** 0.5))
    elif flags & RELU:
        ref = torch.relu(pre)
    else:
        ref = pre
    return bias, pre, ref, terms


def head_linears(R, D, hidden=1024, lang_dim=768):
    """the four hidden Linears of LanguageReward over R rows, all with bias + ReLU"""
    return [((R, 2 * D + lang_dim, hidden), BR)] + [((R, hidden, hidden), BR)] * 3


def text_linears(R, dim=768, ffn=3072):
    """QKV, the output Linear, lin1 (bias + GELU) and lin2 of one distilbert-base layer over R = B * T rows"""
    return [((R, dim, 3 * dim), B), ((R, dim, dim), B), ((R, dim, ffn), BG), ((R, ffn, dim), B)]
