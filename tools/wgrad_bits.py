#!/usr/bin/env python
"""Bit record of the weight gradients behind the stem (GPU only): one SHA-256 line per case and precision over the dW that the library named
by R3M_HIP_LIB writes through r3m_conv2d_wgrad_dt -- into a NaN-prefilled tensor (and workspace) with accumulate = 0, then onto that result
with accumulate = 1. Two builds compute the same bits iff their listings are equal:
  R3M_HIP_LIB=r3m_amd/lib/libr3m_hip_base.so python tools/wgrad_bits.py > base.txt;  python tools/wgrad_bits.py > new.txt;  diff base.txt new.txt
Cases: every weight gradient of the GPU operator lists (tests/route_sig.py wgrad_operator_cases: all routes and template variants of
csrc/wgrad.hip wgrad_plan, pinned by tests/test_dispatch.py), the edge shapes below, and the six shapes of tools/wgrad_win_check.py."""
import hashlib
import os
import sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import route_sig
from r3m_amd import _lib

# (N, Hi, Wi, Ci, Co, k, stride, pad), dtypes: kernel rows off the window kernel (stride 2; Co off the 64 grid), gathered and simple per-tap
# rows on both tiles, the bf16 per-tap K steps and kernel rows at stride 2, several splits with a short last one (M = 2331)
EDGES = [((3, 9, 7, 128, 128, 3, 2, 1), (0, 1)), ((3, 9, 7, 64, 64, 3, 2, 1), (0, 1)), ((2, 9, 7, 64, 68, 3, 1, 1), (0,)),
         ((3, 9, 7, 64, 128, 1, 2, 0), (0, 1)), ((2, 9, 7, 128, 128, 1, 1, 0), (0, 1)), ((2, 9, 7, 64, 100, 1, 1, 0), (0,)),
         ((2, 9, 7, 64, 128, 1, 1, 0), (0, 1)), ((37, 9, 7, 64, 64, 3, 1, 1), (0, 1))]
WIN_CHECK = [(37, 28, 128, 128), (70, 14, 256, 256), (130, 7, 512, 512), (9, 56, 64, 64), (5, 9, 64, 128), (3, 13, 128, 64)]

L = _lib.lib()
st = torch.cuda.current_stream().cuda_stream
cases = [(c, dt) for (_, c, dt) in route_sig.wgrad_operator_cases()] + [(c, dt) for (c, dts) in EDGES for dt in dts]
cases += [((N, H, H, Ci, Co, 3, 1, 1), dt) for (N, H, Ci, Co) in WIN_CHECK for dt in (0, 1)]
for (case, dt) in dict.fromkeys(cases):
    N, Hi, Wi, Ci, Co, k, s, p = case
    Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
    g = torch.Generator(device="cuda").manual_seed(7)
    tdt = torch.bfloat16 if dt else torch.float32
    x = torch.randn((N, Hi, Wi, Ci), device="cuda", generator=g).to(tdt)
    dy = torch.randn((N, Ho, Wo, Co), device="cuda", generator=g).to(tdt)
    dw = torch.full((Co, k, k, Ci), float("nan"), device="cuda")
    wsb = L.r3m_conv2d_wgrad_workspace_bytes_dt(*case, dt)
    ws = torch.full((max(wsb, 16) // 4,), float("nan"), device="cuda")
    sha = []
    for acc in (0, 1):
        assert L.r3m_conv2d_wgrad_dt(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb, *case, acc, dt, st) == 0, L.r3m_last_error()
        torch.cuda.synchronize()
        sha.append(hashlib.sha256(dw.cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32])
    print(f"{' '.join(map(str, case))} {'bf16' if dt else 'fp32'} ws={wsb} {sha[0]} {sha[1]}", flush=True)
