#!/usr/bin/env python
"""Bit record of the BatchNorm passes (GPU only): one SHA-256 per case and pass over everything the library named by R3M_HIP_LIB writes
through the C ABI, on the case lists and inputs of tests/util.py. Two builds compute the same bits iff their listings are equal:
  R3M_HIP_LIB=r3m_amd/lib/libr3m_hip_base.so python tools/bn_bits.py > base.txt;  python tools/bn_bits.py > new.txt;  diff base.txt new.txt
Forward: z and the mask words, three modes. Backward: dy, dgamma, dbeta for every mask source (recompute, bits, fp32 zmask) with
use_batch_stats 1 and 0. Pair call: dy, dgamma, dbeta of both BatchNorms."""
import hashlib
import os
import sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from r3m_amd import _lib
from util import DEV, bn_case_id, bn_cases, bn_inputs, bn_pair_cases

L = _lib.lib()
st = torch.cuda.current_stream().cuda_stream


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        torch.cuda.synchronize()
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:32]


def ok(rc):
    assert rc == 0, L.r3m_last_error()


def ptr(t):
    return None if t is None else t.data_ptr()


def nan(shape, dt=torch.float32):
    return torch.full(shape, float("nan"), dtype=dt, device=DEV)


def forward(inp, mode, tdt, dti, want_bits):
    rows, C = inp["y"].shape
    y, z, coef = inp["y"].to(DEV).to(tdt), nan((rows, C), tdt), inp["coef"].to(DEV)
    bits = torch.full((rows * C // 32,), 0x2AAAAAAA, dtype=torch.int32, device=DEV) if want_bits else None
    r = inp["r"].to(DEV).to(tdt) if mode == "identity" else None
    y2 = inp["y2"].to(DEV).to(tdt) if mode == "downsample" else None
    c2 = inp["coef2"].to(DEV) if mode == "downsample" else None
    ok(L.r3m_bn_act_fwd_dt(y.data_ptr(), coef.data_ptr(), ptr(r), ptr(y2), ptr(c2), z.data_ptr(), rows, C, 1, ptr(bits), dti, st))
    return z, bits


for (rows, C, dtype, why) in bn_cases():
    tdt, dti = (torch.float32, 0) if dtype == "fp32" else (torch.bfloat16, 1)
    cid, bits_ok = bn_case_id((rows, C, dtype, why)), rows * C % 32 == 0
    for mode in ("plain", "identity", "downsample"):
        inp = bn_inputs(rows, C, dtype, mode)
        z, bits = forward(inp, mode, tdt, dti, bits_ok)
        print(f"{cid} fwd {mode} {sha(z, *([bits] if bits_ok else []))}")
        if mode == "downsample":
            continue
        y, dz, coef = inp["y"].to(DEV).to(tdt), inp["dz"].to(DEV).to(tdt), inp["coef"].to(DEV)
        wsb = L.r3m_bn_workspace_bytes(rows, C)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        sources = (["recompute"] if mode == "plain" else []) + (["bits"] if bits_ok else []) + (["zmask"] if dtype == "fp32" else [])
        for source in sources:
            for ubs in (1, 0):
                dg, db, dy = nan((C,)), nan((C,)), nan((rows, C), tdt)
                ok(L.r3m_bn_bwd_dt(dz.data_ptr(), ptr(z) if source == "zmask" else None, ptr(bits) if source == "bits" else None, y.data_ptr(),
                                   coef.data_ptr(), dg.data_ptr(), db.data_ptr(), dy.data_ptr(), ws.data_ptr(), wsb, rows, C, ubs, 0, dti, st))
                print(f"{cid} bwd {mode} {source} ubs={ubs} {sha(dy, dg, db)}")

for (rows, C, dtype) in bn_pair_cases():
    tdt, dti = (torch.float32, 0) if dtype == "fp32" else (torch.bfloat16, 1)
    inp = bn_inputs(rows, C, dtype, "downsample")
    z, bits = forward(inp, "downsample", tdt, dti, True)
    ya, yb, dz = inp["y"].to(DEV).to(tdt), inp["y2"].to(DEV).to(tdt), inp["dz"].to(DEV).to(tdt)
    wsb = L.r3m_bn_pair_workspace_bytes(rows, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    for ubs in (1, 0):
        c6a, c6b = (torch.cat([inp[k], torch.zeros((2, C))]).to(DEV) for k in ("coef", "coef2"))
        dga, dba, dgb, dbb, dya, dyb = nan((C,)), nan((C,)), nan((C,)), nan((C,)), nan((rows, C), tdt), nan((rows, C), tdt)
        ok(L.r3m_bn_bwd_pair_dt(dz.data_ptr(), bits.data_ptr(), ya.data_ptr(), c6a.data_ptr(), yb.data_ptr(), c6b.data_ptr(), dga.data_ptr(),
                                dba.data_ptr(), dya.data_ptr(), dgb.data_ptr(), dbb.data_ptr(), dyb.data_ptr(), ws.data_ptr(), wsb, rows, C,
                                ubs, 0, dti, st))
        print(f"{rows}x{C}_{dtype} pair ubs={ubs} {sha(dya, dyb, dga, dba, dgb, dbb)}")
