#!/usr/bin/env python
"""Bit record of every caller of the small-M split-K kernel (GPU only): one SHA-256 per case over what r3m_conv2d_fwd_affine_small writes
(every case, flag set and split of tests/small_conv_cases.py), the ten integers of r3m_debug_conv_small_plan for the same cases, the
same for r3m_linear_fwd_small over tests/linear_small_cases.py, the scores of r3m_langrew_infer at 1, 5 and 17 rows, the hidden state
and features of r3m_text_forward_small for a two-layer model on both sides of the take rule, and the embedding and feature maps of
r3m_resnet_forward_prepared (InferenceSession, split-K kernel on) for ResNet-18 / -50 at 1 and 8 frames, all
with the library named by R3M_HIP_LIB. Two builds compute the same bits iff their listings are equal:
  tools/build_ab.sh HEAD
  R3M_HIP_LIB=r3m_amd/lib/libr3m_hip_base.so python tools/small_conv_bits.py > base.txt;  python tools/small_conv_bits.py > new.txt;  diff base.txt new.txt"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from r3m_amd import _lib
from small_conv_cases import ACCUM, GPU_CASES, conv_small_plan, forced_splits
from util import DEV, _st, nhwc, rnd

L = _lib.lib()


def sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:32]


for case, flag_sets in GPU_CASES:
    N, Hi, Wi, Ci, Co, k, s, p = case
    Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
    xd = nhwc(rnd((N, Ci, Hi, Wi), 1)).to(DEV)
    wd = rnd((Co, Ci, k, k), 2, -0.2, 0.2).permute(0, 2, 3, 1).contiguous().to(DEV)
    sc, sh = rnd((Co,), 21, 0.5, 1.5).to(DEV), rnd((Co,), 22, -0.6, 0.6).to(DEV)
    res = rnd((N, Ho, Wo, Co), 23).to(DEV)
    for fl in flag_sets:
        plan = conv_small_plan(L, case, fl)
        print(f"plan {case} flags {fl} {list(plan.values())}")
        for split in [0] + forced_splits(L, case)[0]:
            need = L.r3m_conv2d_small_workspace_bytes(*case, split)
            ws = torch.full((need // 4,), float("nan"), device=DEV)
            out = res.clone() if fl & ACCUM else torch.full((N, Ho, Wo, Co), float("nan"), device=DEV)
            rc = L.r3m_conv2d_fwd_affine_small(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), sc.data_ptr(), sh.data_ptr(), *case, fl, split,
                                               ws.data_ptr(), need, _st())
            assert rc == 0, _lib.last_error()
            print(f"conv2d_fwd_affine_small {case} flags {fl} split {split} {sha(out)}")

import linear_small_cases as lc

for case, flag_sets in lc.GPU_CASES:
    M, K, N = case
    x, w, _ = lc.operands(case)
    xd, wd = x.to(DEV), w.to(DEV)
    for fl in flag_sets:
        bd = lc.reference(case, fl)[0].to(DEV)
        print(f"plan linear {case} flags {fl} {list(lc.linear_small_plan(L, case, fl).values())}")
        for split in [0] + forced_splits(L, lc.geom(case))[0]:
            need = L.r3m_linear_small_workspace_bytes(M, K, N, split)
            ws = torch.full((need // 4,), float("nan"), device=DEV)
            out = torch.full((M, N), float("nan"), device=DEV)
            rc = L.r3m_linear_fwd_small(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), M, K, N, fl, split, ws.data_ptr(), need, _st())
            assert rc == 0, _lib.last_error()
            print(f"linear_fwd_small {case} flags {fl} split {split} {sha(out)}")

from test_gpu_reward_infer import _setup

size = (512, 1024, 768)
flat, e0, eg, le, _ = _setup(size)
for R in (1, 5, 17):
    need = L.r3m_langrew_infer_workspace_bytes(R, *size)
    ws = torch.full((need // 4,), float("nan"), device=DEV)
    score = torch.full((R,), float("nan"), device=DEV)
    args = [t.contiguous().to(DEV) for t in (e0[:R], eg[:R], le[:R], flat)]
    rc = L.r3m_langrew_infer(*[t.data_ptr() for t in args], score.data_ptr(), ws.data_ptr(), need, R, R, *size, _st())
    assert rc == 0, _lib.last_error()
    print(f"langrew_infer {size} R {R} workspace {need} {sha(score)}")

import text_ref
from oracle import detgen
from r3m_amd.encoder import HipResNet
from r3m_amd.text import HipDistilBert

dims = dict(vocab=64, max_pos=128, dim=256, n_layers=2, n_heads=4, ffn=512)
text = HipDistilBert.from_state_dict(text_ref.detgen_state_dict("deeptext_b", **dims), dims["n_heads"], DEV)
for B, T in ((2, 8), (16, 128)):      # every Linear on the few-row kernel; QKV left to the ordinary one
    taken = [lc.linear_small_plan(L, case, fl)["take"] for case, fl in lc.text_linears(B * T, dims["dim"], dims["ffn"])]
    ids = torch.from_numpy((detgen.unit(f"bits_ids_{B}_{T}", B * T) * dims["vocab"]).astype(np.int64).reshape(B, T))
    hidden, feats = text.hidden_and_pools(ids, torch.from_numpy(text_ref.ragged_mask(B, T, 3)), few_rows=True)
    print(f"text_forward_small {tuple(dims.values())} B={B} T={T} taken {taken} {sha(hidden, feats)}")

for size in (18, 50):
    m = HipResNet(size)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes, "w").items()})
    m = m.to(DEV).eval()
    sess = m.inference_session()
    for F in (1, 8):
        x = torch.from_numpy(detgen.smooth_frames(f"bits{F}", (F, 3, 224, 224), 7)).to(DEV)
        with torch.no_grad():
            h, maps = sess.forward_features(x)
        print(f"resnet_forward_prepared r{size} F={F} {sha(h, *[maps[k] for k in sorted(maps)])}")
