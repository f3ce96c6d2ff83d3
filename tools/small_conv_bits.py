#!/usr/bin/env python
"""Bit record of the small-M split-K convolution entries (GPU only): one SHA-256 per case over what r3m_conv2d_fwd_affine_small writes
(every case, flag set and split of tests/small_conv_cases.py), the ten integers of r3m_debug_conv_small_plan for the same cases, and the
embedding and feature maps of r3m_resnet_forward_prepared (InferenceSession, split-K kernel on) for ResNet-18 / -50 at 1 and 8 frames, all
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

from oracle import detgen
from r3m_amd.encoder import HipResNet

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
