#!/usr/bin/env python
"""Bit record of the fused optimizer steps (GPU only): one SHA-256 per case over everything each of the six entry points
r3m_{adam,sgd}_step{,_ranges,_groups} of the library named by R3M_HIP_LIB writes (p, m, v or the momentum buffer, whole buffers: what
lies outside the ranges counts too), on the tables of tests/optim_cases.py. Two builds compute the same bits iff their listings are equal:
  R3M_HIP_LIB=r3m_amd/lib/libr3m_hip_base.so python tools/optim_bits.py > base.txt;  python tools/optim_bits.py > new.txt;  diff base.txt new.txt
Whole-buffer calls: SIZES at step 1 and 7. Ranged calls: CASES (their step counts run from 1 to 1000). Grouped calls: CASES with one
(lr, weight decay) pair and with two distinct pairs in turn, decoupled 0 and 1, without and with a clip coefficient. SGD everywhere in
its four configurations."""
import hashlib
import os
import sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from r3m_amd import _lib
from optim_cases import CASES, HYPER, SGD, SIZES, _dd, _ll, _state
from util import DEV, _st

L = _lib.lib()
H = HYPER
SGD_LR = 1e-2
PAIRS = {"one_pair": [(1e-3, 0.0)], "two_pairs": [(1e-3, 1e-2), (1e-4, 0.3)]}          # (lr, weight decay) of range k: PAIRS[..][k % len]
COEF = {"nocoef": None, "coef0.37": torch.tensor([0.37], dtype=torch.float32, device=DEV)}


def sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:32]


def ok(rc):
    assert rc == 0, _lib.last_error()


def ptr(t):
    return None if t is None else t.data_ptr()


def sgd_name(c, wd=True):
    return f"momentum={c['momentum']:g},damp={c['damp']:g},{'wd=%g,' % c['wd'] if wd else ''}nesterov={c['nesterov']}"


for n in SIZES:
    for step in (1, 7):
        p, g, m, v = _state(40, n)
        ok(L.r3m_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, H["lr"], H["b1"], H["b2"], H["eps"], step, H["gs"], _st()))
        print(f"adam_step n={n} step={step} {sha(p, m, v)}")
        for c in SGD:
            p, g, buf, _ = _state(41, n)
            ok(L.r3m_sgd_step(p.data_ptr(), g.data_ptr(), ptr(buf) if c["momentum"] else None, n, SGD_LR, c["momentum"], c["damp"], c["wd"],
                              c["nesterov"], step, H["gs"], _st()))
            print(f"sgd_step n={n} step={step} {sgd_name(c)} {sha(p, buf)}")

for case, ranges in sorted(CASES.items()):
    off, cnt, step = ([r[k] for r in ranges] for k in range(3))
    k = len(ranges)
    p, g, m, v = _state(42)
    ok(L.r3m_adam_step_ranges(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ll(off), _ll(cnt), _ll(step), k, H["lr"], H["b1"],
                              H["b2"], H["eps"], H["gs"], _st()))
    print(f"adam_step_ranges {case} {sha(p, m, v)}")
    for c in SGD:
        p, g, buf, _ = _state(43)
        ok(L.r3m_sgd_step_ranges(p.data_ptr(), g.data_ptr(), ptr(buf) if c["momentum"] else None, _ll(off), _ll(cnt), _ll(step), k, SGD_LR,
                                 c["momentum"], c["damp"], c["wd"], c["nesterov"], H["gs"], _st()))
        print(f"sgd_step_ranges {case} {sgd_name(c)} {sha(p, buf)}")
    for pname, pairs in PAIRS.items():
        lrs, wds = ([pairs[i % len(pairs)][j] for i in range(k)] for j in range(2))
        for cname, coef in COEF.items():
            for decoupled in (0, 1):
                p, g, m, v = _state(44)
                ok(L.r3m_adam_step_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ll(off), _ll(cnt), _ll(step), _dd(lrs),
                                          _dd(wds), k, H["b1"], H["b2"], H["eps"], decoupled, H["gs"], ptr(coef), _st()))
                print(f"adam_step_groups {case} {pname} decoupled={decoupled} {cname} {sha(p, m, v)}")
            for c in SGD:
                p, g, buf, _ = _state(45)
                ok(L.r3m_sgd_step_groups(p.data_ptr(), g.data_ptr(), ptr(buf) if c["momentum"] else None, _ll(off), _ll(cnt), _ll(step),
                                         _dd([10 * lr for lr in lrs]), _dd(wds), k, c["momentum"], c["damp"], c["nesterov"], H["gs"], ptr(coef),
                                         _st()))
                print(f"sgd_step_groups {case} {pname} {cname} {sgd_name(c, False)} {sha(p, buf)}")
