#!/usr/bin/env python
"""GPU: what parameter groups, weight decay and gradient clipping cost on ResNet-50's flat buffers (23.5 M fp32 elements), HIP events
around the calls, median of `reps` after a warm-up:
  adam_step             r3m_adam_step over the whole buffer (the plain optimizer step)
  adam_step_ranges      r3m_adam_step_ranges over the plan of FusedAdam with layer1 frozen (partial-freeze fine-tuning)
  sgd_step              r3m_sgd_step over the whole buffer with momentum 0.9
  ... (baseline)        the same three calls through another build of the library (R3M_HIP_LIB_BASE=<libr3m_hip_base.so of the parent
                        commit, tools/build_ab.sh>), on the same buffers. The baseline adam_step is timed twice, first and last in the
                        run: the difference between its two readings is the run's own spread
  adam_step_groups      r3m_adam_step_groups over the ranges FusedAdamW._plan gives for the no_decay_groups split (decoupled decay on the
                        convolution weights, none on BatchNorm), without and with a clip coefficient
  grad_sqnorm           r3m_grad_sqnorm_ranges over the same ranges, and over those ranges with neighbours coalesced, which is what
                        step() passes (one range when every tensor has a gradient); + r3m_clip_coef
  plain read            torch.sum over the gradient buffer: a read of the same bytes with an fp32 reduction
usage: optim_bench.py [reps=30]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from r3m_amd import _lib
    from r3m_amd.encoder import HipResNet
    from r3m_amd.optim import FusedAdam, FusedAdamW, _coalesce, _dd, _ll, no_decay_groups
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    dev = torch.device("cuda:0")
    L = _lib.lib()
    net = HipResNet(50).to(dev)
    p, g = net.flat_params(), net.flat_grads()
    g.normal_(0.0, 1e-3)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    n = p.numel()
    opt = FusedAdamW([net], lr=1e-4, param_groups=no_decay_groups(net, 0.05))
    net._grads.mark_all_written()                                # as after a backward with everything trainable
    plan = opt._plan(0, net)
    launches = (len(plan.offs) + 63) // 64
    print(f"ResNet-50: {n} elements, {len(net.param_ranges())} tensors; no_decay_groups -> {len(plan.offs)} merged ranges, "
          f"{launches} launch(es) per grouped step, {2 * launches} per norm; distinct (lr, wd): {sorted(set(zip(plan.lrs, plan.wds)))}")
    st = _lib.stream_ptr(dev)
    ws = torch.empty(int(L.r3m_grad_sqnorm_workspace_bytes()), dtype=torch.uint8, device=dev)
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    coef = torch.ones(2, device=dev)
    offs, counts, steps, lrs, wds = _ll(plan.offs), _ll(plan.counts), _ll(plan.steps), _dd(plan.lrs), _dd(plan.wds)
    k = len(plan.offs)
    co, cc = _coalesce(plan.offs, plan.counts)                   # what FusedAdam.step() hands the norm: neighbours as one range
    ptrs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())

    layer1 = {(q.data_ptr() - p.data_ptr()) // 4 for name, q in net.named_parameters() if name.startswith("layer1.")}
    net._grads.written = [off not in layer1 for off, _ in net.param_ranges()]         # as after a backward with layer1 frozen
    fplan = FusedAdam([net], lr=1e-4)._plan(0, net)
    print(f"layer1 frozen -> {len(fplan.offs)} ranges of {fplan.counts} elements at steps {fplan.steps}")
    foffs, fcounts, fsteps, fk = _ll(fplan.offs), _ll(fplan.counts), _ll([2] * len(fplan.offs)), len(fplan.offs)
    trained = sum(fplan.counts)

    def adam_with(lib):
        return lambda: _lib.check(lib.r3m_adam_step(*ptrs, n, 1e-4, 0.9, 0.999, 1e-8, 2, 1.0, st), "adam_step")

    def ranges_with(lib):
        return lambda: _lib.check(lib.r3m_adam_step_ranges(*ptrs, foffs, fcounts, fsteps, fk, 1e-4, 0.9, 0.999, 1e-8, 1.0, st), "adam_step_ranges")

    def sgd_with(lib):
        return lambda: _lib.check(lib.r3m_sgd_step(*ptrs[:3], n, 1e-4, 0.9, 0.0, 0.0, 0, 2, 1.0, st), "sgd_step")

    def groups(c):
        return lambda: _lib.check(L.r3m_adam_step_groups(*ptrs, offs, counts, steps, lrs, wds, k, 0.9, 0.999, 1e-8, 1, 1.0, c, st), "groups")

    def sqnorm(o, c, kk):
        return lambda: _lib.check(L.r3m_grad_sqnorm_ranges(g.data_ptr(), o, c, kk, acc.data_ptr(), 0, ws.data_ptr(), ws.numel(), st), "sqnorm")

    base = os.environ.get("R3M_HIP_LIB_BASE")
    pairs = [("adam_step", adam_with, 7 * 4 * n), (f"adam_step_ranges, layer1 frozen ({fk} ranges)", ranges_with, 7 * 4 * trained),
             ("sgd_step, momentum", sgd_with, 5 * 4 * n)]
    rows, last = [], []
    if base:
        B = C.CDLL(base)
        for name in ("r3m_adam_step", "r3m_adam_step_ranges", "r3m_sgd_step"):
            getattr(B, name).restype, getattr(B, name).argtypes = _lib.SIGNATURES[name]
        tag = f"(baseline {os.path.basename(base)})"
        rows.append((f"adam_step {tag}, first", adam_with(B), 7 * 4 * n))
        last.append((f"adam_step {tag}, last", adam_with(B), 7 * 4 * n))
    for name, make, nbytes in pairs:
        rows.append((name, make(L), nbytes))
        if base and make is not adam_with:
            rows.append((f"{name} {tag}", make(B), nbytes))
    rows += [("adam_step_groups, no coefficient", groups(None), 7 * 4 * n),
             ("adam_step_groups, clip coefficient", groups(coef.data_ptr()), 7 * 4 * n),
             (f"grad_sqnorm over the {k} ranges", sqnorm(offs, counts, k), 4 * n),
             (f"grad_sqnorm over the {len(co)} coalesced range(s) (step())", sqnorm(_ll(co), _ll(cc), len(co)), 4 * n),
             ("clip_coef", lambda: _lib.check(L.r3m_clip_coef(acc.data_ptr(), 1.0, 1.0, coef.data_ptr(), st), "clip_coef"), 0),
             ("plain read: torch.sum(grads)", lambda: g.sum(), 4 * n)] + last
    for name, fn, nbytes in rows:
        for _ in range(5):
            fn()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        med = statistics.median(times)
        bw = f"{nbytes / med / 1e6:8.0f} GB/s" if nbytes else " " * 13
        print(f"{name:60s} median {med * 1e3:8.1f} us  min {min(times) * 1e3:8.1f} us  {bw}", flush=True)
    print(f"sqnorm = {float(acc):.6e} (torch float64: {float((g.double() ** 2).sum()):.6e})")


if __name__ == "__main__":
    main()
