#!/usr/bin/env python
"""GPU: per-call latency of the frozen encoder on 1 - 16 frames: the existing no_grad forward() against InferenceSession, in one process.

  latency_bench.py grid [--baseline-only]     ResNet-18 / -50 x fp32 / bf16 x 224 x 224 x F in {1, 2, 4, 8, 16}; per point the two legs
                                              alternate, 5 repeats each of (warm-up, median of 200 calls). A call is timed with stream
                                              events around it, the stream idle before it (request -> result on the device, launch
                                              gaps included). --baseline-only: forward() alone — the leg that also runs against the
                                              parent commit's library (tools/build_ab.sh, R3M_HIP_LIB=...), to show whose baseline it is.
  latency_bench.py launches                   per-launch A/B of every ResNet-18 / -50 convolution (F = 1, 8, 16, up to 8192 rows) that
                                              the split-K kernel accepts: r3m_conv2d_fwd_affine_dt (the kernel the launch runs today)
                                              against r3m_conv2d_fwd_affine_small, and whether the routing rule takes it.
  latency_bench.py loop LEG SIZE PREC F N     N calls of one leg (forward | session) after a warm-up: what rocprofv3 --kernel-trace wraps
  latency_bench.py trace DIR N                launches and copies per call from that run's CSV files

Everything prints to stdout; profiles/small_batch_latency.txt is a run of all of it."""
import csv
import ctypes as C
import glob
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
CALLS, REPEATS, WARMUP = 200, 5, 20


def make(size, prec):
    from r3m_amd import R3M
    torch.manual_seed(1)
    return R3M("cuda", 1e-4, 1024, size=size, langweight=0.0, tcnweight=1.0, precision=prec).to(DEV).eval()


def median_call_us(fn, x, calls=CALLS, warmup=WARMUP):
    for _ in range(warmup):
        fn(x)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        torch.cuda.synchronize()
        a.record()
        fn(x)
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def grid(baseline_only):
    from r3m_amd import _lib
    print(f"# library: {_lib.LIB_PATH}")
    print("# us per call: median of %d calls, %d repeats -> min / median / max of the medians; spread = max - min of forward()'s" % (CALLS, REPEATS))
    print("size prec  F   forward(min med max) spread   session(min med max)   forward/session   verdict")
    for size in (18, 50):
        for prec in ("fp32", "bf16"):
            m = make(size, prec)
            sess = None if baseline_only else m.inference_session()
            for F in (1, 2, 4, 8, 16):
                x = torch.randint(0, 256, (F, 3, 224, 224), device=DEV).float()
                fw, ss = [], []
                with torch.no_grad():
                    for _ in range(REPEATS):
                        fw.append(median_call_us(m, x))
                        if sess is not None:
                            ss.append(median_call_us(sess, x))
                f_med, spread = statistics.median(fw), max(fw) - min(fw)
                line = f"r{size:<3d} {prec}  {F:<3d} {min(fw):8.1f} {f_med:8.1f} {max(fw):8.1f} {spread:7.1f}"
                if ss:
                    s_med = statistics.median(ss)
                    verdict = "faster" if f_med - s_med > spread else ("SLOWER" if s_med - f_med > spread else "within spread")
                    line += f"   {min(ss):8.1f} {s_med:8.1f} {max(ss):8.1f}   {f_med / s_med:6.2f}   {verdict}"
                print(line, flush=True)


def launches():
    from r3m_amd import _lib
    L = _lib.lib()
    st = lambda: torch.cuda.current_stream().cuda_stream
    buf = (C.c_int * 10)()

    def per_launch_us(fn, n=100):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e30
        for _ in range(3):
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b) / n * 1e3)
        return best

    print("# per launch, us (best of 3 x 100 back-to-back launches, flags 128|16): today = r3m_conv2d_fwd_affine_dt, small = "
          "r3m_conv2d_fwd_affine_small (its hipMemsetAsync included)")
    print("net  F   Ci   Co k s  HxW      rows  tile  S grid  rule   today   small  today/small")
    wrong = 0
    for size in (18, 50):
        for F in (1, 8, 16):
            h = L.r3m_resnet_create(size, F)
            seen = set()
            for i in range(1, L.r3m_resnet_num_convs(h)):
                v = [C.c_int() for _ in range(9)]
                L.r3m_resnet_conv_info(h, i, *[C.byref(q) for q in v])
                Ci, Co, k, s, p, Hi, Wi, Ho, Wo = [q.value for q in v]
                key, M = (Ci, Co, k, s, Hi, Wi), F * Ho * Wo
                L.r3m_debug_conv_small_plan(F, Hi, Wi, Ci, Co, k, s, p, 144, buf, 10)
                if key in seen or M > 8192 or not buf[4]:
                    continue
                seen.add(key)
                x = torch.randn(F, Hi, Wi, Ci, device=DEV)
                w = torch.randn(Co, k, k, Ci, device=DEV) * 0.05
                sc, sh = torch.ones(Co, device=DEV), torch.zeros(Co, device=DEV)
                out = torch.empty(F, Ho, Wo, Co, device=DEV)
                args = (x.data_ptr(), w.data_ptr(), out.data_ptr(), sc.data_ptr(), sh.data_ptr(), F, Hi, Wi, Ci, Co, k, s, p, 144)
                t_old = per_launch_us(lambda: _lib.check(L.r3m_conv2d_fwd_affine_dt(*args, 0, st())))
                need = L.r3m_conv2d_small_workspace_bytes(F, Hi, Wi, Ci, Co, k, s, p, 0)
                ws = torch.zeros(max(need, 4) // 4, device=DEV)
                t_new = per_launch_us(lambda: _lib.check(L.r3m_conv2d_fwd_affine_small(*args, 0, ws.data_ptr(), need, st())))
                mark = ""
                if bool(buf[0]) != (t_old > t_new):
                    mark, wrong = "  <- rule and A/B disagree", wrong + 1
                print(f"r{size:<3d} {F:<3d} {Ci:4d} {Co:4d} {k} {s} {Hi:3d}x{Wi:<3d} {M:6d}  {buf[1]:4d} {buf[3]:2d} {buf[4]:4d}  "
                      f"{'take' if buf[0] else 'leave'} {t_old:7.1f} {t_new:7.1f}  {t_old / t_new:6.2f}{mark}", flush=True)
            L.r3m_resnet_destroy(h)
    print(f"# launches where the rule and the A/B disagree: {wrong}")


def loop(leg, size, prec, F, n):
    m = make(size, prec)
    fn = m.inference_session() if leg == "session" else m
    x = torch.randint(0, 256, (F, 3, 224, 224), device=DEV).float()
    with torch.no_grad():
        for _ in range(3):
            fn(x)
        torch.cuda.synchronize()
        for _ in range(n):
            fn(x)
        torch.cuda.synchronize()


def trace(d, n):
    """per call = (rows of the last n calls) / n: the run makes 3 warm-up calls first, so counts are taken from the tail of the trace"""
    def rows(pattern):
        out = []
        for f in glob.glob(os.path.join(d, "**", pattern), recursive=True):
            out += list(csv.DictReader(open(f)))
        return out
    kern = sorted(rows("*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    cop = rows("*memory_copy_trace.csv")
    names = [r["Kernel_Name"] for r in kern]
    per = {}
    # one call's launches: the trace tail splits into n equal runs that end with the average pool
    ends = [i for i, k in enumerate(names) if "avgpool" in k]
    assert len(ends) >= n + 1, (len(ends), n)
    a, b = ends[-2] + 1, ends[-1] + 1
    for k in names[a:b]:
        k = k.split("(")[0].replace("void ", "").replace("r3m::", "")
        per[k] = per.get(k, 0) + 1
    print(f"# {d}: {b - a} kernel activities per call (the last call of the trace), {len(kern)} in the whole trace; memory copies in the "
          f"whole trace: {len(cop)}")
    for k, c in sorted(per.items(), key=lambda kv: -kv[1]):
        print(f"  {c:4d}  {k[:140]}")
    by = {}
    for r in cop:
        key = (r.get("Direction", "?"),)
        by[key] = by.get(key, 0) + 1
    for k, c in by.items():
        print(f"  copies {k[0]}: {c}")
    # what stands in front of each copyBuffer activity
    prev = {}
    for i in range(a, b):
        if "copyBuffer" in names[i]:
            p = names[i - 1].split("(")[0].replace("void ", "").replace("r3m::", "")[:80]
            prev[p] = prev.get(p, 0) + 1
    for p, c in prev.items():
        print(f"  copyBuffer behind {p}: {c}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "grid"
    if mode == "grid":
        grid("--baseline-only" in sys.argv)
    elif mode == "launches":
        launches()
    elif mode == "loop":
        loop(sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5]), int(sys.argv[6]))
    elif mode == "trace":
        trace(sys.argv[2], int(sys.argv[3]))
    else:
        sys.exit(__doc__)
