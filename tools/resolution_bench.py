#!/usr/bin/env python
"""GPU: the ResNet-50 encoder at native resolution — frames/s and pixels/s at 128², 224², 256² and 320², fp32 and bf16:
  train   forward (training = 1) + backward with parameter gradients
  infer   forward under no_grad in eval mode (fused inference, training = 2)
  stem    the stem kernels alone at 224 (forward with BatchNorm partials, weight gradient): general (csrc/stem_gen.hip) vs specialised
usage:
  resolution_bench.py [frames=64] [steps=10]          every config, one line each
Timings are CUDA-event medians over `steps` calls after two warm-up calls."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (128, 224, 256, 320)


def timed(fn, steps):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def encoder(prec, frames, steps):
    import torch
    from r3m_amd.encoder import HipResNet
    torch.manual_seed(1)
    m = HipResNet(50, precision=prec).to("cuda:0")
    for s in SIZES:
        x = torch.randint(0, 256, (frames, 3, s, s), device="cuda:0").float()
        cw = torch.rand(frames, m.outdim, device="cuda:0")

        def train():
            m.train()
            (m(x) * cw).sum().backward()

        def infer():
            m.eval()
            with torch.no_grad():
                m(x)
        for name, fn in (("train", train), ("infer", infer)):
            ms = timed(fn, steps)
            fps = frames / ms * 1e3
            print(f"r50 {prec} {name} {s}x{s} F={frames}: {ms:8.2f} ms  {fps:8.0f} frames/s  {fps * s * s / 1e6:8.1f} Mpixel/s", flush=True)


def stem(prec, frames, steps):
    import torch
    from r3m_amd import _lib
    L = _lib.lib()
    dt = 1 if prec == "bf16" else 0
    tdt = torch.bfloat16 if dt else torch.float32
    s = _lib.stream_ptr(torch.device("cuda:0"))
    x = torch.randint(0, 256, (frames, 3, 224, 224), device="cuda:0").float()
    w = torch.randn(64, 7, 7, 3, device="cuda:0") * 0.1
    y = torch.empty(frames, 112, 112, 64, dtype=tdt, device="cuda:0")
    dy = torch.randn(frames, 112, 112, 64, device="cuda:0").to(tdt)
    st = torch.empty((frames * 12544 + 255) // 256, 2, 64, device="cuda:0")
    dw = torch.empty(64, 7, 7, 3, device="cuda:0")
    xg = torch.empty(L.r3m_stem_gen_image_bytes(frames, 224, 224, dt), dtype=torch.uint8, device="cuda:0")
    wsg = torch.empty(L.r3m_stem_gen_wgrad_ws_bytes(), dtype=torch.uint8, device="cuda:0")
    _lib.check(L.r3m_stem_gen_prep(x.data_ptr(), xg.data_ptr(), frames, 224, 224, dt, s), "prep")
    if dt:
        xs = torch.empty(L.r3m_stem_xn16_bytes(frames), dtype=torch.uint8, device="cuda:0")
        wss = torch.empty(L.r3m_stem_conv_wgrad_bf16_workspace_bytes(), dtype=torch.uint8, device="cuda:0")
        _lib.check(L.r3m_stem_prep_bf16(x.data_ptr(), xs.data_ptr(), frames, s), "prep16")
        spec_f = lambda: _lib.check(L.r3m_stem_conv_fwd_bf16(xs.data_ptr(), w.data_ptr(), y.data_ptr(), st.data_ptr(), frames, s), "f")
        spec_w = lambda: _lib.check(L.r3m_stem_conv_wgrad_bf16(xs.data_ptr(), dy.data_ptr(), dw.data_ptr(), wss.data_ptr(), wss.numel(),
                                                               frames, 0, s), "w")
    else:
        xs = torch.empty(frames, 224, 224, 3, device="cuda:0")
        wss = torch.empty(L.r3m_stem_conv_wgrad_workspace_bytes(), dtype=torch.uint8, device="cuda:0")
        _lib.check(L.r3m_stem_prep(x.data_ptr(), xs.data_ptr(), frames, s), "prep")
        spec_f = lambda: _lib.check(L.r3m_stem_conv_fwd(xs.data_ptr(), w.data_ptr(), y.data_ptr(), st.data_ptr(), frames, s), "f")
        spec_w = lambda: _lib.check(L.r3m_stem_conv_wgrad(xs.data_ptr(), dy.data_ptr(), dw.data_ptr(), wss.data_ptr(), wss.numel(),
                                                          frames, 0, s), "w")
    gen_f = lambda: _lib.check(L.r3m_stem_gen_fwd(xg.data_ptr(), w.data_ptr(), y.data_ptr(), st.data_ptr(), frames, 224, 224, dt, s), "gf")
    gen_w = lambda: _lib.check(L.r3m_stem_gen_wgrad(xg.data_ptr(), dy.data_ptr(), dw.data_ptr(), wsg.data_ptr(), frames, 224, 224, 0, dt,
                                                    s), "gw")
    for name, a, b in (("forward", gen_f, spec_f), ("weight gradient", gen_w, spec_w)):
        tg, ts = timed(a, steps), timed(b, steps)
        print(f"stem {prec} {name} 224x224 F={frames}: general {tg:.3f} ms, specialised {ts:.3f} ms, ratio {tg / ts:.2f}", flush=True)


def main():
    sys.path.insert(0, ROOT)
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    for prec in ("fp32", "bf16"):
        stem(prec, max(frames, 256), steps)
        encoder(prec, frames, steps)


if __name__ == "__main__":
    main()
