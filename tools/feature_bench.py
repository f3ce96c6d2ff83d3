#!/usr/bin/env python
"""GPU: the two feature-map kernels (csrc/feat.hip) against what a user would write in torch instead, on the same tensors in the
same process, at ResNet-50's four stage outputs for 224 x 224 frames.
  export    r3m_feature_export_dt          vs  z.permute(0, 3, 1, 2).float().contiguous()
  grad_add  r3m_feature_grad_add_dt        vs  g += d.permute(0, 2, 3, 1)          (computed in fp32, rounded once to g's dtype)
Timing: device events around `inner` back-to-back launches (as many as fill about 25 ms), `warm` untimed rounds first, the median
(and min / max) of `reps` rounds. Rows whose bytes fit the 256 MiB Infinity Cache are marked: their rate is a cache rate.
Bytes are what the operation must move: export n * (size(z) + 4), grad_add n * (4 + 2 * size(g)). The results are compared bit for
bit before anything is timed.
usage: feature_bench.py [frames=256] [out=<file>]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = [("layer1", 56, 56, 256), ("layer2", 28, 28, 512), ("layer3", 14, 14, 1024), ("layer4", 7, 7, 2048)]
L3_BYTES = 256 << 20  # Infinity Cache: a call that moves less than this loops inside it, its bytes/s is not an HBM rate
WINDOW_MS = 25.0      # one timed round lasts about this long: `inner` back-to-back launches between two events


def timed(torch, fn, warm=3, reps=15):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        fn()
    e1.record()
    e1.synchronize()
    inner = max(5, min(2000, int(WINDOW_MS / max(e0.elapsed_time(e1) / 5, 1e-3))))
    ts = []
    for _ in range(reps):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ts), min(ts), max(ts)


def main():
    import torch
    sys.path.insert(0, ROOT)
    from r3m_amd import _lib
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    frames = int(args.get("frames", 256))
    assert torch.cuda.is_available(), "feature_bench.py measures on the GPU; there is no CPU path"
    L = _lib.lib()
    dev = torch.device("cuda:0")
    s = _lib.stream_ptr(dev)
    lines = [f"# tools/feature_bench.py frames={frames}  {torch.cuda.get_device_name(0)}",
             "# ms = median of 15 rounds of ~25 ms of back-to-back launches (min .. max); TB/s = required bytes / median; ratio = torch ms / kernel ms",
             "# L3 = the call moves less than the 256 MiB Infinity Cache and is looped: a cache-resident rate, not an HBM rate"]
    worst = None
    for dt, dtype in ((0, torch.float32), (1, torch.bfloat16)):
        for name, H, W, C in MAPS:
            torch.manual_seed(H)
            n = frames * H * W * C
            z = torch.randn(frames, H, W, C, device=dev).to(dtype)
            d = torch.randn(frames, C, H, W, device=dev)
            out = torch.empty(frames, C, H, W, device=dev)
            # same results first
            _lib.check(L.r3m_feature_export_dt(z.data_ptr(), out.data_ptr(), frames, H, W, C, dt, s), "feature_export")
            assert torch.equal(out, z.permute(0, 3, 1, 2).float().contiguous())
            g1, g2 = z.clone(), z.clone()
            _lib.check(L.r3m_feature_grad_add_dt(d.data_ptr(), g1.data_ptr(), frames, H, W, C, dt, s), "feature_grad_add")
            g2 += d.permute(0, 2, 3, 1)
            assert torch.equal(g1, g2)
            del g2
            rows = [
                ("export", n * (z.element_size() + 4),
                 lambda: L.r3m_feature_export_dt(z.data_ptr(), out.data_ptr(), frames, H, W, C, dt, s),
                 lambda: z.permute(0, 3, 1, 2).float().contiguous()),
                ("grad_add", n * (4 + 2 * z.element_size()),
                 lambda: L.r3m_feature_grad_add_dt(d.data_ptr(), g1.data_ptr(), frames, H, W, C, dt, s),
                 lambda: g1.add_(d.permute(0, 2, 3, 1))),
            ]
            for op, nbytes, hip_fn, torch_fn in rows:
                th, tl = timed(torch, hip_fn), timed(torch, torch_fn)
                ratio = tl[0] / th[0]
                if worst is None or ratio < worst[0]:
                    worst = (ratio, op, name, "bf16" if dt else "fp32")
                lines.append(f"{op:8s} {'bf16' if dt else 'fp32'} {name} [{frames},{H},{W},{C}] {nbytes / 1e6:8.1f} MB  "
                             f"kernel {th[0]:.4f} ms ({th[1]:.4f} .. {th[2]:.4f}) {nbytes / th[0] / 1e9:5.2f} TB/s   "
                             f"torch {tl[0]:.4f} ms ({tl[1]:.4f} .. {tl[2]:.4f}) {nbytes / tl[0] / 1e9:5.2f} TB/s   ratio {ratio:.2f}"
                             + ("   L3" if nbytes < L3_BYTES else ""))
                print(lines[-1], flush=True)
            del z, d, out, g1
            torch.cuda.empty_cache()
    lines.append(f"# smallest torch / kernel ratio: {worst[0]:.2f} ({worst[1]} {worst[3]} {worst[2]}); the kernels must be no slower "
                 f"than torch on every row (ratio >= 1)")
    print(lines[-1], flush=True)
    if "out" in args:
        os.makedirs(os.path.dirname(os.path.abspath(args["out"])), exist_ok=True)
        with open(args["out"], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if worst[0] >= 1.0 else 3)


if __name__ == "__main__":
    main()
