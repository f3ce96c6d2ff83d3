#!/usr/bin/env python
"""GPU: forward + input-gradient backward (obs.grad) of the ResNet-50 encoder, eval mode, two cases:
  frozen     parameters requires_grad_(False): no weight-gradient launch (r3m_resnet_backward_ex with grads = NULL)
  trainable  parameters trainable and obs.requires_grad: weight gradients are written as well (the side effect INTEGRATION.md names)
usage:
  input_grad_bench.py                                   all four (fp32 | bf16) x (frozen | trainable) configs, each in a child process
                                                        under its own `timeout`, one line each
  input_grad_bench.py run <fp32|bf16> <frozen|trainable> [frames=256] [steps=10]
                                                        one config in this process (what rocprofv3 --kernel-trace wraps)"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(prec, case, frames, steps):
    import torch
    sys.path.insert(0, ROOT)
    from r3m_amd.encoder import HipResNet
    torch.manual_seed(1)
    m = HipResNet(50, precision=prec).to("cuda:0").eval()
    if case == "frozen":
        for p in m.parameters():
            p.requires_grad_(False)
    elif case != "trainable":
        raise SystemExit(f"case {case!r}: frozen or trainable")
    x = torch.randint(0, 256, (frames, 3, 224, 224), device="cuda:0").float()
    cw = torch.rand(frames, m.outdim, device="cuda:0")

    def step():
        xg = x.requires_grad_(True)
        (m(xg) * cw).sum().backward()
        xg.grad = None

    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    print(f"ResNet-50 {prec} eval {case:9s} {frames} frames: forward + obs.grad backward {ms:.2f} ms per step", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        a = sys.argv[2:]
        run(a[0], a[1], int(a[2]) if len(a) > 2 else 256, int(a[3]) if len(a) > 3 else 10)
        return
    for prec in ("fp32", "bf16"):
        for case in ("frozen", "trainable"):
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "run", prec, case])
            if r.returncode != 0:
                print(f"{prec} {case}: exit status {r.returncode}; stopping", flush=True)
                sys.exit(r.returncode)


if __name__ == "__main__":
    main()
