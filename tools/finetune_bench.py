#!/usr/bin/env python
"""GPU: ms per ResNet-50 backward under the trainable masks of the fine-tuning recipes (r3m_resnet_set_trainable), HIP events around
the backward call, one forward, then stage-0 restarts over its saved activations:
  all        everything trainable (the pre-training backward)
  layer4     the stem and layer1-3 frozen
  bn_only    only the BatchNorm affine trainable (full dgrad chain, no wgrad)
  frozen+dx  nothing trainable, the input gradient asked for (grads = NULL)
usage:
  finetune_bench.py [frames=1280] [reps=5]            both precisions, each in a child process under its own `timeout`
  finetune_bench.py run <fp32|bf16> [frames] [reps]   one precision in this process
  R3M_HIP_LIB=<libr3m_hip_base.so of the parent commit (tools/build_ab.sh)> finetune_bench.py ...
                                                      the same rows through another build of the library: a library from before
                                                      the trainable mask runs `all` and `frozen+dx` only (the baseline rows)
Drives the C ABI directly (its own ctypes handle), so any build of the library with the engine's plan entry points will do."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("R3M_HIP_LIB") or os.path.join(ROOT, "r3m_amd", "lib", "libr3m_hip.so")


def _lib():
    L = C.CDLL(LIB)
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.r3m_last_error.restype = C.c_char_p
    L.r3m_resnet_create_dt.restype = vp
    L.r3m_resnet_create_dt.argtypes = [i, i, i]
    L.r3m_resnet_destroy.argtypes = [vp]
    for f in ("r3m_resnet_num_params", "r3m_resnet_num_buffers", "r3m_resnet_arena_bytes"):
        getattr(L, f).restype = ll
        getattr(L, f).argtypes = [vp]
    L.r3m_resnet_num_tensors.argtypes = [vp]
    L.r3m_resnet_out_dim.argtypes = [vp]
    L.r3m_resnet_tensor_info.argtypes = [vp, i, C.c_char_p, i, C.POINTER(i), C.POINTER(ll), C.POINTER(i), C.POINTER(i)]
    L.r3m_resnet_forward.argtypes = [vp] * 6 + [i, vp]
    L.r3m_resnet_backward_ex.argtypes = [vp] * 5 + [i, i, i, vp, i, vp]
    if hasattr(L, "r3m_resnet_set_trainable"):
        L.r3m_resnet_set_trainable.argtypes = [vp, C.c_char_p, i]
    return L


def run(prec, frames, reps):
    import torch
    sys.path.insert(0, ROOT)
    L = _lib()
    dev = "cuda:0"
    h = L.r3m_resnet_create_dt(50, frames, 1 if prec == "bf16" else 0)
    if not h:
        raise SystemExit(L.r3m_last_error().decode())
    name, kind, off, nd, shp = C.create_string_buffer(128), C.c_int(), C.c_longlong(), C.c_int(), (C.c_int * 4)()
    tensors = []
    for t in range(L.r3m_resnet_num_tensors(h)):
        L.r3m_resnet_tensor_info(h, t, name, 128, C.byref(kind), C.byref(off), C.byref(nd), shp)
        tensors.append((name.value.decode(), kind.value, off.value, [shp[k] for k in range(nd.value)]))
    torch.manual_seed(1)
    p = torch.zeros(L.r3m_resnet_num_params(h), device=dev)
    b = torch.zeros(L.r3m_resnet_num_buffers(h), device=dev)
    for n, k, o, shape in tensors:                       # torchvision's init: kaiming fan_out convs, BatchNorm (1, 0), statistics (0, 1)
        cnt = 1
        for d in shape:
            cnt *= d
        if k == 0:
            p[o:o + cnt].normal_(0.0, (2.0 / (shape[0] * shape[2] * shape[3])) ** 0.5)
        elif k == 1:
            p[o:o + cnt] = 1.0
        elif k == 4:
            b[o:o + cnt] = 1.0
    g = torch.zeros_like(p)
    arena = torch.empty(L.r3m_resnet_arena_bytes(h), dtype=torch.uint8, device=dev)
    D = L.r3m_resnet_out_dim(h)
    x = torch.randint(0, 256, (frames, 3, 224, 224), device=dev).float()
    out = torch.empty(frames, D, device=dev)
    dh = torch.rand(frames, D, device=dev)
    dx = torch.empty_like(x)
    s = torch.cuda.current_stream().cuda_stream

    def check(rc):
        if rc:
            raise SystemExit(L.r3m_last_error().decode())

    check(L.r3m_resnet_forward(h, x.data_ptr(), p.data_ptr(), b.data_ptr(), arena.data_ptr(), out.data_ptr(), 1, s))
    masked = hasattr(L, "r3m_resnet_set_trainable")
    cases = [("all", None, True, False), ("layer4", lambda n, k: n.startswith("layer4."), True, False),
             ("bn_only", lambda n, k: k in (1, 2), True, False), ("frozen+dx", None, False, True)]
    for label, pick, grads, want_dx in cases:
        if pick is not None and not masked:
            continue
        if masked:
            m = None if pick is None else bytes(1 if (k <= 2 and pick(n, k)) else 0 for n, k, _, _ in tensors)
            check(L.r3m_resnet_set_trainable(h, m, 0 if m is None else len(m)))

        def backward():
            check(L.r3m_resnet_backward_ex(h, dh.data_ptr(), p.data_ptr(), g.data_ptr() if grads else None, arena.data_ptr(), 0, 4, 0,
                                           dx.data_ptr() if want_dx else None, 0, s))

        for _ in range(2):
            backward()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            backward()
            e.record()
            e.synchronize()
            ms.append(a.elapsed_time(e))
        ms.sort()
        print(f"ResNet-50 {prec} {frames} frames backward {label:9s}: median {ms[len(ms) // 2]:8.2f} ms  (min {ms[0]:.2f} max {ms[-1]:.2f}, "
              f"{reps} reps) lib={os.path.basename(LIB)}", flush=True)
    L.r3m_resnet_destroy(h)


def main():
    a = sys.argv[1:]
    if a and a[0] == "run":
        run(a[1], int(a[2]) if len(a) > 2 else 1280, int(a[3]) if len(a) > 3 else 5)
        return
    frames, reps = (a[0] if a else "1280"), (a[1] if len(a) > 1 else "5")
    for prec in ("fp32", "bf16"):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "run", prec, frames, reps])
        if r.returncode != 0:
            print(f"{prec}: exit status {r.returncode}; stopping", flush=True)
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()
