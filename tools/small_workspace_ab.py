#!/usr/bin/env python
"""GPU: per-call latency of the few-row kernel's callers with the library named by R3M_HIP_LIB, for A/B legs of two builds
(profiles/small_workspace_latency.txt). A library is loaded once per process, so a leg is one process:

  small_workspace_ab.py leg            measures every point once and prints `LEG {point: median us per call}`: the encoder session
                                       (ResNet-18 / -50 fp32, 1 and 8 frames; tools/latency_bench.py's loop), r3m_langrew_infer (D 512 /
                                       2048, 1 / 4 / 16 rows) and HipDistilBert.features with few_rows on and off at distilbert-base
                                       sizes (tools/reward_bench.py's loop and shapes)
  small_workspace_ab.py report LOG     no GPU: LOG holds lines `LEG base {...}` / `LEG new {...}` in the order the legs ran -> per point
                                       min / median / max of either side, the spread of the base legs and whether the new median lies in it

  tools/build_ab.sh HEAD~
  for i in 1 2 3 4; do
    R3M_HIP_LIB=r3m_amd/lib/libr3m_hip_base.so python tools/small_workspace_ab.py leg | sed -n 's/^LEG /LEG base /p' >> legs.log
    python tools/small_workspace_ab.py leg | sed -n 's/^LEG /LEG new /p' >> legs.log
  done; python tools/small_workspace_ab.py report legs.log"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]


def leg():
    import torch

    import latency_bench as lb
    import reward_bench as rb
    import text_ref
    from r3m_amd import _lib
    from r3m_amd.text import HipDistilBert
    assert torch.cuda.is_available(), "small_workspace_ab.py leg measures on the GPU; there is no CPU path"
    DEV = "cuda:0"
    out = {}
    L = _lib.lib()
    for size in (18, 50):
        m = lb.make(size, "fp32")
        sess = m.inference_session()
        for F in (1, 8):
            torch.manual_seed(F)
            x = torch.randint(0, 256, (F, 3, 224, 224), device=DEV).float()
            with torch.no_grad():
                out[f"session r{size} F={F}"] = lb.median_call_us(sess, x)
        del m, sess
    for D in (512, 2048):
        H, LD = 1024, 768
        n = L.r3m_langrew_num_params(D, H, LD)
        torch.manual_seed(D)
        params = torch.randn((n + 3) // 4 * 4, device=DEV) * 0.02
        for R in (1, 4, 16):
            e0, eg, le = torch.rand(R, D, device=DEV), torch.rand(R, D, device=DEV), torch.randn(R, LD, device=DEV) * 0.3
            score = torch.empty(R, device=DEV)
            need = L.r3m_langrew_infer_workspace_bytes(R, D, H, LD)
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)

            def infer():
                _lib.check(L.r3m_langrew_infer(e0.data_ptr(), eg.data_ptr(), le.data_ptr(), params.data_ptr(), score.data_ptr(), ws.data_ptr(),
                                               need, R, R, D, H, LD, rb.st()))
            out[f"langrew_infer D={D} R={R}"] = rb.median_call_us(infer)
    d = rb.TEXT_DIMS
    torch.manual_seed(0)
    sd = {}
    for name, shape in text_ref.tensor_shapes(d["vocab"], d["max_pos"], d["dim"], d["n_layers"], d["ffn"]):
        sd[name] = 1.0 + 0.1 * torch.randn(shape) if name.endswith("orm.weight") else 0.05 * torch.randn(shape)
    native = HipDistilBert.from_state_dict(sd, d["n_heads"], DEV)
    for B, T in ((1, 8), (4, 16), (16, 16)):
        g = torch.Generator().manual_seed(B * 1000 + T)
        ids = torch.randint(0, d["vocab"], (B, T), generator=g)
        n = torch.randint(1, T + 1, (B,), generator=g)
        n[0] = T
        mask = (torch.arange(T)[None, :] < n[:, None]).long()
        out[f"text few_rows B={B} T={T}"] = rb.median_call_us(lambda: native.features(ids, mask, few_rows=True))
        out[f"text default  B={B} T={T}"] = rb.median_call_us(lambda: native.features(ids, mask))
    torch.cuda.synchronize()
    print("LEG " + json.dumps(out), flush=True)


def report(path):
    legs = {"base": [], "new": []}
    for line in open(path):
        if line.startswith("LEG "):
            _, which, js = line.split(" ", 2)
            legs[which].append(json.loads(js))
    print(f"# us per call; {len(legs['base'])} legs of the parent commit's library and {len(legs['new'])} of this tree's, one process per leg, "
          "alternating parent, new, parent, ...")
    print("# spread = max - min of the parent's own legs; verdict: the new median against the parent's [min, max]")
    print(f"{'point':28s} {'parent min':>10s} {'median':>8s} {'max':>8s} {'spread':>7s}   {'new min':>8s} {'median':>8s} {'max':>8s}   "
          f"{'new - parent':>12s}  verdict")
    bad, rows = 0, []
    for k in legs["base"][0]:
        b, n = [l[k] for l in legs["base"]], [l[k] for l in legs["new"]]
        mb, mn = statistics.median(b), statistics.median(n)
        v = ("inside the parent's spread" if min(b) <= mn <= max(b) else
             "below the parent's fastest leg" if mn < min(b) else "ABOVE the parent's slowest leg")
        bad += mn > max(b)
        print(f"{k:28s} {min(b):10.1f} {mb:8.1f} {max(b):8.1f} {max(b) - min(b):7.1f}   {min(n):8.1f} {mn:8.1f} {max(n):8.1f}   "
              f"{mn - mb:+12.1f}  {v}")
        rows.append((k, b, n))
    print(f"# points whose new median lies above the parent's slowest leg: {bad}")
    print("# the legs, in the order they ran")
    for k, b, n in rows:
        print(f"{k:28s} parent " + " ".join(f"{x:7.1f}" for x in b))
        print(f"{'':28s} new    " + " ".join(f"{x:7.1f}" for x in n))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "leg":
        leg()
    elif len(sys.argv) == 3 and sys.argv[1] == "report":
        report(sys.argv[2])
    else:
        sys.exit(__doc__)
