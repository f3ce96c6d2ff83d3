#!/usr/bin/env python
"""GPU: the native DistilBERT forward (r3m_amd/text.py, csrc/text.hip) against what LangEncoder runs without it, transformers'
DistilBertModel in eager fp32 torch, on the same GPU in the same process with the same random weights at the distilbert-base sizes
(vocab 30522, 512 positions, dim 768, 6 layers, 12 heads, ffn 3072).
  native   HipDistilBert.features(ids, mask)                                   ids / mask uploaded from the host, as LangEncoder does
  eager    model(ids.to(dev), attention_mask=mask.to(dev)).last_hidden_state.mean(1)     under no_grad, eval mode
Shapes (B, T): 256 sentences of 8 / 16 / 32 tokens (a training batch) and one sentence of 8 tokens (a get_reward call). Masks are
ragged. Timing: device events around `inner` back-to-back calls (as many as fill about 50 ms), `warm` untimed rounds first, the
median (and min / max) of `reps` rounds. The two results are compared before anything is timed. Launches per call: the native count
is the library's own launch list (2 + 8 layers); the eager count is the kernels torch.profiler sees in one call, taken after all
timing ("not measured" where the profiler is unavailable). Without transformers on the machine only the native column is printed.
usage: text_bench.py [out=<file>]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = dict(vocab=30522, max_pos=512, dim=768, n_layers=6, n_heads=12, ffn=3072)
SHAPES = [(256, 8), (256, 16), (256, 32), (1, 8)]
WINDOW_MS = 50.0


def timed(torch, fn, warm=3, reps=11):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        fn()
    e1.record()
    e1.synchronize()
    inner = max(3, min(500, int(WINDOW_MS / max(e0.elapsed_time(e1) / 3, 1e-3))))
    ts = []
    for _ in range(reps):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ts), min(ts), max(ts)


def flops(B, T):
    """algorithmic FLOPs of one forward: the six Linears per layer plus the two attention products"""
    D, F, L = DIMS["dim"], DIMS["ffn"], DIMS["n_layers"]
    return L * (2.0 * B * T * (4 * D * D + 2 * D * F) + 4.0 * B * T * T * D)


def eager_launches(torch, fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return str(n) if n else "not measured"
    except Exception:  # noqa: BLE001
        return "not measured"


def main():
    import torch
    sys.path.insert(0, ROOT)
    from r3m_amd.text import HipDistilBert
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    assert torch.cuda.is_available(), "text_bench.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    try:
        from transformers import DistilBertConfig, DistilBertModel
        hf = DistilBertModel(DistilBertConfig(vocab_size=DIMS["vocab"], dim=DIMS["dim"], n_layers=DIMS["n_layers"], n_heads=DIMS["n_heads"],
                                              hidden_dim=DIMS["ffn"], max_position_embeddings=DIMS["max_pos"])).eval()
        sd = hf.state_dict()
        hf = hf.to(dev)
    except ImportError:
        hf = None
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import text_ref
        sd = text_ref.detgen_state_dict("textbench", **DIMS)
    native = HipDistilBert.from_state_dict(sd, DIMS["n_heads"], dev)
    lines = [f"# tools/text_bench.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}"
             + ("" if hf is None else f"  transformers {__import__('transformers').__version__}"),
             f"# distilbert-base sizes {DIMS}, random weights, fp32; ms = median of 11 rounds of ~{WINDOW_MS:.0f} ms of back-to-back calls "
             "(min .. max), host upload of ids / mask included in both columns",
             "# TFLOP/s = algorithmic FLOPs of the forward / median; ratio = eager ms / native ms (> 1: native is faster)"]
    if hf is None:
        lines.append("# transformers is not installed here: native column only, eager not measured")
    eager_calls = []
    for B, T in SHAPES:
        g = torch.Generator().manual_seed(B * 1000 + T)
        ids = torch.randint(0, DIMS["vocab"], (B, T), generator=g)
        n = torch.randint(1, T + 1, (B,), generator=g)
        n[0] = T
        mask = (torch.arange(T)[None, :] < n[:, None]).long()

        def run_native(ids=ids, mask=mask):
            return native.features(ids, mask)

        def run_eager(ids=ids, mask=mask):
            with torch.no_grad():
                return hf(ids.to(dev), attention_mask=mask.to(dev)).last_hidden_state.mean(1)
        a = run_native()
        row = f"B={B:3d} T={T:2d}  {flops(B, T) / 1e9:7.1f} GFLOP"
        if hf is not None:
            b = run_eager()
            err = float((a - b).abs().max() / b.abs().max())
            assert err < 1e-4, f"native and eager features differ: max error {err:.3e} of the range at B={B} T={T}"
            row += f"  max |native - eager| {err:.1e} of the range"
        tn = timed(torch, run_native)
        row += (f"   native {tn[0]:.3f} ms ({tn[1]:.3f} .. {tn[2]:.3f}) {flops(B, T) / tn[0] / 1e9:6.1f} TFLOP/s, "
                f"{native.launches_per_call} launches")
        if hf is not None:
            te = timed(torch, run_eager)
            row += f"   eager {te[0]:.3f} ms ({te[1]:.3f} .. {te[2]:.3f}) {flops(B, T) / te[0] / 1e9:6.1f} TFLOP/s   ratio {te[0] / tn[0]:.2f}"
            eager_calls.append((B, T, run_eager))
        lines.append(row)
        print(row, flush=True)

    def write():
        if "out" in args:
            os.makedirs(os.path.dirname(os.path.abspath(args["out"])), exist_ok=True)
            with open(args["out"], "w") as f:
                f.write("\n".join(lines) + "\n")
    write()                                   # the timings are on disk before the profiler is started
    if eager_calls:
        lines.append("# eager launches per call (kernels torch.profiler sees in one call): "
                     + ", ".join(f"B={B} T={T}: {eager_launches(torch, fn)}" for B, T, fn in eager_calls))
        print(lines[-1], flush=True)
        write()


if __name__ == "__main__":
    main()
