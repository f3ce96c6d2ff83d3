#!/usr/bin/env python
"""GPU: what the few-row Linear (r3m_linear_fwd_small, csrc/conv_small.hip) buys the language reward and the text model. Four legs; the
alternatives of a leg alternate in ONE process; a call is timed with stream events around it, the stream idle before it, as
tools/latency_bench.py times a call: per point REPEATS repeats of (warm-up, median of CALLS calls) -> min / median / max of the medians.
The spread of a baseline is max - min of its repeat medians; a verdict is "faster" / "SLOWER" only beyond that spread.

  reward_bench.py launches      per launch: r3m_linear_fwd (+ r3m_bias_gelu for lin1: today's launches) against r3m_linear_fwd_small
                                (its hipMemsetAsync included) for every Linear shape of the head (D 512 and 2048, rows 1, 4, 16) and of
                                distilbert-base (rows 8, 64, 256, 512, 4096), with the plan and whether the rule takes it
  reward_bench.py calls         per call: r3m_langrew_call_forward against r3m_langrew_infer (D 512 / 2048, hidden 1024, rows 1, 4, 16)
  reward_bench.py steps [--baseline-only]
                                per control step, ResNet-18 / -50 fp32, rows 1, 4, 16: get_reward(e0, model(frame), feats) under
                                no_grad against RewardSession.step. --baseline-only: the first leg alone, the one that also runs
                                against the parent commit's library (tools/build_ab.sh, R3M_HIP_LIB=...)
  reward_bench.py text          HipDistilBert.features at (B, T) = (1, 8), (4, 16), (16, 16), (256, 16) with few_rows off and on, and
                                transformers' eager DistilBertModel where it is importable (distilbert-base sizes, random weights)
  reward_bench.py all           the four legs

Everything prints to stdout; profiles/reward_latency.txt is a run of all of it."""
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
DEV = "cuda:0"
CALLS, REPEATS, WARMUP = 100, 5, 10
BIAS, RELU, GELU = 8, 16, 256
TEXT_DIMS = dict(vocab=30522, max_pos=512, dim=768, n_layers=6, n_heads=12, ffn=3072)


def median_call_us(fn, calls=CALLS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def alternate(legs):
    """legs: [fn]; -> per leg the list of REPEATS medians, the legs taking turns"""
    out = [[] for _ in legs]
    for _ in range(REPEATS):
        for i, fn in enumerate(legs):
            out[i].append(median_call_us(fn))
    return out


def stats(v):
    return f"{min(v):8.1f} {statistics.median(v):8.1f} {max(v):8.1f}"


def verdict(base, new):
    spread = max(base) - min(base)
    b, n = statistics.median(base), statistics.median(new)
    return spread, b / n, "faster" if b - n > spread else ("SLOWER" if n - b > spread else "within spread")


def st():
    return torch.cuda.current_stream().cuda_stream


def launches():
    from r3m_amd import _lib
    L = _lib.lib()
    buf = (C.c_int * 10)()
    shapes = []
    for D in (512, 2048):
        for R in (1, 4, 16):
            shapes += [(f"head D={D} layer 0", R, 2 * D + 768, 1024, BIAS | RELU)]
    shapes += [("head layers 1-3", R, 1024, 1024, BIAS | RELU) for R in (1, 4, 16)]
    for R in (8, 64, 256, 512, 4096):
        shapes += [("text QKV", R, 768, 2304, BIAS), ("text out", R, 768, 768, BIAS), ("text lin1", R, 768, 3072, BIAS | GELU),
                   ("text lin2", R, 3072, 768, BIAS)]
    print("# per launch, us: today = r3m_linear_fwd (lin1: without bias, + r3m_bias_gelu), small = r3m_linear_fwd_small (its memset included)")
    print("# min med max of %d repeat medians of %d calls each; spread = max - min of today's" % (REPEATS, CALLS))
    print("what                  rows     K     N flags tile  S grid rule    today(min med max)  spread    small(min med max)  today/small  verdict")
    slower = 0
    for what, M, K, N, fl in shapes:
        x = torch.randn(M, K, device=DEV)
        w = torch.randn(N, K, device=DEV) * 0.05
        b = torch.randn(N, device=DEV)
        y = torch.empty(M, N, device=DEV)
        L.r3m_debug_linear_small_plan(M, K, N, fl, buf, 10)
        need = L.r3m_linear_small_workspace_bytes(M, K, N, 0)
        ws = torch.zeros(max(need, 4) // 4, device=DEV)
        if fl & GELU:
            def today():
                _lib.check(L.r3m_linear_fwd(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), M, K, N, 0, st()))
                _lib.check(L.r3m_bias_gelu(y.data_ptr(), b.data_ptr(), M, N, st()))
        else:
            def today():
                _lib.check(L.r3m_linear_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, 1 if fl & RELU else 0, st()))

        def small():
            _lib.check(L.r3m_linear_fwd_small(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, fl, 0, ws.data_ptr(), need, st()))
        t, s = alternate([today, small])
        spread, ratio, v = verdict(t, s)
        mark = ""
        if buf[0] and v == "SLOWER":
            mark, slower = "  <- taken and slower than the spread", slower + 1
        print(f"{what:20s} {M:5d} {K:5d} {N:5d} {fl:5d} {buf[1]:4d} {buf[3]:2d} {buf[4]:4d} {'take ' if buf[0] else 'leave'} {stats(t)} {spread:7.1f} "
              f"{stats(s)}   {ratio:6.2f}  {v}{mark}", flush=True)
    print(f"# launches the rule takes that are slower than today's kernel by more than the spread: {slower}")


def calls():
    from r3m_amd import _lib
    L = _lib.lib()
    print("# per call, us: call_forward = r3m_langrew_call_forward (what LanguageReward.forward runs), infer = r3m_langrew_infer; hidden 1024, lang_dim 768")
    print("   D rows   call_forward(min med max)  spread      infer(min med max)   call/infer  verdict")
    for D in (512, 2048):
        H, LD = 1024, 768
        n = L.r3m_langrew_num_params(D, H, LD)
        params = torch.randn((n + 3) // 4 * 4, device=DEV) * 0.02
        for R in (1, 4, 16):
            e0, eg, le = torch.rand(R, D, device=DEV), torch.rand(R, D, device=DEV), torch.randn(R, LD, device=DEV) * 0.3
            s1, s2 = torch.empty(R, device=DEV), torch.empty(R, device=DEV)
            n1, n2 = L.r3m_langrew_call_workspace_bytes(R, D, H, LD), L.r3m_langrew_infer_workspace_bytes(R, D, H, LD)
            w1, w2 = torch.empty(n1, dtype=torch.uint8, device=DEV), torch.empty(n2, dtype=torch.uint8, device=DEV)

            def old():
                _lib.check(L.r3m_langrew_call_forward(e0.data_ptr(), eg.data_ptr(), le.data_ptr(), params.data_ptr(), s1.data_ptr(), w1.data_ptr(),
                                                      n1, R, D, H, LD, st()))

            def new():
                _lib.check(L.r3m_langrew_infer(e0.data_ptr(), eg.data_ptr(), le.data_ptr(), params.data_ptr(), s2.data_ptr(), w2.data_ptr(), n2,
                                               R, R, D, H, LD, st()))
            t, s = alternate([old, new])
            torch.cuda.synchronize()
            err = float((s1 - s2).abs().max() / s1.abs().max())
            spread, ratio, v = verdict(t, s)
            print(f"{D:4d} {R:4d}   {stats(t)} {spread:7.1f}   {stats(s)}   {ratio:6.2f}  {v}   (scores differ by {err:.1e} of the range)", flush=True)


def steps(baseline_only):
    from r3m_amd import R3M, _lib
    print(f"# library: {os.path.relpath(_lib.LIB_PATH, ROOT)}")
    print("# per control step, us, fp32, 224 x 224: get_reward = model.get_reward(e0, model(frames), feats) under no_grad; step = RewardSession.step")
    print("size rows    get_reward(min med max)  spread       step(min med max)   get_reward/step  verdict")
    for size in (18, 50):
        torch.manual_seed(1)
        m = R3M("cuda", 1e-4, 1024, size=size, langweight=1.0).to(DEV).eval()
        rs = None if baseline_only else m.reward_session()
        for R in (1, 4, 16):
            first = torch.randint(0, 256, (1, 3, 224, 224), device=DEV).float()
            frames = torch.randint(0, 256, (R, 3, 224, 224), device=DEV).float()
            feats = torch.randn(1, 768, device=DEV) * 0.3
            with torch.no_grad():
                e0 = m(first).expand(R, -1).contiguous()
                fR = feats.expand(R, -1).contiguous()

                def old():
                    return m.get_reward(e0, m(frames), fR)
                legs = [old]
                if rs is not None:
                    rs.reset(first, feats)
                    legs.append(lambda: rs.step(frames))
                got = alternate(legs)
            line = f"r{size:<3d} {R:4d}   {stats(got[0])} {max(got[0]) - min(got[0]):7.1f}"
            if rs is not None:
                _, ratio, v = verdict(got[0], got[1])
                line += f"   {stats(got[1])}   {ratio:6.2f}  {v}"
            print(line, flush=True)


def text():
    import text_ref
    from r3m_amd.text import HipDistilBert
    d = TEXT_DIMS
    torch.manual_seed(0)
    try:
        from transformers import DistilBertConfig, DistilBertModel
        hf = DistilBertModel(DistilBertConfig(vocab_size=d["vocab"], dim=d["dim"], n_layers=d["n_layers"], n_heads=d["n_heads"],
                                              hidden_dim=d["ffn"], max_position_embeddings=d["max_pos"])).eval()
        sd = hf.state_dict()
        hf = hf.to(DEV)
    except ImportError:
        hf = None
        sd = {}
        for name, shape in text_ref.tensor_shapes(d["vocab"], d["max_pos"], d["dim"], d["n_layers"], d["ffn"]):
            sd[name] = 1.0 + 0.1 * torch.randn(shape) if name.endswith("orm.weight") else 0.05 * torch.randn(shape)
    native = HipDistilBert.from_state_dict(sd, d["n_heads"], DEV)
    print("# per call, us, distilbert-base sizes, random weights, fp32, the host upload of ids / mask included in every column")
    print("# native = HipDistilBert.features, few_rows = the same with few_rows=True, eager = transformers' DistilBertModel + mean(1) under no_grad"
          + ("" if hf is not None else " (transformers is not importable here: not measured)"))
    print("   B   T     native(min med max)  spread    few_rows(min med max)  native/few_rows  verdict" + ("        eager(min med max)  eager/few_rows" if hf else ""))
    for B, T in ((1, 8), (4, 16), (16, 16), (256, 16)):
        g = torch.Generator().manual_seed(B * 1000 + T)
        ids = torch.randint(0, d["vocab"], (B, T), generator=g)
        n = torch.randint(1, T + 1, (B,), generator=g)
        n[0] = T
        mask = (torch.arange(T)[None, :] < n[:, None]).long()
        legs = [lambda: native.features(ids, mask), lambda: native.features(ids, mask, few_rows=True)]
        if hf is not None:
            def eager():
                with torch.no_grad():
                    return hf(ids.to(DEV), attention_mask=mask.to(DEV)).last_hidden_state.mean(1)
            legs.append(eager)
        a, b = legs[0](), legs[1]()
        err = float((a - b).abs().max() / a.abs().max())
        assert err < 1e-4, f"few_rows and default features differ by {err:.3e} of the range at B={B} T={T}"
        got = alternate(legs)
        spread, ratio, v = verdict(got[0], got[1])
        line = f"{B:4d} {T:3d}   {stats(got[0])} {spread:7.1f}   {stats(got[1])}   {ratio:6.2f}  {v}"
        if hf is not None:
            line += f"   {stats(got[2])}   {statistics.median(got[2]) / statistics.median(got[1]):6.2f}"
        print(line + f"   (features differ by {err:.1e} of the range)", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    assert torch.cuda.is_available(), "reward_bench.py measures on the GPU; there is no CPU path"
    print(f"# tools/reward_bench.py {mode}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    if mode in ("launches", "all"):
        launches()
    if mode in ("calls", "all"):
        calls()
    if mode in ("steps", "all"):
        steps("--baseline-only" in sys.argv)
    if mode in ("text", "all"):
        text()
    if mode not in ("launches", "calls", "steps", "text", "all"):
        sys.exit(__doc__)
