#!/usr/bin/env python
"""GPU: what a cross-clip negative costs in a whole Trainer.update step. ResNet-50, 256 clips (1280 frames), two configurations:
  fp32-tcn    fp32 encoder, time-contrastive loss only (langweight 0)
  bf16-lang   bf16 encoder and head, time-contrastive + language loss on precomputed sentence features
each at num_negatives N = 1, 3, 8, 16, plus N = 3 on the parent commit's library through the entry points it has ("3 base":
tools/build_ab.sh HEAD, R3M_HIP_LIB). Every leg is a fresh child process (one library per process); the legs of a configuration are
interleaved, `rounds` times over, and the spread between the rounds of the same leg is printed next to every figure: a difference
between two legs below that spread is not a difference. Per leg: ms per step (median of `steps` after `warmup`, host-synchronised),
the objective (ops.r3m_loss forward, which computes its gradients too) and the head (batched_scores forward + backward) timed on their
own with HIP events on the step's shapes, their share of the step, and the cost per added negative from N = 3 to N = 16.
usage: negatives_bench.py [rounds=2] [steps=8] [warmup=3] [out=profiles/negatives.txt]      (writes the table to `out` and to stdout)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
BASE_LIB = os.path.join(ROOT, "r3m_amd", "lib", "libr3m_hip_base.so")
B, SIZE = 256, 50


def events_ms(fn, reps=10):
    import torch
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def leg(cfg, N, steps, warmup, old):
    import time
    import torch
    from r3m_amd import R3M, _lib, ops
    from r3m_amd.parallel import SingleDevice
    from r3m_amd.trainer import Trainer
    if old:
        from negatives_bits import use_old_entries
        use_old_entries(_lib.lib())
    lang = cfg == "bf16-lang"
    dev = "cuda:0"
    m = R3M("cuda", 1e-4, 1024, size=SIZE, l2weight=1e-5, l1weight=1e-5, langweight=1.0 if lang else 0.0, tcnweight=1.0,
            precision="bf16" if lang else "fp32", num_negatives=N)
    model = SingleDevice(m).to(dev)
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (B, 5, 3, 224, 224), generator=g, dtype=torch.uint8).to(dev).float()
    feats = (torch.rand((B, 768), generator=g) * 1.2 - 0.6).to(dev)
    batch = (frames, (feats, torch.ones(B)) if lang else [""] * B)
    T = Trainer(1)
    torch.manual_seed(1)
    times = []
    for s in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T.update(model, batch, s)
        torch.cuda.synchronize()
        if s >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    D = m.outdim
    alle = torch.relu(torch.rand((B, 5, D), generator=g) * 1.5 - 0.5).to(dev)
    tcn_perm = torch.stack([torch.randperm(B, generator=g) for _ in range(2 * N)]).to(torch.int32).to(dev)
    lang_perm = torch.stack([torch.randperm(B, generator=g) for _ in range(3 * N)]).to(torch.int32).to(dev)
    scores = torch.rand((6 + 3 * N, B), generator=g).to(dev) if lang else None
    mask = torch.ones(B, device=dev) if lang else None
    obj_ms = events_ms(lambda: ops.r3m_loss(alle, tcn_perm, 1e-5, 1e-5, 1.0, scores=scores, mask=mask, langweight=1.0 if lang else 0.0,
                                            num_negatives=N))
    head_ms = 0.0
    if lang:
        a = alle.clone().requires_grad_(True)
        w = torch.rand((6 + 3 * N, B), generator=g).to(dev)

        def head():
            m.lang_rew.mark_grads_stale()
            a.grad = None
            (m.lang_rew.batched_scores(a, feats, lang_perm) * w).sum().backward()
        head_ms = events_ms(head)
    print(json.dumps({"cfg": cfg, "N": N, "old": old, "step_ms": statistics.median(times), "objective_ms": obj_ms, "head_ms": head_ms}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        return leg(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6] == "old")
    rounds, steps, warmup = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 2), (2, 8), (3, 3)))
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "negatives.txt")
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    have_base = os.path.exists(BASE_LIB)
    legs = [(3, "base")] * have_base + [(1, ""), (3, ""), (8, ""), (16, "")]
    res = {}
    for cfg in ("fp32-tcn", "bf16-lang"):
        for r in range(rounds):
            for N, which in (legs if r % 2 == 0 else legs[::-1]):
                env = dict(os.environ)
                env.pop("R3M_HIP_LIB", None)
                if which == "base":
                    env["R3M_HIP_LIB"] = BASE_LIB
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", cfg, str(N), str(steps), str(warmup), "old" if which else "n"]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.exit(f"leg {cfg} N={N} {which} failed ({p.returncode}):\n{p.stderr[-2000:]}")
                res.setdefault((cfg, N, which), []).append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(f"round {r} {cfg} N={N} {which}: {p.stdout.strip().splitlines()[-1]}", file=sys.stderr, flush=True)
    emit(f"ResNet-{SIZE}, {B} clips, Trainer.update; {rounds} interleaved rounds per leg, median of {steps} steps after {warmup}; "
          "figure = mean over the rounds, +- = half the range over the rounds of that leg")
    if not have_base:
        emit("no r3m_amd/lib/libr3m_hip_base.so (tools/build_ab.sh HEAD): the parent-library legs were left out")
    for cfg in ("fp32-tcn", "bf16-lang"):
        emit(f"\n{cfg}\n  {'leg':<10}{'step ms':>18}{'objective ms':>20}{'head fwd+bwd ms':>20}{'objective share':>17}{'head share':>12}")
        mean = {}
        for N, which in legs:
            rows = res[(cfg, N, which)]
            col = {}
            for k in ("step_ms", "objective_ms", "head_ms"):
                v = [x[k] for x in rows]
                col[k] = (sum(v) / len(v), (max(v) - min(v)) / 2)
            mean[(N, which)] = col
            st = col["step_ms"][0]
            emit(f"  N={N:<2} {which:<5}" + "".join(f"{col[k][0]:>11.3f} +-{col[k][1]:6.3f}" for k in ("step_ms", "objective_ms", "head_ms"))
                  + f"{100 * col['objective_ms'][0] / st:>15.2f} %{100 * col['head_ms'][0] / st:>10.2f} %")
        a, b = mean[(3, "")], mean[(16, "")]
        emit(f"  per added negative (N = 3 -> 16): step {(b['step_ms'][0] - a['step_ms'][0]) / 13:.3f} ms, objective "
              f"{(b['objective_ms'][0] - a['objective_ms'][0]) / 13:.4f} ms, head {(b['head_ms'][0] - a['head_ms'][0]) / 13:.3f} ms")
        if have_base:
            o = mean[(3, "base")]
            for k, name in (("step_ms", "step"), ("objective_ms", "objective (3 launches)"), ("head_ms", "head")):
                d, spread = a[k][0] - o[k][0], max(a[k][1], o[k][1])
                emit(f"  N = 3 against the parent's library, {name}: {d:+.3f} ms, spread of the legs {spread:.3f} ms -> "
                      + ("inside the spread" if abs(d) <= spread else ("SLOWER than the parent beyond the spread" if d > 0 else
                                                                          "faster than the parent beyond the spread")))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
