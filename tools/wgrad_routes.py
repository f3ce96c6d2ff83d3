#!/usr/bin/env python
"""Table of the weight-gradient dispatch (no GPU): one line per launch with the plan r3m_debug_wgrad_route reports (csrc/wgrad.hip
wgrad_plan) and the split-K workspace, for every convolution behind the stem of ResNet-18 / 34 / 50 at the frame counts of
tests/test_dispatch.py, the reward head's Linear layers, and every case of the GPU operator lists; fp32 and bf16.
profiles/wgrad_unify_routes.txt is this listing from the dispatch before it was unified: the library must reproduce it field for field.
  python tools/wgrad_routes.py | diff - profiles/wgrad_unify_routes.txt"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import route_sig
from r3m_amd import _lib
from test_dispatch import _layers


def launches():
    for (size, frames) in ((50, 1280), (34, 2560), (18, 2560), (18, 8)):
        for (name, H, Ci, Co, k, s, p, _, _) in _layers(size):
            yield f"resnet{size}_F{frames} {name}", (frames, H, H, Ci, Co, k, s, p), (0, 1)
    for R in (15 * 256, 15 * 512):
        for K in (2 * 512 + 768, 2 * 2048 + 768, 1024):
            yield f"head_R{R}", (R, 1, 1, K, 1024, 1, 1, 0), (0, 1)
    for (origin, case, dt) in route_sig.wgrad_operator_cases():
        yield origin, case, (dt,)


def plan(L, case, dt):
    return tuple(route_sig.wgrad_plan(L, case, dt))


def main(plan=plan):
    L = _lib.lib()
    print("# origin | N Hi Wi Ci Co k stride pad | dtype | " + " ".join(route_sig.WgPlan._fields) + " | workspace floats / (Co k k Ci)")
    seen = set()
    for (origin, case, dts) in launches():
        for dt in dts:
            if (origin, case, dt) in seen:
                continue
            seen.add((origin, case, dt))
            N, Hi, Wi, Ci, Co, k, s, p = case
            ws = L.r3m_conv2d_wgrad_workspace_bytes_dt(*case, dt) // (4 * Co * k * k * Ci)
            print(f"{origin} | {' '.join(map(str, case))} | {'bf16' if dt else 'fp32'} | {' '.join(map(str, plan(L, case, dt)))} | {ws}")


if __name__ == "__main__":
    main()
