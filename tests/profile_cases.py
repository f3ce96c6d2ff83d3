"""The cases of tests/test_gpu_profile.py, picked from the lists the operator tests already have: of every group of cases that the
dispatch and the profiler's classes cannot tell apart, the smallest member. Needs the library's host-side queries, no GPU.

A group is (routes of the forward with statistics, routes of the plain forward, routes of the input gradient, weight-gradient route,
classes of the three operations). Shared by the GPU test and by tests/test_profile_model.py, which checks what the picked cases cover."""
import functools

import profile_model as pm
import route_sig

FP32, BF16 = 0, 1
STEM_CASES = [(2, 34, 32), (3, 33, 35)]          # two of util.STEM_EDGE_CASES: a straddling last tile; odd H and W
HEAD_SHAPE = (1, 32, 64, 32)                     # test_gpu_langrew_edges.FP32_CASES[0]: B = 1 -> R = 15 rows, K1 = 2 D + LD = 96, H = 64
HEAD_SHAPE_BF16 = (1, 32, 64, 64)                # test_gpu_langrew_edges.BF16_CASES[0]
# one fp32 1x1 and one 3x3 for the switch tests: forward, input gradient and weight gradient of the first are wide (classes 0, 0, 2), of
# the second narrow (1, 1, 3)
SWITCH_CASES = [(2, 9, 7, 256, 128, 1, 1, 0), (2, 9, 7, 64, 64, 3, 1, 1)]


def case_key(L, case, dt):
    fwd_s = route_sig.routes(L, case, 0, route_sig.STATS, 0, dt)
    fwd = route_sig.routes(L, case, 0, 0, 0, dt)
    dg = route_sig.routes(L, case, 1, 0, 0, dt)
    plan = route_sig.wgrad_plan(L, case, dt)
    cls = (pm.forward_launches(case, dt, 0, fwd)[0].kclass, tuple(l.kclass for l in pm.dgrad_launches(case, dt, 0, 0, dg)),
           pm.wgrad_class(case))
    return (fwd_s, fwd, dg, route_sig.wgrad_variant(plan), plan.split > 1, cls)


def work(case):
    N, Hi, Wi, Ci, Co, k, s, p = case
    return N * Hi * Wi * Ci * Co * k * k


@functools.lru_cache(maxsize=None)
def conv_cases():
    """[(case, dt)]"""
    import test_gpu_ops_hw as T
    from r3m_amd import _lib
    L = _lib.lib()
    out = []
    for dt, cases in ((FP32, T.HW_CONV_CASES), (BF16, T.HW_BF16_CASES + T.HW_ROW16_CASES)):
        best = {}
        for c in cases:
            if not route_sig.routes(L, c, 0, 0, 0, dt) or not route_sig.routes(L, c, 1, 0, 0, dt):
                continue                    # a combination the dispatch refuses for this dtype
            key = case_key(L, c, dt)
            if key not in best or (work(c), c) < (work(best[key]), best[key]):
                best[key] = c
        out += [(c, dt) for c in sorted(best.values())]
    return out


def case_id(v):
    if isinstance(v, tuple) and len(v) == 8:
        return "N{}_{}x{}_{}to{}_k{}s{}p{}".format(*v)
    return {0: "fp32", 1: "bf16"}.get(v, str(v))
