"""The ranged optimizer steps (r3m_adam_step_ranges / r3m_sgd_step_ranges): inside every range bit for bit what r3m_adam_step /
r3m_sgd_step on that slice with that range's step count gives, outside every range nothing is touched. Both forms run the same
element loop, so the comparison is exact (torch.equal on p and the moments)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 4 * 257 * 9 + 64          # a few blocks of 256 float4 groups, not a multiple of the block


def _st():
    from r3m_amd import _lib
    return _lib.stream_ptr(torch.device(DEV))


def _ll(v):
    return (C.c_longlong * len(v))(*v)


def _state(seed, n=N):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * 0.01
    m = torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 1e-4
    return [t.to(DEV) for t in (p, grad, m, v)]


# (ranges [(offset, count, step)]) — multiples of 4, sorted, disjoint
CASES = {
    "count4": [(8, 4, 1)],
    "count4x257": [(16, 4 * 257, 3)],
    "adjacent": [(0, 64, 2), (64, 1024, 2), (1088, 4, 5)],
    "ends_at_buffer_end": [(4, 12, 1), (N - 4 * 300, 4 * 300, 7)],
    "distinct_steps": [(0, 256, 1), (512, 2048, 2), (4096, 4 * 257, 1000), (N - 8, 8, 4)],
    "65_ranges": [(32 * i, 4 * (1 + i % 7), 1 + i % 3) for i in range(65)],
    "empty_range_between": [(0, 8, 1), (8, 0, 1), (16, 8, 2)],
}
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, gs=0.5)


def _adam(hip, p, g, m, v, n, step, off=0):
    o = off * 4
    assert hip.r3m_adam_step(p.data_ptr() + o, g.data_ptr() + o, m.data_ptr() + o, v.data_ptr() + o, n, HYPER["lr"], HYPER["b1"],
                             HYPER["b2"], HYPER["eps"], step, HYPER["gs"], _st()) == 0


def _adam_ranges(hip, p, g, m, v, ranges):
    off, cnt, step = ([r[k] for r in ranges] for k in range(3))
    return hip.r3m_adam_step_ranges(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ll(off), _ll(cnt), _ll(step), len(ranges),
                                    HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], HYPER["gs"], _st())


def test_one_range_over_the_whole_buffer_equals_adam_step(hip):
    for step in (1, 2, 50):
        p, g, m, v = _state(10 + step)
        p2, m2, v2 = p.clone(), m.clone(), v.clone()
        _adam(hip, p, g, m, v, N, step)
        assert _adam_ranges(hip, p2, g, m2, v2, [(0, N, step)]) == 0
        torch.cuda.synchronize()
        assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2), step
        assert torch.isfinite(p).all()


@pytest.mark.parametrize("case", sorted(CASES))
def test_adam_ranges_inside_equal_slices_outside_untouched(hip, case):
    ranges = CASES[case]
    p, g, m, v = _state(20)
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    pr, mr, vr = p.clone(), m.clone(), v.clone()          # reference: r3m_adam_step on each sub-slice
    inside = torch.zeros(N, dtype=torch.bool, device=DEV)
    for off, cnt, step in ranges:
        if cnt:
            _adam(hip, pr, g, mr, vr, cnt, step, off)
            inside[off:off + cnt] = True
    assert _adam_ranges(hip, p, g, m, v, ranges) == 0
    torch.cuda.synchronize()
    for got, ref, before in ((p, pr, p0), (m, mr, m0), (v, vr, v0)):
        assert torch.equal(got, ref)
        assert torch.equal(got[~inside], before[~inside])
        assert not torch.equal(got[inside], before[inside])


SGD = [dict(momentum=0.0, damp=0.0, wd=0.0, nesterov=0), dict(momentum=0.9, damp=0.0, wd=0.0, nesterov=0),
       dict(momentum=0.9, damp=0.1, wd=1e-2, nesterov=0), dict(momentum=0.9, damp=0.0, wd=1e-2, nesterov=1)]


@pytest.mark.parametrize("cfg", SGD, ids=["plain", "momentum", "damp+wd", "nesterov"])
@pytest.mark.parametrize("case", ["one_range", "adjacent", "distinct_steps", "65_ranges", "ends_at_buffer_end"])
def test_sgd_ranges_inside_equal_slices_outside_untouched(hip, case, cfg):
    ranges = [(0, N, 2)] if case == "one_range" else CASES[case]
    p, g, buf, _ = _state(30)
    p0, b0 = p.clone(), buf.clone()
    pr, br = p.clone(), buf.clone()
    lr, gs = 1e-2, 0.5
    bp = lambda t: t.data_ptr() if cfg["momentum"] else None
    inside = torch.zeros(N, dtype=torch.bool, device=DEV)
    for off, cnt, step in ranges:
        o = off * 4
        assert hip.r3m_sgd_step(pr.data_ptr() + o, g.data_ptr() + o, bp(br) + o if cfg["momentum"] else None, cnt, lr, cfg["momentum"],
                                cfg["damp"], cfg["wd"], cfg["nesterov"], step, gs, _st()) == 0
        inside[off:off + cnt] = True
    off, cnt, step = ([r[k] for r in ranges] for k in range(3))
    assert hip.r3m_sgd_step_ranges(p.data_ptr(), g.data_ptr(), bp(buf), _ll(off), _ll(cnt), _ll(step), len(ranges), lr, cfg["momentum"],
                                   cfg["damp"], cfg["wd"], cfg["nesterov"], gs, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(p, pr) and torch.equal(buf, br)
    assert torch.equal(p[~inside], p0[~inside]) and torch.equal(buf[~inside], b0[~inside])
    assert not torch.equal(p[inside], p0[inside])
    if cfg["momentum"]:
        assert not torch.equal(buf[inside], b0[inside])
