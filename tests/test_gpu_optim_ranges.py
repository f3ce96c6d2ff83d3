"""The ranged optimizer steps (r3m_adam_step_ranges / r3m_sgd_step_ranges): inside every range bit for bit what r3m_adam_step /
r3m_sgd_step on that slice with that range's step count gives, outside every range nothing is touched. Both forms run the same
element loop of the same kernel, so the comparison is exact (torch.equal on p and the moments): it guards what the entry points hand
that kernel, a dropped step count or offset for instance."""
import pytest
import torch

from optim_cases import CASES, HYPER, N, SGD, _ll, _state
from util import DEV, _st

pytestmark = pytest.mark.gpu


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
