"""GradLedger (r3m_amd/flat_grads.py): the rule for what the flat gradient buffer holds, driven on the CPU over five plain
parameters with a stand-in for the engine. No native library, no GPU; every comparison is exact."""
import torch
import torch.nn as nn

from r3m_amd.flat_grads import GradLedger, _spans

SIZES = (8, 4, 4, 12, 4)
RANGES = [(sum(SIZES[:i]), n) for i, n in enumerate(SIZES)]
N = sum(SIZES)


def _setup():
    flat_p = torch.zeros(N)
    params = [nn.Parameter(flat_p[off:off + n]) for off, n in RANGES]
    return GradLedger(RANGES), flat_p, params


def _grad(k):
    """the gradient 'backward k' produces: distinct, non-zero, exactly representable values everywhere"""
    return torch.arange(1, N + 1, dtype=torch.float32) * float(k)


def _backward(led, flat_p, params, g):
    """what HipResNet._run_backward does around the engine call; the stand-in engine overwrites (accumulate = 0) or adds to
    (accumulate = 1) the trainable ranges and leaves frozen ranges alone. Returns accumulate."""
    buf = led.grads(flat_p, lambda: params)
    req = [p.requires_grad for p in params]
    accumulate = led.begin(params, req)
    for (off, n), r in zip(RANGES, req):
        if r and accumulate:
            buf[off:off + n] += g[off:off + n]
        elif r:
            buf[off:off + n] = g[off:off + n]
    led.finish()
    return accumulate


def _freeze(params, frozen):
    for i, p in enumerate(params):
        p.requires_grad_(i not in frozen)


def _is_view(p, buf, off):
    return p.grad is not None and p.grad.data_ptr() == buf.data_ptr() + off * 4


def test_gradient_accumulates_only_over_the_backwards_a_tensor_was_trainable_in():
    led, flat_p, params = _setup()
    assert _backward(led, flat_p, params, _grad(100)) == 0       # an earlier step: stale values everywhere
    led.mark_stale()
    _freeze(params, {0, 1, 2, 3})
    g1, g2 = _grad(1), _grad(2)
    assert _backward(led, flat_p, params, g1) == 0
    _freeze(params, {0, 1, 2})
    assert _backward(led, flat_p, params, g2) == 1
    buf = led.grads(flat_p, lambda: params)
    for i, (off, n) in enumerate(RANGES):
        sl = slice(off, off + n)
        if i == 4:
            assert torch.equal(buf[sl], g1[sl] + g2[sl]) and _is_view(params[i], buf, off)
        elif i == 3:
            assert torch.equal(buf[sl], g2[sl]) and _is_view(params[i], buf, off)
        else:
            assert not buf[sl].any() and params[i].grad is None, i
    assert led.written == [False, False, False, True, True]
    assert led.pending()


def test_a_tensor_frozen_across_zero_grad_loses_its_view_and_its_values_but_not_a_grad_of_the_users():
    led, flat_p, params = _setup()
    _backward(led, flat_p, params, _grad(1))
    buf = led.buffer
    assert all(_is_view(p, buf, off) for p, (off, _) in zip(params, RANGES))
    mine = torch.full((SIZES[2],), 7.0)
    params[2].grad = mine                                        # not our view: the user's own tensor
    led.mark_stale()
    assert led.written == [False] * 5 and not led.pending()
    _freeze(params, {1, 2})
    g = _grad(3)
    assert _backward(led, flat_p, params, g) == 0
    assert params[1].grad is None and params[2].grad is mine and torch.equal(mine, torch.full((SIZES[2],), 7.0))
    assert not buf[8:16].any()                                   # both frozen ranges zeroed
    for i in (0, 3, 4):
        off, n = RANGES[i]
        assert torch.equal(buf[off:off + n], g[off:off + n]) and _is_view(params[i], buf, off)
    assert led.written == [True, False, False, True, True] and led.viewed == [True, False, False, True, True]
    # trainable again inside the same window: a fresh view, starting from zero
    _freeze(params, {2})
    assert _backward(led, flat_p, params, g) == 1
    assert _is_view(params[1], buf, 8) and torch.equal(buf[8:12], g[8:12]) and params[2].grad is mine and not buf[12:16].any()


def test_everything_trainable_accumulates_without_a_fill(monkeypatch):
    led, flat_p, params = _setup()
    fills = []
    real = torch.Tensor.zero_
    monkeypatch.setattr(torch.Tensor, "zero_", lambda t: (fills.append(t.numel()), real(t))[1])
    g = _grad(1)
    assert [_backward(led, flat_p, params, g) for _ in range(3)] == [0, 1, 1]
    assert torch.equal(led.buffer, 3 * g)
    led.mark_stale()
    assert _backward(led, flat_p, params, g) == 0
    assert torch.equal(led.buffer, g) and led.written == [True] * 5
    assert fills == []


def test_neighbouring_stale_ranges_are_zeroed_in_one_span():
    assert _spans(RANGES, [0, 1, 3]) == [(0, 12), (16, 28)]
    assert _spans(RANGES, [1, 2, 3, 4]) == [(8, 32)] and _spans(RANGES, [0, 2, 4]) == [(0, 8), (12, 16), (28, 32)]
    assert _spans(RANGES, []) == []
    led, flat_p, params = _setup()
    g = _grad(1)
    _backward(led, flat_p, params, g)
    led.mark_stale()
    _freeze(params, {0, 1, 3})                                   # 0 and 1 are neighbours, 3 stands alone
    g5 = _grad(5)
    _backward(led, flat_p, params, g5)
    buf = led.buffer
    assert not buf[0:12].any() and not buf[16:28].any()
    # the borders: the last zeroed element's neighbours belong to trainable tensors and hold this backward's values
    assert buf[11] == 0 and buf[12] == g5[12] and buf[15] == g5[15] and buf[16] == 0 and buf[27] == 0 and buf[28] == g5[28]
    assert torch.equal(buf[12:16], g5[12:16]) and torch.equal(buf[28:32], g5[28:32])


def test_drop_leaves_no_buffer_no_views_and_nothing_written():
    led, flat_p, params = _setup()
    _backward(led, flat_p, params, _grad(1))
    assert led.pending() and all(led.viewed) and all(led.dirty)
    led.mark_all_written()
    led.drop()
    assert led.buffer is None and led.fresh and not led.pending() and led.ranges == RANGES
    assert led.written == led.dirty == led.viewed == [False] * 5
    for p in params:                                             # the module clears the old views (re-flatten, __setstate__)
        p.grad = None
    buf = led.grads(flat_p, lambda: params)
    assert not buf.any() and all(_is_view(p, buf, off) for p, (off, _) in zip(params, RANGES))
