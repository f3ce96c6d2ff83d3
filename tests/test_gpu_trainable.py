"""Partial-freeze backward of the engine (r3m_resnet_set_trainable): for every mask of the fine-tuning recipes, a masked backward over
the saved activations of ONE forward against the full backward over the same activations. The masked backward only drops launches —
the kernels that remain see the inputs of the full backward and the engine is deterministic — so every trainable tensor's gradient
and the input gradient are BIT-identical to the full backward's, and every frozen tensor's range of the gradient buffer is never
written (it still holds the sentinel it was filled with). ResNet-18 / 50, fp32 / bf16, F = 2 frames of 64 x 64 (general stem, layer4
map 2 x 2) and of 224 x 224 (specialised stem)."""
import pytest
import torch

from trainable_masks import mask_bytes, masks, tensor_ranges

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 2
SENTINEL = 0x7FC5A5A5      # (int32) a NaN bit pattern no kernel produces
CONFIGS = [(size, prec, hw) for size in (18, 50) for prec in ("fp32", "bf16") for hw in (64, 224)]


def _stream():
    from r3m_amd import _lib
    return _lib.stream_ptr(torch.device(DEV))


class _Run:
    """One plan, one forward, and the full backward's results (with dx) on it."""

    def __init__(self, hip, size, prec, hw):
        from r3m_amd.encoder import HipResNet
        self.hip = hip
        torch.manual_seed(1000 + size + hw)
        enc = HipResNet(size).to(DEV)
        with torch.no_grad():                                   # BatchNorm affine away from (1, 0): every sum matters
            for n, p in enc.named_parameters():
                if p.dim() == 1:
                    p.add_(torch.randn_like(p) * 0.1)
        self.p = enc.flat_params().clone()
        self.b = enc._flat_b.clone()
        self.h = hip.r3m_resnet_create_hw(size, F, 1 if prec == "bf16" else 0, hw, hw)
        assert self.h
        self.tensors = tensor_ranges(hip, self.h)
        self.names = [(n, k) for n, k, _, _ in self.tensors]
        self.arena = torch.empty(hip.r3m_resnet_arena_bytes(self.h), dtype=torch.uint8, device=DEV)
        D = hip.r3m_resnet_out_dim(self.h)
        self.x = torch.rand(F, 3, hw, hw, device=DEV) * 255
        self.out = torch.empty(F, D, device=DEV)
        self.dh = torch.randn(F, D, device=DEV)
        assert hip.r3m_resnet_forward(self.h, self.x.data_ptr(), self.p.data_ptr(), self.b.data_ptr(), self.arena.data_ptr(),
                                      self.out.data_ptr(), 1, _stream()) == 0
        self.full, self.full_dx = self.backward(None, True)
        torch.cuda.synchronize()
        assert torch.isfinite(self.full).all() and torch.isfinite(self.full_dx).all()

    def close(self):
        self.hip.r3m_resnet_destroy(self.h)

    def set_mask(self, trainable):
        """trainable: set of tensor names, or None = the default"""
        if trainable is None:
            return self.hip.r3m_resnet_set_trainable(self.h, None, 0)
        m = mask_bytes(self.names, trainable)
        return self.hip.r3m_resnet_set_trainable(self.h, m, len(m))

    def call(self, g, dx, stage_begin=0, stage_end=4, dx_now=True):
        return self.hip.r3m_resnet_backward_ex(self.h, self.dh.data_ptr(), self.p.data_ptr(), None if g is None else g.data_ptr(),
                                               self.arena.data_ptr(), stage_begin, stage_end, 0,
                                               dx.data_ptr() if dx is not None and dx_now else None, 0, _stream())

    def backward(self, trainable, want_dx, staged=False, grads=True):
        """-> (gradient buffer as int32 bits pre-filled with the sentinel, dx or None) of a stage-0 restart under the mask"""
        assert self.set_mask(trainable) == 0
        g = torch.full((self.p.numel(),), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32) if grads else None
        dx = torch.full_like(self.x, float("nan")) if want_dx else None
        if staged:
            for st in range(4):
                assert self.call(g, dx, st, st + 1) == 0, st
        else:
            assert self.call(g, dx) == 0
        return g, dx

    def check(self, g, trainable, what):
        gi, fi = g.view(torch.int32), self.full.view(torch.int32)
        for name, kind, off, n in self.tensors:
            if kind > 2:
                continue
            if name in trainable:
                assert torch.equal(gi[off:off + n], fi[off:off + n]), f"{what}: gradient of {name} differs from the full backward's"
            else:
                assert bool((gi[off:off + n] == SENTINEL).all()), f"{what}: frozen {name} was written"


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: f"r{c[0]}-{c[1]}-{c[2]}")
def run(request, hip):
    r = _Run(hip, *request.param)
    yield r
    r.close()


def test_full_backward_is_reproducible_and_mask_free(run):
    """the comparisons below rest on this: a stage-0 restart over the same activations gives the same bits, with or without dx, with
    the all-ones mask or none"""
    every = {n for n, k in run.names if k <= 2}
    for trainable, want_dx in ((None, False), (every, True), (every, False)):
        g, dx = run.backward(trainable, want_dx)
        torch.cuda.synchronize()
        assert torch.equal(g.view(torch.int32), run.full.view(torch.int32))
        if want_dx:
            assert torch.equal(dx, run.full_dx)


@pytest.mark.parametrize("want_dx", [False, True], ids=["nodx", "dx"])
def test_masked_backward_is_bit_identical_where_trainable_and_silent_where_frozen(run, want_dx):
    for name, trainable in masks(run.names).items():
        g, dx = run.backward(trainable, want_dx)
        torch.cuda.synchronize()
        run.check(g, trainable, f"mask {name}")
        if want_dx:
            assert torch.equal(dx, run.full_dx), f"mask {name}: dx differs from the full backward's"


def test_all_zero_mask_equals_the_backward_without_gradient_buffer(run):
    g, dx = run.backward(set(), True)
    _, dx_null = run.backward(None, True, grads=False)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_null) and torch.equal(dx, run.full_dx)
    run.check(g, set(), "all-zero mask")


def test_staged_calls_equal_one_call(run):
    all_masks = masks(run.names)
    for name in ("layer4", "from_layer3.1", "bn_only", "layer1.0.conv1", "none"):
        g, dx = run.backward(all_masks[name], True, staged=True)
        torch.cuda.synchronize()
        run.check(g, all_masks[name], f"staged, mask {name}")
        assert torch.equal(dx, run.full_dx), name
    # without dx: stages without work enqueue nothing and return 0
    g, _ = run.backward(all_masks["layer4"], False, staged=True)
    torch.cuda.synchronize()
    run.check(g, all_masks["layer4"], "staged, mask layer4, no dx")


def test_set_trainable_between_stages_is_refused(run):
    from r3m_amd import _lib
    all_masks = masks(run.names)
    assert run.set_mask(all_masks["layer4"]) == 0
    g = torch.full((run.p.numel(),), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    assert run.call(g, None, 0, 1) == 0
    assert run.set_mask(all_masks["bn_only"]) != 0
    assert "between its stages" in _lib.last_error()
    assert run.set_mask(None) != 0
    # the running backward goes on under the mask it began with ...
    assert run.call(g, None, 1, 4) == 0
    torch.cuda.synchronize()
    run.check(g, all_masks["layer4"], "after a refused set_trainable")
    # ... and the next stage-0 restart takes a new one
    g, dx = run.backward(all_masks["bn_only"], True)
    torch.cuda.synchronize()
    run.check(g, all_masks["bn_only"], "restart under a new mask")
    assert torch.equal(dx, run.full_dx)


def test_dx_must_be_announced_at_stage_zero_when_the_chain_stops_early(run):
    """layer4 only: the backward planned without dx stops at layer4.0; asking stage 3 for dx then is an error, not garbage"""
    from r3m_amd import _lib
    all_masks = masks(run.names)
    assert run.set_mask(all_masks["layer4"]) == 0
    g = torch.full((run.p.numel(),), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    dx = torch.zeros_like(run.x)
    assert run.call(g, dx, 0, 3, dx_now=False) == 0
    assert run.call(g, dx, 3, 4) != 0
    assert "stage 0" in _lib.last_error()
    # all trainable: dx handed to the stage-3 call alone works as it always did
    assert run.set_mask(None) == 0
    assert run.call(g, dx, 0, 3, dx_now=False) == 0
    assert run.call(g, dx, 3, 4) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, run.full_dx)
