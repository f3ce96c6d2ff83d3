"""Partial-freeze fine-tuning through the Python surface: HipResNet honours requires_grad per parameter and FusedAdam steps exactly
the tensors that received a gradient, with torch's per-parameter step counts. The reference module is a plain autograd graph around
torchvision's ResNet (/root/reference/r3m/models/models_r3m.py:44-52,76,99) where requires_grad_(False) on a sub-tree does this by
itself. ResNet-18, F = 2 frames of 64 x 64.

The optimizer is compared with torch.optim.Adam on the CPU fed the SAME gradients (read back from the HIP encoder), to the tolerances
of test_gpu_ops.py::test_adam_matches_torch (rtol 1e-6): what is under test here is which tensors step and with which step count."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, HW = 2, 64


def _encoder(seed=5):
    from r3m_amd.encoder import HipResNet
    torch.manual_seed(seed)
    m = HipResNet(18).to(DEV)
    m.train()
    flat = m.flat_params()                                  # named_parameters() walks the tensors in flat-buffer order (param_ranges)
    assert all(p.data_ptr() == flat.data_ptr() + off * 4 and p.numel() == cnt for p, (off, cnt) in zip(m.parameters(), m.param_ranges()))
    return m


def _frames(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(F, 3, HW, HW, generator=g) * 255).to(DEV)


def _loss(m, x, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    cw = (torch.rand(F, m.outdim, generator=g) + 0.5).to(DEV)
    return (m(x) * cw).sum()


def _freeze(m, prefixes, frozen=True):
    for n, p in m.named_parameters():
        if n.startswith(tuple(prefixes)):
            p.requires_grad_(not frozen)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


class _TorchAdam:
    """torch.optim.Adam on CPU copies of the encoder's parameters, fed the encoder's own gradients"""

    def __init__(self, m, lr):
        self.p = {n: torch.nn.Parameter(p.detach().cpu().clone()) for n, p in m.named_parameters()}
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr)

    def step(self, m):
        for n, p in m.named_parameters():
            self.p[n].grad = None if p.grad is None else p.grad.detach().cpu().clone()
        self.opt.step()

    def compare(self, m, opt, what):
        for n, p in m.named_parameters():
            torch.testing.assert_close(p.detach().cpu(), self.p[n].detach(), rtol=1e-6, atol=1e-9, msg=lambda s: f"{what}: {n}: {s}")
            st = self.opt.state.get(self.p[n])
            mom = opt.moments(p)
            if st:
                torch.testing.assert_close(mom[0].cpu(), st["exp_avg"], rtol=1e-6, atol=1e-12, msg=lambda s: f"{what}: exp_avg {n}: {s}")
                torch.testing.assert_close(mom[1].cpu(), st["exp_avg_sq"], rtol=1e-6, atol=1e-14, msg=lambda s: f"{what}: exp_avg_sq {n}: {s}")
            elif mom is not None:
                assert not mom[0].any() and not mom[1].any(), f"{what}: {n} never stepped in torch but has moments"


def test_layer4_only_recipe(hip):
    from r3m_amd.optim import FusedAdam
    m = _encoder()
    opt = FusedAdam([m], lr=1e-3)
    # one step with everything trainable: every moment is non-zero, every range of the flat gradient buffer holds something
    opt.zero_grad()
    _loss(m, _frames(1)).backward()
    opt.step()
    assert all(p.grad is not None for p in m.parameters())
    # the recipe: freeze the stem and layer1-3, train layer4
    _freeze(m, ["conv1", "bn1", "layer1", "layer2", "layer3"])
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    assert frozen and len(frozen) < len(list(m.parameters()))
    before = {n: (_bits(p), _bits(opt.moments(p)[0]), _bits(opt.moments(p)[1])) for n, p in m.named_parameters()}
    rm_before = dict(m.named_buffers())["layer1.0.bn1.running_mean"].clone()
    ref = _TorchAdam(m, 1e-3)
    # the reference's state for the trainable tensors: one step taken, the moments the fused optimizer holds
    for n, p in m.named_parameters():
        if n not in frozen:
            mom = opt.moments(p)
            ref.opt.state[ref.p[n]] = {"step": torch.tensor(1.0), "exp_avg": mom[0].cpu().clone(), "exp_avg_sq": mom[1].cpu().clone()}
    opt.zero_grad()
    _loss(m, _frames(2)).backward()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert (p.grad is None) == (n in frozen), n
    g = m.flat_grads()
    for (off, cnt), (n, p) in zip(m.param_ranges(), m.named_parameters()):
        if n in frozen:
            assert not g[off:off + cnt].any(), f"{n}: the never-written range of the flat gradient buffer is not zero"
    ref.step(m)
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        same = [torch.equal(a, b) for a, b in zip(before[n], (_bits(p), _bits(opt.moments(p)[0]), _bits(opt.moments(p)[1])))]
        if n in frozen:
            assert all(same), f"frozen {n} or its moments moved: {same}"
        else:
            assert not any(same), f"trainable {n} did not step: {same}"
            torch.testing.assert_close(p.detach().cpu(), ref.p[n].detach(), rtol=1e-6, atol=1e-9)
    # train-mode BatchNorm in a frozen layer still updates its running statistics, as in torch
    assert not torch.equal(dict(m.named_buffers())["layer1.0.bn1.running_mean"], rm_before)
    assert opt.tensor_steps(0) is not None and set(opt.tensor_steps(0)) == {1, 2}


def test_freeze_unfreeze_schedule_matches_torch_per_parameter_steps(hip):
    from r3m_amd.optim import FusedAdam
    m = _encoder(6)
    opt = FusedAdam([m], lr=1e-3)
    ref = _TorchAdam(m, 1e-3)
    for step, frozen_l1 in enumerate([False, True, False]):
        _freeze(m, ["layer1"], frozen=frozen_l1)
        opt.zero_grad()
        _loss(m, _frames(10 + step), step).backward()
        torch.cuda.synchronize()
        assert all((p.grad is None) == (frozen_l1 and n.startswith("layer1")) for n, p in m.named_parameters())
        ref.step(m)
        opt.step()
        torch.cuda.synchronize()
        ref.compare(m, opt, f"step {step}")
    steps = opt.tensor_steps(0)
    names = [n for n, _ in m.named_parameters()]
    assert all(s == (2 if n.startswith("layer1") else 3) for n, s in zip(names, steps))
    assert opt._steps == [3]
    # the per-tensor counts survive a state_dict round trip; a snapshot without them means "every tensor at the owner's step"
    sd = opt.state_dict()
    opt2 = FusedAdam([m], lr=1e-3)
    opt2.load_state_dict(sd)
    assert opt2.tensor_steps(0) == steps and opt2._steps == [3]
    opt2.load_state_dict({k: v for k, v in sd.items() if k != "tensor_steps"})
    assert opt2.tensor_steps(0) is None and opt2._steps == [3]


def test_gradient_accumulates_only_over_the_backwards_a_tensor_was_trainable_in(hip):
    """zero_grad(); backward 1 with layer4 trainable; unfreeze layer3; backward 2: layer4 holds g1 + g2 (what two accumulating
    backwards of an all-trainable encoder leave there, bit for bit), layer3 holds g2 alone (it starts from zero, not from what an
    earlier step left in the buffer), everything else has no gradient and a zero range."""
    m = _encoder(7)
    x1, x2 = _frames(21), _frames(22)
    full = copy.deepcopy(m)
    only2 = copy.deepcopy(m)
    _loss(m, _frames(20)).backward()                       # an earlier step: stale values everywhere in the flat gradient buffer
    m.mark_grads_stale()                                   # = optimizer.zero_grad()
    _freeze(m, ["conv1", "bn1", "layer1", "layer2", "layer3"])
    _loss(m, x1, 1).backward()
    _freeze(m, ["layer3"], frozen=False)
    _loss(m, x2, 2).backward()
    _loss(full, _frames(20)).backward()                    # (the same BatchNorm running statistics history; gradients do not depend on it)
    full.mark_grads_stale()
    _loss(full, x1, 1).backward()
    _loss(full, x2, 2).backward()
    _loss(only2, x2, 2).backward()
    torch.cuda.synchronize()
    g, g_acc, g_2 = m.flat_grads(), full.flat_grads(), only2.flat_grads()
    for (off, cnt), (n, p) in zip(m.param_ranges(), m.named_parameters()):
        sl = slice(off, off + cnt)
        if n.startswith("layer4"):
            assert torch.equal(g[sl], g_acc[sl]), n
            assert p.grad is not None and p.grad.data_ptr() == g.data_ptr() + off * 4
        elif n.startswith("layer3"):
            assert torch.equal(g[sl], g_2[sl]), n
            assert not torch.equal(g[sl], g_acc[sl]) and p.grad is not None
        else:
            assert not g[sl].any() and p.grad is None, n
    assert m.grads_written() == [n.startswith(("layer3", "layer4")) for n, _ in m.named_parameters()]


@pytest.mark.parametrize("recipe", ["layer4", "bn_only", "all"])
def test_stage_hooks_fire_for_all_four_stages(hip, recipe):
    m = _encoder(8)
    if recipe == "layer4":
        _freeze(m, ["conv1", "bn1", "layer1", "layer2", "layer3"])
    elif recipe == "bn_only":
        for n, p in m.named_parameters():
            p.requires_grad_(p.dim() == 1)
    seen = []
    m._stage_hook = lambda stage, off, cnt: seen.append((stage, off, cnt))
    _loss(m, _frames(30)).backward()
    torch.cuda.synchronize()
    assert [s[0] for s in seen] == [0, 1, 2, 3]
    assert sum(s[2] for s in seen) == m.flat_params().numel()
    assert all((p.grad is not None) == p.requires_grad for p in m.parameters())


def test_input_gradient_with_partly_frozen_parameters(hip):
    """torch.autograd.grad(out, obs) / obs.grad with some parameters frozen: dx equals the all-trainable encoder's bit for bit, and only
    the trainable parameters get a gradient"""
    m = _encoder(9)
    full = copy.deepcopy(m)
    _freeze(m, ["conv1", "bn1", "layer1", "layer2", "layer3"])
    dxs = []
    for enc in (m, full):
        x = _frames(40).requires_grad_(True)
        _loss(enc, x).backward()
        dxs.append(x.grad.clone())
    torch.cuda.synchronize()
    assert torch.equal(dxs[0], dxs[1]) and torch.isfinite(dxs[0]).all()
    for (n, p), (_, q) in zip(m.named_parameters(), full.named_parameters()):
        if p.requires_grad:
            assert torch.equal(p.grad, q.grad), n
        else:
            assert p.grad is None, n
