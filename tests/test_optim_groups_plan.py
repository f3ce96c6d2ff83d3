"""not gpu: the host side of parameter groups, weight decay and gradient clipping in the fused optimizers (r3m_amd/optim.py): how groups
become ranges (neighbours merge only when step count, learning rate and weight decay are all equal), the constructor's refusals, when
the grouped entry points are needed at all, what the two group builders put where for ResNet-18 / 34 / 50, and the host-side refusals of
the new C entry points (nothing is launched, so no GPU is needed for them to return)."""
import ctypes as C

import pytest
import torch

from r3m_amd.optim import FusedAdam, FusedAdamW, FusedSGD, _StepPlan, layerwise_lr_groups, no_decay_groups


class _Ranged(torch.nn.Module):
    """a fake owner with param_ranges(): tensors of the given sizes (multiples of 4), views into one flat CPU buffer"""

    def __init__(self, sizes=(8, 4, 16, 4, 12)):
        super().__init__()
        self.flat = torch.arange(float(sum(sizes)))
        self.g = torch.zeros(sum(sizes))
        self._ranges, off = [], 0
        for k, n in enumerate(sizes):
            shape = (n // 4, 4) if k % 2 == 0 else (n,)          # even tensors 2-D ("weights"), odd ones 1-D ("biases")
            self.register_parameter(f"t{k}", torch.nn.Parameter(self.flat[off:off + n].view(shape)))
            self._ranges.append((off, n))
            off += n
        self.written = [True] * len(sizes)

    def flat_params(self):
        return self.flat

    def flat_grads(self):
        return self.g

    def mark_grads_stale(self):
        pass

    def param_ranges(self):
        return self._ranges

    def grads_written(self):
        return self.written


class _Whole(torch.nn.Module):
    """a fake owner without param_ranges() (the language head: all or nothing)"""

    def __init__(self):
        super().__init__()
        self.flat = torch.zeros(24)
        self.w = torch.nn.Parameter(self.flat[:20].view(4, 5))
        self.b = torch.nn.Parameter(self.flat[20:24])

    def flat_params(self):
        return self.flat

    def flat_grads(self):
        return torch.zeros(24)

    def mark_grads_stale(self):
        pass

    def has_grads(self):
        return True


def _plan(opt, i=0):
    p = opt._plan(i, opt.owners[i])
    return None if p is None else (p.whole, p.offs, p.counts, p.steps, p.lrs, p.wds)


def test_without_groups_the_plan_is_the_whole_buffer_and_needs_no_grouped_call():
    o = _Ranged()
    opt = FusedAdam([o], lr=1e-3)
    assert _plan(opt) == (True, [0], [44], [1], [1e-3], [0.0])
    p = opt._plan(0, o)
    assert p.steps == [2] and not p.needs_groups(False, False)
    assert p.needs_groups(True, False)                               # clipping needs the coefficient
    o.written = [True, True, False, True, True]                      # a frozen tensor: ranges, still the plain ranged call
    p = opt._plan(0, o)
    assert (p.whole, p.offs, p.counts, p.steps) == (False, [0, 28], [12, 16], [3, 3]) and not p.needs_groups(False, False)


def test_equal_neighbours_merge_and_differences_split():
    o = _Ranged()
    t = [o.t0, o.t1, o.t2, o.t3, o.t4]
    # lr differs between t1 and t2; weight decay between t3 and t4; t0, t1 equal
    opt = FusedAdam([o], lr=1e-3, param_groups=[{"params": [t[0], t[1]], "lr": 1e-4}, {"params": [t[2], t[3]]},
                                                {"params": [t[4]], "weight_decay": 0.1}])
    assert _plan(opt) == (False, [0, 12, 32], [12, 20, 12], [1, 1, 1], [1e-4, 1e-3, 1e-3], [0.0, 0.0, 0.1])
    # a step difference splits too: t3 misses a step, then comes back one count behind t2
    o.written = [True, True, True, False, True]
    assert _plan(opt) == (False, [0, 12, 32], [12, 16, 12], [2, 2, 2], [1e-4, 1e-3, 1e-3], [0.0, 0.0, 0.1])
    o.written = [True] * 5
    assert _plan(opt) == (False, [0, 12, 28, 32], [12, 16, 4, 12], [3, 3, 2, 3], [1e-4, 1e-3, 1e-3, 1e-3], [0.0, 0.0, 0.0, 0.1])
    assert opt.tensor_steps(0) == [3, 3, 3, 2, 3]
    # groups are read on every call: equal hyper-parameters everywhere and no lag left -> one range again
    o2 = _Ranged()
    opt2 = FusedAdam([o2], lr=1e-3, param_groups=[{"params": [o2.t0], "lr": 1e-4}])
    assert len(opt2.param_groups) == 2 and _plan(opt2)[1:3] == ([0, 8], [8, 36])
    opt2.param_groups[0]["lr"] = 1e-3
    assert _plan(opt2) == (True, [0], [44], [2], [1e-3], [0.0])
    opt2.param_groups[1]["weight_decay"] = 0.5
    assert _plan(opt2) == (False, [0, 8], [8, 36], [3, 3], [1e-3, 1e-3], [0.0, 0.5])


def test_the_ranges_to_step_decide_not_the_groups_that_exist():
    """a frozen group with another learning rate does not force the grouped call"""
    o = _Ranged()
    opt = FusedAdam([o], lr=1e-3, param_groups=[{"params": [o.t0, o.t1], "lr": 1e-5}])
    o.written = [False, False, True, True, True]
    p = opt._plan(0, o)
    assert (p.offs, p.counts, p.lrs) == ([12], [32], [1e-3]) and not p.needs_groups(False, False)
    o.written = [True] * 5
    assert opt._plan(0, o).needs_groups(False, False)


def test_needs_groups_predicate():
    one = lambda lr, wd: _StepPlan(True, [0], [8], [1], [lr], [wd])
    assert not one(1e-3, 0.0).needs_groups(False, False)
    assert one(1e-3, 0.0).needs_groups(True, False) and one(1e-3, 0.0).needs_groups(True, True)
    assert one(1e-3, 0.1).needs_groups(False, False)                 # r3m_adam_step has no weight decay
    assert not one(1e-3, 0.1).needs_groups(False, True)              # r3m_sgd_step has one
    two = lambda a, b: _StepPlan(False, [0, 8], [4, 4], [1, 1], [a[0], b[0]], [a[1], b[1]])
    assert not two((1e-3, 0.0), (1e-3, 0.0)).needs_groups(False, False)
    assert two((1e-3, 0.0), (1e-4, 0.0)).needs_groups(False, True)
    assert two((1e-3, 0.0), (1e-3, 0.1)).needs_groups(False, True)
    assert not two((1e-3, 0.1), (1e-3, 0.1)).needs_groups(False, True)
    assert FusedAdam._plain_weight_decay is False and FusedSGD._plain_weight_decay is True


def test_the_norm_takes_neighbouring_ranges_as_one():
    from r3m_amd.optim import _coalesce
    assert _coalesce([0, 12, 32], [12, 20, 12]) == ([0], [44])
    assert _coalesce([0, 12, 36], [12, 20, 8]) == ([0, 36], [32, 8])
    assert _coalesce([8], [4]) == ([8], [4]) and _coalesce([], []) == ([], [])


def test_an_owner_without_ranges_takes_its_groups_values():
    o, w = _Ranged(), _Whole()
    opt = FusedSGD([o, w], lr=1e-2, momentum=0.9, param_groups=[{"params": list(w.parameters()), "lr": 0.5, "weight_decay": 0.25}])
    assert _plan(opt, 1) == (True, [0], [24], [1], [0.5], [0.25])
    assert _plan(opt, 0) == (True, [0], [44], [1], [1e-2], [0.0])


def test_constructor_refusals():
    o, w = _Ranged(), _Whole()
    with pytest.raises(ValueError, match=r"_Ranged\.t2 appears in more than one parameter group"):
        FusedAdam([o], param_groups=[{"params": [o.t2, o.t0]}, {"params": [o.t1, o.t2]}])
    with pytest.raises(ValueError, match="no parameter of the owners"):
        FusedAdam([o], param_groups=[{"params": [torch.nn.Parameter(torch.zeros(4))]}])
    with pytest.raises(ValueError, match="_Whole has no param_ranges.*one group"):
        FusedAdam([o, w], param_groups=[{"params": [w.w], "weight_decay": 0.1}])
    with pytest.raises(ValueError, match="_Whole has no param_ranges"):
        FusedSGD([o, w], param_groups=no_decay_groups([o, w], 0.1))
    FusedAdam([o, w], param_groups=[{"params": [w.w, w.b], "weight_decay": 0.1}])          # the head as a whole: fine
    with pytest.raises(ValueError, match="betas.*optimizer-wide"):
        FusedAdam([o], param_groups=[{"params": [o.t0], "betas": (0.5, 0.9)}])
    with pytest.raises(ValueError, match="eps.*optimizer-wide"):
        FusedAdamW([o], param_groups=[{"params": [o.t0], "eps": 1e-3}])
    with pytest.raises(ValueError, match="momentum.*optimizer-wide"):
        FusedSGD([o], momentum=0.9, param_groups=[{"params": [o.t0], "momentum": 0.5}])
    FusedAdam([o], param_groups=[{"params": [o.t0], "betas": (0.9, 0.999)}])               # restating the optimizer's own value: fine
    with pytest.raises(ValueError, match="must be >= 0"):
        FusedAdam([o], weight_decay=-1.0)


def test_defaults_and_snapshot_keys():
    o = _Ranged()
    a = FusedAdamW([o])
    g = a.param_groups[0]
    assert g["weight_decay"] == 1e-2 and g["decoupled_weight_decay"] is True and g["max_grad_norm"] is None and a.last_grad_norm is None
    assert FusedAdam([o]).param_groups[0]["weight_decay"] == 0.0 and FusedAdam([o]).param_groups[0]["decoupled_weight_decay"] is False
    opt = FusedAdam([o], lr=1e-3, max_grad_norm=2.0, param_groups=[{"params": [o.t0], "lr": 1e-4, "weight_decay": 0.3}])
    sd = opt.state_dict()
    assert [(g["lr"], g["weight_decay"], g["max_grad_norm"]) for g in sd["param_groups"]] == [(1e-4, 0.3, 2.0), (1e-3, 0.0, 2.0)]
    fresh = FusedAdam([o], lr=7.0, param_groups=[{"params": [o.t0]}])
    fresh.load_state_dict(sd)
    assert [(g["lr"], g["weight_decay"]) for g in fresh.param_groups] == [(1e-4, 0.3), (1e-3, 0.0)] and fresh.max_grad_norm == 2.0
    # a snapshot from before: one group without the new keys -> the constructor's values hold
    old = dict(sd, param_groups=[{"lr": 5.0, "betas": (0.9, 0.999), "eps": 1e-8}])
    keep = FusedAdam([o], lr=1e-3, max_grad_norm=2.0, param_groups=[{"params": [o.t0], "lr": 1e-4, "weight_decay": 0.3}])
    keep.load_state_dict(old)
    assert [(g["lr"], g["weight_decay"]) for g in keep.param_groups] == [(1e-4, 0.3), (1e-3, 0.0)] and keep.max_grad_norm == 2.0
    single = FusedAdam([o], lr=1e-3, weight_decay=0.2)
    single.load_state_dict(old)
    assert single.param_groups[0]["lr"] == 5.0 and single.param_groups[0]["weight_decay"] == 0.2
    with pytest.raises(ValueError, match="parameter groups"):
        FusedAdam([o], param_groups=[{"params": [o.t0]}, {"params": [o.t1]}]).load_state_dict(sd)


@pytest.mark.parametrize("size", [18, 34, 50])
def test_group_builders_on_the_encoders(size):
    from r3m_amd.encoder import HipResNet
    net = HipResNet(size)
    named = dict(net.named_parameters())
    name_of = {id(p): n for n, p in named.items()}
    decay, plain = no_decay_groups(net, 0.05, lr=3e-4)
    assert decay["weight_decay"] == 0.05 and plain["weight_decay"] == 0.0 and decay["lr"] == plain["lr"] == 3e-4
    dn, pn = {name_of[id(p)] for p in decay["params"]}, {name_of[id(p)] for p in plain["params"]}
    assert dn | pn == set(named) and not dn & pn
    assert dn == {n for n in named if "conv" in n or "downsample.0" in n}                 # exactly the convolution weights
    assert pn == {n for n in named if "bn" in n or "downsample.1" in n} and all(named[n].dim() == 1 for n in pn)
    lw = layerwise_lr_groups(net, 1e-3, 0.5)
    assert [g["lr"] for g in lw] == [1e-3 * 0.5 ** 4, 1e-3 * 0.5 ** 3, 1e-3 * 0.25, 1e-3 * 0.5, 1e-3]
    sets = [{name_of[id(p)] for p in g["params"]} for g in lw]
    assert sets[0] == {"conv1.weight", "bn1.weight", "bn1.bias"}
    for k in range(1, 5):
        assert sets[k] == {n for n in named if n.startswith(f"layer{k}.")} and sets[k]
    assert sum(len(s) for s in sets) == len(named)
    both = no_decay_groups(lw, 0.05)                                                       # composed: ten groups
    assert len(both) == 10 and [g["lr"] for g in both[::2]] == [g["lr"] for g in lw]
    assert all(g["weight_decay"] == (0.05 if i % 2 == 0 else 0.0) for i, g in enumerate(both))
    opt = FusedAdamW([net], param_groups=both)
    assert len(opt.param_groups) == 10                                                     # every tensor named: no rest group
    net._grads.mark_all_written()
    p = opt._plan(0, net)
    # every range is one run of neighbours with one (lr, wd); adjacent ranges differ; together they cover the buffer
    assert p.offs[0] == 0 and p.offs[-1] + p.counts[-1] == net.flat_params().numel()
    assert all(a + n == b for a, n, b in zip(p.offs, p.counts, p.offs[1:]))
    assert all(x != y for x, y in zip(zip(p.lrs, p.wds), list(zip(p.lrs, p.wds))[1:]))
    want = {}
    for g in both:
        for t in g["params"]:
            want[(t.data_ptr() - net.flat_params().data_ptr()) // 4] = (g["lr"], g["weight_decay"])
    for (off, n) in net.param_ranges():
        k = max(i for i, o in enumerate(p.offs) if o <= off)
        assert off + n <= p.offs[k] + p.counts[k] and (p.lrs[k], p.wds[k]) == want[off]


def _ll(v):
    return (C.c_longlong * len(v))(*v)


def _dd(v):
    return (C.c_double * len(v))(*v)


@pytest.mark.parametrize("entry", ["adam", "sgd", "sqnorm"])
def test_new_entry_points_refuse_on_the_host(entry):
    """Bad ranges, a negative learning rate or weight decay and null arrays with n_ranges > 0 return non-zero with a message before
    anything is launched: the buffer pointers are never dereferenced."""
    from r3m_amd import _lib
    lib = _lib.lib()
    fake = 4096
    assert lib.r3m_grad_sqnorm_workspace_bytes() >= 64 * 8

    def call(off, count, step, lr=None, wd=None, null=False):
        n = len(off)
        lr = [1e-3] * n if lr is None else lr
        wd = [0.0] * n if wd is None else wd
        arr = (lambda f, v: None) if null else (lambda f, v: f(v))
        if entry == "adam":
            return lib.r3m_adam_step_groups(fake, fake, fake, fake, arr(_ll, off), arr(_ll, count), arr(_ll, step), arr(_dd, lr), arr(_dd, wd),
                                            n, 0.9, 0.999, 1e-8, 1, 1.0, None, None)
        if entry == "sgd":
            return lib.r3m_sgd_step_groups(fake, fake, fake, arr(_ll, off), arr(_ll, count), arr(_ll, step), arr(_dd, lr), arr(_dd, wd), n,
                                           0.9, 0.0, 0, 1.0, None, None)
        return lib.r3m_grad_sqnorm_ranges(fake, arr(_ll, off), arr(_ll, count), n, fake, 0, fake, lib.r3m_grad_sqnorm_workspace_bytes(), None)

    bad = {
        "offset not a multiple of 4": ([2], [8], [1]),
        "count not a multiple of 4": ([0], [6], [1]),
        "overlapping": ([0, 4], [8, 8], [1, 1]),
        "unsorted": ([16, 0], [4, 4], [1, 1]),
        "negative offset": ([-4], [4], [1]),
    }
    tag = {"adam": "adam_groups", "sgd": "sgd_groups", "sqnorm": "grad_sqnorm_ranges"}[entry]
    for what, (off, count, step) in bad.items():
        assert call(off, count, step) != 0, what
        assert tag in _lib.last_error(), (what, _lib.last_error())
    assert call([0], [4], [1], null=True) != 0 and "null" in _lib.last_error()
    if entry != "sqnorm":
        assert call([0], [4], [0]) != 0 and "step" in _lib.last_error()
        assert call([0, 8], [4, 4], [1, 1], lr=[1e-3, -1e-3]) != 0 and "lr" in _lib.last_error()
        assert call([0, 8], [4, 4], [1, 1], wd=[-0.1, 0.0]) != 0 and "weight_decay" in _lib.last_error()
        assert call([0], [4], [1], lr=[float("nan")]) != 0
        assert call([], [], []) == 0                                  # no range: nothing to launch
    else:
        assert lib.r3m_grad_sqnorm_ranges(fake, _ll([0]), _ll([4]), 1, fake, 0, fake, 16, None) != 0 and "workspace" in _lib.last_error()
        assert lib.r3m_grad_sqnorm_ranges(fake, _ll([0]), _ll([4]), 1, None, 0, fake, 1 << 30, None) != 0
    assert lib.r3m_clip_coef(None, 1.0, 1.0, fake, None) != 0 and "clip_coef" in _lib.last_error()
    assert lib.r3m_clip_coef(fake, -1.0, 1.0, fake, None) != 0 and "max_norm" in _lib.last_error()
    assert lib.r3m_abi_version() == 1
