"""Fused Adam over flat parameter buffers (one HIP kernel per flat buffer) — the `encoder_opt` of R3M.

Replaces torch.optim.Adam(params, lr=lr) built at /root/reference/r3m/models/models_r3m.py:76 and stepped at
/root/reference/r3m/trainer.py:156-158 (defaults: betas (0.9, 0.999), eps 1e-8, weight_decay 0, amsgrad False).
"""
import ctypes as C

import torch

from . import _lib


def _ll(v):
    return (C.c_longlong * len(v))(*v)


class _PerTensorSteps:
    """Step counts per parameter TENSOR of an owner, as torch.optim keeps them per parameter: a tensor that got no gradient (frozen,
    requires_grad False) is not stepped and its count — hence its Adam bias correction — stays behind. Kept as each tensor's lag
    behind the owner's count `_steps[i]` (None: no tensor lags, the state of every run that never froze anything), so code that sets
    `_steps` by hand keeps meaning "every tensor at that step".

    Owners that expose param_ranges() / grads_written() (HipResNet) are stepped tensor by tensor; the others (the language head,
    whose tensors are not 4-aligned) stay all-or-nothing through has_grads()."""

    def _advance(self, i, owner):
        """Advance the counts of owner i's tensors that received a gradient since zero_grad(). Returns None when there is nothing to
        step, "all" when the whole flat buffer steps with one count (self._steps[i], already advanced), else (offsets, counts, steps)
        of the merged ranges: neighbouring tensors with equal counts form one range."""
        if not hasattr(owner, "param_ranges"):
            if not getattr(owner, "has_grads", lambda: True)():
                return None
            self._steps[i] += 1
            return "all"
        written = owner.grads_written()
        if not any(written):
            return None
        lag = self._lag[i]
        if lag is None and all(written):
            self._steps[i] += 1
            return "all"
        ranges = owner.param_ranges()
        base = self._steps[i]
        steps = [base] * len(ranges) if lag is None else [base - l for l in lag]
        steps = [s + 1 if w else s for s, w in zip(steps, written)]
        base = max(steps)
        self._steps[i] = base
        lag = [base - s for s in steps]
        self._lag[i] = lag if any(lag) else None
        offs, counts, rsteps = [], [], []
        for (off, n), s, w in zip(ranges, steps, written):
            if not w:
                continue
            if offs and offs[-1] + counts[-1] == off and rsteps[-1] == s:
                counts[-1] += n
            else:
                offs.append(off); counts.append(n); rsteps.append(s)
        if len(offs) == 1 and offs[0] == 0 and counts[0] == owner.flat_params().numel():
            return "all"
        return offs, counts, rsteps

    def tensor_steps(self, i):
        """absolute step count per tensor of owner i (None: every tensor at self._steps[i])"""
        return None if self._lag[i] is None else [self._steps[i] - l for l in self._lag[i]]

    def _load_tensor_steps(self, sd):
        ts = sd.get("tensor_steps")        # absent in snapshots from before per-tensor counts: every tensor at its owner's step
        self._lag = [None] * len(self.owners)
        for i, t in enumerate(ts or []):
            if t is not None:
                lag = [self._steps[i] - int(s) for s in t]
                self._lag[i] = lag if any(lag) else None


class FusedAdam(_PerTensorSteps, torch.optim.Optimizer):
    """`owners` are modules exposing flat_params() / flat_grads() / mark_grads_stale() (HipResNet, LanguageReward)."""

    def __init__(self, owners, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.owners = list(owners)
        params = [p for o in self.owners for p in o.parameters()]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._steps = [0] * len(self.owners)   # torch.optim.Adam keeps `step` per parameter: an owner that receives its first
        self._m = [None] * len(self.owners)    # gradient later (the language head) starts its bias correction then
        self._v = [None] * len(self.owners)
        self._lag = [None] * len(self.owners)  # per-tensor lag behind _steps (_PerTensorSteps)
        self.grad_scale = 1.0

    def __getstate__(self):
        # Optimizer.__getstate__ keeps defaults/state/param_groups only; deepcopy(R3M) and pickling must keep the owners
        # protocol and the moments too (the reference's torch.optim.Adam deep-copies with its state).
        st = super().__getstate__()
        st.update(owners=self.owners, _steps=self._steps, _m=self._m, _v=self._v, _lag=self._lag, grad_scale=self.grad_scale)
        return st

    def zero_grad(self, set_to_none=True):
        # Gradients live in persistent flat buffers; "zeroing" = the next backward overwrites them (no memset pass).
        for o in self.owners:
            o.mark_grads_stale()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("FusedAdam.step(closure) is not supported")
        g0 = self.param_groups[0]
        lr, (b1, b2), eps = g0["lr"], g0["betas"], g0["eps"]
        L = _lib.lib()
        for i, o in enumerate(self.owners):
            p = o.flat_params()
            if not p.is_cuda:
                raise RuntimeError("r3m_amd.FusedAdam: parameters must live on the GPU (HIP kernel, no CPU fallback)")
            todo = self._advance(i, o)         # what torch.optim.Adam steps: the tensors with a gradient since zero_grad()
            if todo is None:
                continue
            g = o.flat_grads()
            if self._m[i] is None or self._m[i].device != p.device or self._m[i].numel() != p.numel():
                self._m[i] = torch.zeros_like(p)
                self._v[i] = torch.zeros_like(p)
            n = p.numel()
            pad = (-n) % 4
            assert pad == 0, "flat buffers are padded to multiples of 4 floats"
            with _lib.on(p):
                if todo == "all":
                    _lib.check(L.r3m_adam_step(p.data_ptr(), g.data_ptr(), self._m[i].data_ptr(), self._v[i].data_ptr(), n, float(lr),
                                               float(b1), float(b2), float(eps), self._steps[i], float(self.grad_scale),
                                               _lib.stream_ptr(p.device)), "adam_step")
                else:                          # some tensors frozen, or at other step counts: one launch over the ranges
                    offs, counts, steps = todo
                    _lib.check(L.r3m_adam_step_ranges(p.data_ptr(), g.data_ptr(), self._m[i].data_ptr(), self._v[i].data_ptr(),
                                                      _ll(offs), _ll(counts), _ll(steps), len(offs), float(lr), float(b1), float(b2),
                                                      float(eps), float(self.grad_scale), _lib.stream_ptr(p.device)), "adam_step_ranges")

    def moments(self, param):
        """Read-only views (exp_avg, exp_avg_sq) of Adam's moments for one parameter, shaped and strided like it — what
        `torch.optim.Adam.state[param]` holds in the reference (models_r3m.py:76). None before the owner's first step."""
        for i, o in enumerate(self.owners):
            flat = o.flat_params()
            off = (param.data_ptr() - flat.data_ptr()) // flat.element_size()
            if param.device == flat.device and 0 <= off and off + param.numel() <= flat.numel():
                if self._m[i] is None:
                    return None
                view = lambda t: torch.as_strided(t.detach(), param.shape, param.stride(), off)
                return view(self._m[i]), view(self._v[i])
        raise KeyError("FusedAdam.moments: the tensor is not a parameter of this optimizer's owners")

    @property
    def _step(self):
        """Step count of the first owner (the encoder): what the snapshot's `step` key has always meant."""
        return self._steps[0]

    # state: enough to resume (the reference never saved optimizer state, train_representation.py:123-130)
    def state_dict(self):
        return {"step": self._steps[0], "steps": list(self._steps), "tensor_steps": [self.tensor_steps(i) for i in range(len(self.owners))],
                "exp_avg": [None if m is None else m.cpu() for m in self._m],
                "exp_avg_sq": [None if v is None else v.cpu() for v in self._v], "grad_scale": float(self.grad_scale), "param_groups": [
                    {k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def load_state_dict(self, sd):
        steps = sd.get("steps")           # round-1 snapshots carry one shared `step`
        steps = [int(s) for s in steps] if steps is not None else [int(sd["step"])] * len(self.owners)
        n = len(self.owners)
        if len(steps) != n or len(sd["exp_avg"]) != n or len(sd["exp_avg_sq"]) != n:
            # e.g. saved with langweight=0 (encoder only) and resumed with a language head, or the reverse: silently
            # mis-assigning moments between owners would be worse than refusing
            raise ValueError(f"FusedAdam.load_state_dict: the snapshot holds optimizer state for {len(steps)} flat buffer(s) "
                             f"({len(sd['exp_avg'])} moment entries), this optimizer has {n} "
                             f"({', '.join(type(o).__name__ for o in self.owners)}); was it saved with a different langweight?")
        for i, o in enumerate(self.owners):
            m = sd["exp_avg"][i]
            if m is not None and m.numel() != o.flat_params().numel():
                raise ValueError(f"FusedAdam.load_state_dict: moments of owner {i} ({type(o).__name__}) have {m.numel()} elements, "
                                 f"its parameters {o.flat_params().numel()}")
        self._steps = steps
        self._load_tensor_steps(sd)
        for i, o in enumerate(self.owners):
            if sd["exp_avg"][i] is not None:
                dev = o.flat_params().device
                self._m[i] = sd["exp_avg"][i].to(dev)
                self._v[i] = sd["exp_avg_sq"][i].to(dev)
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        if "grad_scale" in sd:              # absent in older snapshots: the optimizer keeps the one it has
            self.grad_scale = float(sd["grad_scale"])


class FusedSGD(_PerTensorSteps, torch.optim.Optimizer):
    """torch.optim.SGD semantics (momentum, dampening, weight_decay, nesterov) as one HIP kernel per flat buffer. The reference
    only ever builds Adam (models_r3m.py:76); this is the plain alternative on the same owners protocol."""

    def __init__(self, owners, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.owners = list(owners)
        params = [p for o in self.owners for p in o.parameters()]
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov))
        self._steps = [0] * len(self.owners)
        self._buf = [None] * len(self.owners)
        self._lag = [None] * len(self.owners)
        self.grad_scale = 1.0

    def zero_grad(self, set_to_none=True):
        for o in self.owners:
            o.mark_grads_stale()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("FusedSGD.step(closure) is not supported")
        g0 = self.param_groups[0]
        L = _lib.lib()
        for i, o in enumerate(self.owners):
            p = o.flat_params()
            if not p.is_cuda:
                raise RuntimeError("r3m_amd.FusedSGD: parameters must live on the GPU (HIP kernel, no CPU fallback)")
            todo = self._advance(i, o)
            if todo is None:
                continue
            g = o.flat_grads()
            if g0["momentum"] != 0 and (self._buf[i] is None or self._buf[i].device != p.device or self._buf[i].numel() != p.numel()):
                self._buf[i] = torch.zeros_like(p)
            buf_ptr = None if self._buf[i] is None else self._buf[i].data_ptr()
            with _lib.on(p):
                if todo == "all":
                    _lib.check(L.r3m_sgd_step(p.data_ptr(), g.data_ptr(), buf_ptr, p.numel(), float(g0["lr"]), float(g0["momentum"]),
                                              float(g0["dampening"]), float(g0["weight_decay"]), int(bool(g0["nesterov"])),
                                              self._steps[i], float(self.grad_scale), _lib.stream_ptr(p.device)), "sgd_step")
                else:
                    offs, counts, steps = todo
                    _lib.check(L.r3m_sgd_step_ranges(p.data_ptr(), g.data_ptr(), buf_ptr, _ll(offs), _ll(counts), _ll(steps), len(offs),
                                                     float(g0["lr"]), float(g0["momentum"]), float(g0["dampening"]),
                                                     float(g0["weight_decay"]), int(bool(g0["nesterov"])), float(self.grad_scale),
                                                     _lib.stream_ptr(p.device)), "sgd_step_ranges")

    def __getstate__(self):
        st = super().__getstate__()
        st.update(owners=self.owners, _steps=self._steps, _buf=self._buf, _lag=self._lag, grad_scale=self.grad_scale)
        return st

    # state: enough to resume, in the manner of FusedAdam's (torch's own state_dict would drop the momentum buffers, the step counts and
    # grad_scale, which all live outside Optimizer.state)
    def state_dict(self):
        return {"steps": list(self._steps), "tensor_steps": [self.tensor_steps(i) for i in range(len(self.owners))],
                "momentum_buffer": [None if b is None else b.cpu() for b in self._buf], "grad_scale": float(self.grad_scale),
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def load_state_dict(self, sd):
        n = len(self.owners)
        if len(sd["steps"]) != n or len(sd["momentum_buffer"]) != n:
            raise ValueError(f"FusedSGD.load_state_dict: the snapshot holds optimizer state for {len(sd['steps'])} flat buffer(s), this "
                             f"optimizer has {n} ({', '.join(type(o).__name__ for o in self.owners)})")
        for i, o in enumerate(self.owners):
            b = sd["momentum_buffer"][i]
            if b is not None and b.numel() != o.flat_params().numel():
                raise ValueError(f"FusedSGD.load_state_dict: the momentum buffer of owner {i} ({type(o).__name__}) has {b.numel()} elements, "
                                 f"its parameters {o.flat_params().numel()}")
        self._steps = [int(s) for s in sd["steps"]]
        self._load_tensor_steps(sd)
        for i, o in enumerate(self.owners):
            b = sd["momentum_buffer"][i]
            self._buf[i] = None if b is None else b.to(o.flat_params().device)
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        if "grad_scale" in sd:
            self.grad_scale = float(sd["grad_scale"])
