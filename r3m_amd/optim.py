"""Fused Adam over flat parameter buffers (one HIP kernel per flat buffer) — the `encoder_opt` of R3M.

Replaces torch.optim.Adam(params, lr=lr) built at /root/reference/r3m/models/models_r3m.py:76 and stepped at
/root/reference/r3m/trainer.py:156-158 (defaults: betas (0.9, 0.999), eps 1e-8, weight_decay 0, amsgrad False).

Beyond the reference: parameter groups with their own lr / weight_decay (torch's `[{"params": [...], "lr": ...}]` idiom), weight decay
(L2 as torch.optim.Adam(weight_decay=), decoupled as torch.optim.AdamW) and global gradient-norm clipping (torch.nn.utils.clip_grad_norm_)
without leaving the one-launch-per-flat-buffer design: see FusedAdam, FusedAdamW, FusedSGD, no_decay_groups, layerwise_lr_groups.
"""
import ctypes as C

import torch

from . import _lib


def _ll(v):
    return (C.c_longlong * len(v))(*v)


def _dd(v):
    return (C.c_double * len(v))(*v)


class _StepPlan:
    """What one owner steps now: sorted ranges with a step count, a learning rate and a weight decay each. `whole`: one range over the
    whole flat buffer."""
    __slots__ = ("whole", "offs", "counts", "steps", "lrs", "wds")

    def __init__(self, whole, offs, counts, steps, lrs, wds):
        self.whole, self.offs, self.counts, self.steps, self.lrs, self.wds = whole, offs, counts, steps, lrs, wds

    def needs_groups(self, clip, plain_weight_decay):
        """False: the plain entry points (r3m_*_step / r3m_*_step_ranges) do this step, argument for argument as before parameter
        groups existed. True when the ranges differ in (lr, weight_decay), when the gradient is clipped, or when there is a weight
        decay the plain entry point does not know (`plain_weight_decay`: r3m_sgd_step has one, r3m_adam_step has none)."""
        if clip or len(set(zip(self.lrs, self.wds))) > 1:
            return True
        return self.wds[0] != 0 and not plain_weight_decay


def _coalesce(offs, counts):
    """neighbouring ranges as one: the same elements in fewer, larger ranges (the gradient norm knows no step count, lr or decay)"""
    o, c = [], []
    for off, n in zip(offs, counts):
        if o and o[-1] + c[-1] == off:
            c[-1] += n
        else:
            o.append(off); c.append(n)
    return o, c


def _owner_param_names(owners):
    return {id(p): (i, f"{type(o).__name__}.{name}") for i, o in enumerate(owners) for name, p in o.named_parameters()}


def _make_groups(what, owners, param_groups, defaults, optimizer_wide):
    """torch's `[{"params": [...], "lr": ...}, ...]` checked against the owners -> the groups to hand torch.optim.Optimizer. Owner
    parameters that no group names form a last group with the defaults."""
    names = _owner_param_names(owners)
    seen, groups = {}, []
    for gi, g in enumerate(param_groups):
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError(f"{what}: param_groups[{gi}] must be a dict with a 'params' entry")
        ps = g["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        for k in optimizer_wide:
            if k in g and g[k] != defaults[k]:
                raise ValueError(f"{what}: param_groups[{gi}] sets {k}={g[k]!r}, but {k} is optimizer-wide ({defaults[k]!r}); only lr and "
                                 f"weight_decay may differ between groups")
        for p in ps:
            if id(p) not in names:
                shape = tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__
                raise ValueError(f"{what}: param_groups[{gi}] holds a tensor {shape} that is no parameter of the owners")
            if id(p) in seen:
                raise ValueError(f"{what}: {names[id(p)][1]} appears in more than one parameter group "
                                 f"(param_groups[{seen[id(p)]}] and param_groups[{gi}])")
            seen[id(p)] = gi
        groups.append({**g, "params": ps})
    rest = [p for o in owners for p in o.parameters() if id(p) not in seen]
    if rest:
        for p in rest:
            seen[id(p)] = len(groups)
        groups.append({"params": rest})
    for o in owners:
        if not hasattr(o, "param_ranges"):
            gs = sorted({seen[id(p)] for p in o.parameters()})
            if len(gs) > 1:
                raise ValueError(f"{what}: {type(o).__name__} has no param_ranges() (its tensors are not 4-aligned) and cannot be split: "
                                 f"all of its parameters must lie in one group, they lie in param_groups{gs}")
    return groups


class _FlatOptimizer(torch.optim.Optimizer):
    """What FusedAdam and FusedSGD share: the owners protocol, step counts per parameter tensor, parameter groups turned into ranges,
    gradient clipping and the snapshot.

    Step counts per parameter TENSOR of an owner, as torch.optim keeps them per parameter: a tensor that got no gradient (frozen,
    requires_grad False) is not stepped and its count — hence its Adam bias correction — stays behind. Kept as each tensor's lag
    behind the owner's count `_steps[i]` (None: no tensor lags, the state of every run that never froze anything), so code that sets
    `_steps` by hand keeps meaning "every tensor at that step".

    Owners that expose param_ranges() / grads_written() (HipResNet) are stepped tensor by tensor; the others (the language head,
    whose tensors are not 4-aligned) stay all-or-nothing through has_grads()."""
    _name = None                     # the class name in messages (FusedAdamW speaks as FusedAdam)
    _plain_weight_decay = False      # whether the plain entry points take a (global) weight decay: r3m_sgd_step does
    _moments = ()                    # (attribute, snapshot key) of the per-owner state buffers; the first leads in messages
    _mismatch = _elements = None     # load_state_dict's refusals

    def __init__(self, owners, defaults, param_groups, optimizer_wide):
        if defaults["weight_decay"] < 0 or defaults["lr"] < 0:
            raise ValueError(f"{self._name}: lr={defaults['lr']} and weight_decay={defaults['weight_decay']} must be >= 0")
        self.owners = list(owners)
        if param_groups is None:
            params = [p for o in self.owners for p in o.parameters()]
        else:
            params = _make_groups(type(self).__name__, self.owners, param_groups, defaults, optimizer_wide + ("max_grad_norm",))
        super().__init__(params, defaults)
        n = len(self.owners)
        self._steps = [0] * n                  # torch.optim.Adam keeps `step` per parameter: an owner that receives its first gradient
        self._lag = [None] * n                 # later (the language head) starts its bias correction then; per-tensor lag behind _steps
        self._range_groups = [None] * n        # per owner: (address of its flat buffer, group index of each range) -- found again by address
        self._clip_bufs = {}                   # device -> (fp64 accumulator [1], {coef, norm} [2], workspace)
        self.last_grad_norm = None             # device scalar: the gradient norm of the last clipped step, before clipping
        self.grad_scale = 1.0
        for attr, _ in self._moments:
            setattr(self, attr, [None] * n)

    def __getstate__(self):
        # Optimizer.__getstate__ keeps defaults/state/param_groups only; deepcopy(R3M) and pickling must keep the owners
        # protocol and the moments too (the reference's torch.optim.Adam deep-copies with its state).
        st = super().__getstate__()
        st.update(owners=self.owners, _steps=self._steps, _lag=self._lag, grad_scale=self.grad_scale,
                  _range_groups=[None] * len(self.owners), _clip_bufs={}, last_grad_norm=None,      # device scratch is re-created
                  **{attr: getattr(self, attr) for attr, _ in self._moments})
        return st

    @property
    def max_grad_norm(self):
        return self.param_groups[0].get("max_grad_norm")

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        for g in self.param_groups:
            g["max_grad_norm"] = v

    def zero_grad(self, set_to_none=True):
        # Gradients live in persistent flat buffers; "zeroing" = the next backward overwrites them (no memset pass).
        for o in self.owners:
            o.mark_grads_stale()

    def tensor_steps(self, i):
        """absolute step count per tensor of owner i (None: every tensor at self._steps[i])"""
        return None if self._lag[i] is None else [self._steps[i] - l for l in self._lag[i]]

    # ---- groups -> ranges ----
    def _groups_of_ranges(self, i, owner):
        """group index per param_ranges() entry of owner i (one entry for an owner without ranges), by address like moments()"""
        flat = owner.flat_params()
        cached = self._range_groups[i]
        if cached is not None and cached[0] == (flat.data_ptr(), flat.device):
            return cached[1]
        ranges = owner.param_ranges() if hasattr(owner, "param_ranges") else None
        index = {off: k for k, (off, _) in enumerate(ranges)} if ranges is not None else None
        out = [None] * (len(ranges) if ranges is not None else 1)
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                off = (p.data_ptr() - flat.data_ptr()) // flat.element_size()
                if p.device != flat.device or off < 0 or off + p.numel() > flat.numel():
                    continue
                k = 0 if index is None else index.get(off)
                if k is None:
                    raise RuntimeError("parameter groups: a parameter does not start at a range of its owner's flat buffer")
                if out[k] is not None and out[k] != gi:
                    raise RuntimeError("parameter groups: one flat range belongs to two groups")
                out[k] = gi
        if any(k is None for k in out):
            raise RuntimeError("parameter groups: some of the owners' parameters are in no group (were parameters replaced after the "
                               "optimizer was built?)")
        self._range_groups[i] = ((flat.data_ptr(), flat.device), out)
        return out

    def _hyper(self, i, owner):
        """(lr, weight_decay) of owner i as the groups hold them NOW (schedulers and manual edits take effect): one pair when it is the
        same for all of the owner's ranges, else a list with one pair per param_ranges() entry"""
        groups = self.param_groups
        pair = lambda g: (float(g["lr"]), float(g.get("weight_decay", 0.0)))
        if len(groups) == 1:
            return pair(groups[0])
        pairs = [pair(groups[k]) for k in self._groups_of_ranges(i, owner)]
        return pairs[0] if all(p == pairs[0] for p in pairs) else pairs

    def _plan(self, i, owner):
        """Advance the step counts of owner i's tensors that received a gradient since zero_grad() and return what to step now as a
        _StepPlan (None: nothing). Neighbouring tensors form one range when step count, learning rate and weight decay are all equal."""
        h = self._hyper(i, owner)
        per_range = isinstance(h, list)
        n = owner.flat_params().numel()
        ranged = hasattr(owner, "param_ranges")
        written = owner.grads_written() if ranged else [getattr(owner, "has_grads", lambda: True)()]
        if not any(written):
            return None
        lag = self._lag[i]
        if not ranged or (lag is None and all(written) and not per_range):      # the whole flat buffer at one step count
            self._steps[i] += 1
            return _StepPlan(True, [0], [n], [self._steps[i]], [h[0]], [h[1]])
        ranges = owner.param_ranges()
        base = self._steps[i]
        steps = [base] * len(ranges) if lag is None else [base - l for l in lag]
        steps = [s + 1 if w else s for s, w in zip(steps, written)]
        base = max(steps)
        self._steps[i] = base
        lag = [base - s for s in steps]
        self._lag[i] = lag if any(lag) else None
        plan = _StepPlan(False, [], [], [], [], [])
        for (off, count), s, w, (lr, wd) in zip(ranges, steps, written, h if per_range else [h] * len(ranges)):
            if not w:
                continue
            if plan.offs and (plan.offs[-1] + plan.counts[-1], plan.steps[-1], plan.lrs[-1], plan.wds[-1]) == (off, s, lr, wd):
                plan.counts[-1] += count
            else:
                plan.offs.append(off); plan.counts.append(count); plan.steps.append(s); plan.lrs.append(lr); plan.wds.append(wd)
        plan.whole = plan.offs == [0] and plan.counts == [n]
        return plan

    # ---- clipping ----
    def _clip_scratch(self, device):
        b = self._clip_bufs.get(device)
        if b is None:
            ws = int(_lib.lib().r3m_grad_sqnorm_workspace_bytes())
            b = (torch.zeros(1, dtype=torch.float64, device=device), torch.zeros(2, dtype=torch.float32, device=device),
                 torch.empty(ws, dtype=torch.uint8, device=device))
            self._clip_bufs[device] = b
        return b

    def _begin_step(self):
        """Advance the step counts of every owner, then (max_grad_norm) take ONE gradient norm over exactly the ranges about to be
        stepped, all owners in order, and form the clip coefficient on the device. -> ([(i, owner, plan)], coefficient pointer or None)"""
        plans = []
        for i, o in enumerate(self.owners):
            if not o.flat_params().is_cuda:
                raise RuntimeError(f"r3m_amd.{self._name}: parameters must live on the GPU (HIP kernel, no CPU fallback)")
            plan = self._plan(i, o)            # what torch.optim steps: the tensors with a gradient since zero_grad()
            if plan is not None:
                plans.append((i, o, plan))
                if hasattr(o, "params_written"):
                    o.params_written()         # the step about to be enqueued rewrites this owner's flat parameters
        max_norm = self.max_grad_norm
        if max_norm is None or not plans:
            return plans, None
        L = _lib.lib()
        dev = plans[0][1].flat_params().device
        if any(o.flat_params().device != dev for _, o, _ in plans):
            raise RuntimeError(f"r3m_amd.{self._name}: max_grad_norm needs every owner on one device (one norm over all of them)")
        acc, coef_norm, ws = self._clip_scratch(dev)
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            for k, (_, o, plan) in enumerate(plans):       # the first owner writes the accumulator, the others add to it
                offs, counts = _coalesce(plan.offs, plan.counts)
                _lib.check(L.r3m_grad_sqnorm_ranges(o.flat_grads().data_ptr(), _ll(offs), _ll(counts), len(offs), acc.data_ptr(),
                                                    int(k > 0), ws.data_ptr(), ws.numel(), st), "grad_sqnorm_ranges")
            _lib.check(L.r3m_clip_coef(acc.data_ptr(), float(max_norm), float(self.grad_scale), coef_norm.data_ptr(), st), "clip_coef")
        self.last_grad_norm = coef_norm[1]
        return plans, coef_norm.data_ptr()

    # ---- state: enough to resume (the reference never saved optimizer state, train_representation.py:123-130; torch's own state_dict
    # would drop the moment buffers, the step counts and grad_scale, which all live outside Optimizer.state) ----
    def state_dict(self):
        return {"steps": list(self._steps), "tensor_steps": [self.tensor_steps(i) for i in range(len(self.owners))],
                **{key: [None if t is None else t.cpu() for t in getattr(self, attr)] for attr, key in self._moments},
                "grad_scale": float(self.grad_scale), "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def _saved_steps(self, sd):
        return sd["steps"]

    def load_state_dict(self, sd):
        what, n = f"{self._name}.load_state_dict", len(self.owners)
        steps = [int(s) for s in self._saved_steps(sd)]
        saved = [(attr, sd[key]) for attr, key in self._moments]
        if len(steps) != n or any(len(s) != n for _, s in saved):
            # e.g. saved with langweight=0 (encoder only) and resumed with a language head, or the reverse: silently
            # mis-assigning moments between owners would be worse than refusing
            raise ValueError(what + self._mismatch.format(k=len(steps), e=len(saved[0][1]), n=n,
                                                          names=", ".join(type(o).__name__ for o in self.owners)))
        for i, o in enumerate(self.owners):
            t = saved[0][1][i]
            if t is not None and t.numel() != o.flat_params().numel():
                raise ValueError(what + self._elements.format(i=i, t=type(o).__name__, k=t.numel(), n=o.flat_params().numel()))
        self._steps = steps
        ts = sd.get("tensor_steps")        # absent in snapshots from before per-tensor counts: every tensor at its owner's step
        self._lag = [None] * n
        for i, t in enumerate(ts or []):
            if t is not None:
                lag = [self._steps[i] - int(s) for s in t]
                self._lag[i] = lag if any(lag) else None
        for attr, s in saved:
            for i, o in enumerate(self.owners):
                if s[i] is not None:        # an owner the snapshot holds no buffer for keeps what it has
                    getattr(self, attr)[i] = s[i].to(o.flat_params().device)
        groups = sd["param_groups"]
        if len(groups) == len(self.param_groups):
            for g, s in zip(self.param_groups, groups):     # keys a snapshot from before lacks keep the constructor's values
                g.update(s)
        elif len(groups) != 1:                              # one group: a snapshot from before parameter groups; the constructor's hold
            raise ValueError(f"{what}: the snapshot has {len(groups)} parameter groups, this optimizer {len(self.param_groups)}")
        if "grad_scale" in sd:              # absent in older snapshots: the optimizer keeps the one it has
            self.grad_scale = float(sd["grad_scale"])


class FusedAdam(_FlatOptimizer):
    """`owners` are modules exposing flat_params() / flat_grads() / mark_grads_stale() (HipResNet, LanguageReward).

    weight_decay: torch.optim.Adam's L2 term (g += wd * p), or with decoupled_weight_decay torch.optim.AdamW's (p *= 1 - lr * wd).
    param_groups: torch's idiom, a list of {"params": [tensors], "lr": ..., "weight_decay": ...}; owner parameters no group names form a
    last group with the defaults; betas, eps, decoupled_weight_decay and max_grad_norm are optimizer-wide. step() reads lr and
    weight_decay from the groups on every call (torch.optim.lr_scheduler.* works, per group).
    max_grad_norm: torch.nn.utils.clip_grad_norm_(all owners' parameters, max_grad_norm) before the step, on the gradient times
    grad_scale (the averaged gradient under the data-parallel wrapper), in two launches per flat buffer and without a host wait;
    `last_grad_norm` is then the norm before clipping as a device scalar (None before the first clipped step).
    Without groups, weight decay and clipping the calls into the library are those of the plain optimizer, argument for argument."""
    _name = "FusedAdam"
    _moments = (("_m", "exp_avg"), ("_v", "exp_avg_sq"))
    _mismatch = (": the snapshot holds optimizer state for {k} flat buffer(s) ({e} moment entries), this optimizer has {n} ({names}); "
                 "was it saved with a different langweight?")
    _elements = ": moments of owner {i} ({t}) have {k} elements, its parameters {n}"

    def __init__(self, owners, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False, max_grad_norm=None,
                 param_groups=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=bool(decoupled_weight_decay),
                        max_grad_norm=max_grad_norm)
        super().__init__(owners, defaults, param_groups, ("betas", "eps", "decoupled_weight_decay"))

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("FusedAdam.step(closure) is not supported")
        g0 = self.param_groups[0]
        (b1, b2), eps, decoupled = g0["betas"], g0["eps"], bool(g0.get("decoupled_weight_decay", False))
        L = _lib.lib()
        plans, coef = self._begin_step()
        for i, o, plan in plans:
            p = o.flat_params()
            g = o.flat_grads()
            if self._m[i] is None or self._m[i].device != p.device or self._m[i].numel() != p.numel():
                self._m[i] = torch.zeros_like(p)
                self._v[i] = torch.zeros_like(p)
            n = p.numel()
            pad = (-n) % 4
            assert pad == 0, "flat buffers are padded to multiples of 4 floats"
            with _lib.on(p):
                if plan.needs_groups(coef is not None, self._plain_weight_decay):     # groups that differ, a weight decay or clipping
                    _lib.check(L.r3m_adam_step_groups(p.data_ptr(), g.data_ptr(), self._m[i].data_ptr(), self._v[i].data_ptr(),
                                                      _ll(plan.offs), _ll(plan.counts), _ll(plan.steps), _dd(plan.lrs), _dd(plan.wds),
                                                      len(plan.offs), float(b1), float(b2), float(eps), int(decoupled),
                                                      float(self.grad_scale), coef, _lib.stream_ptr(p.device)), "adam_step_groups")
                elif plan.whole:
                    _lib.check(L.r3m_adam_step(p.data_ptr(), g.data_ptr(), self._m[i].data_ptr(), self._v[i].data_ptr(), n, float(plan.lrs[0]),
                                               float(b1), float(b2), float(eps), self._steps[i], float(self.grad_scale),
                                               _lib.stream_ptr(p.device)), "adam_step")
                else:                          # some tensors frozen, or at other step counts: one launch over the ranges
                    _lib.check(L.r3m_adam_step_ranges(p.data_ptr(), g.data_ptr(), self._m[i].data_ptr(), self._v[i].data_ptr(),
                                                      _ll(plan.offs), _ll(plan.counts), _ll(plan.steps), len(plan.offs), float(plan.lrs[0]),
                                                      float(b1), float(b2), float(eps), float(self.grad_scale),
                                                      _lib.stream_ptr(p.device)), "adam_step_ranges")

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

    def state_dict(self):
        return {"step": self._steps[0], **super().state_dict()}

    def _saved_steps(self, sd):
        steps = sd.get("steps")           # round-1 snapshots carry one shared `step`
        return steps if steps is not None else [sd["step"]] * len(self.owners)


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW on the owners protocol: FusedAdam with decoupled weight decay and torch's default of 1e-2."""

    def __init__(self, owners, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, param_groups=None):
        super().__init__(owners, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=True,
                         max_grad_norm=max_grad_norm, param_groups=param_groups)


class FusedSGD(_FlatOptimizer):
    """torch.optim.SGD semantics (momentum, dampening, weight_decay, nesterov) as one HIP kernel per flat buffer. The reference
    only ever builds Adam (models_r3m.py:76); this is the plain alternative on the same owners protocol. param_groups (lr and
    weight_decay per group; momentum, dampening and nesterov are optimizer-wide) and max_grad_norm as in FusedAdam."""
    _name = "FusedSGD"
    _plain_weight_decay = True
    _moments = (("_buf", "momentum_buffer"),)
    _mismatch = ": the snapshot holds optimizer state for {k} flat buffer(s), this optimizer has {n} ({names})"
    _elements = ": the momentum buffer of owner {i} ({t}) has {k} elements, its parameters {n}"

    def __init__(self, owners, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, max_grad_norm=None,
                 param_groups=None):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        max_grad_norm=max_grad_norm)
        super().__init__(owners, defaults, param_groups, ("momentum", "dampening", "nesterov"))

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("FusedSGD.step(closure) is not supported")
        g0 = self.param_groups[0]
        L = _lib.lib()
        plans, coef = self._begin_step()
        for i, o, plan in plans:
            p = o.flat_params()
            g = o.flat_grads()
            if g0["momentum"] != 0 and (self._buf[i] is None or self._buf[i].device != p.device or self._buf[i].numel() != p.numel()):
                self._buf[i] = torch.zeros_like(p)
            buf_ptr = None if self._buf[i] is None else self._buf[i].data_ptr()
            with _lib.on(p):
                if plan.needs_groups(coef is not None, self._plain_weight_decay):
                    _lib.check(L.r3m_sgd_step_groups(p.data_ptr(), g.data_ptr(), buf_ptr, _ll(plan.offs), _ll(plan.counts), _ll(plan.steps),
                                                     _dd(plan.lrs), _dd(plan.wds), len(plan.offs), float(g0["momentum"]),
                                                     float(g0["dampening"]), int(bool(g0["nesterov"])), float(self.grad_scale), coef,
                                                     _lib.stream_ptr(p.device)), "sgd_step_groups")
                elif plan.whole:
                    _lib.check(L.r3m_sgd_step(p.data_ptr(), g.data_ptr(), buf_ptr, p.numel(), float(plan.lrs[0]), float(g0["momentum"]),
                                              float(g0["dampening"]), float(plan.wds[0]), int(bool(g0["nesterov"])),
                                              self._steps[i], float(self.grad_scale), _lib.stream_ptr(p.device)), "sgd_step")
                else:
                    _lib.check(L.r3m_sgd_step_ranges(p.data_ptr(), g.data_ptr(), buf_ptr, _ll(plan.offs), _ll(plan.counts), _ll(plan.steps),
                                                     len(plan.offs), float(plan.lrs[0]), float(g0["momentum"]), float(g0["dampening"]),
                                                     float(plan.wds[0]), int(bool(g0["nesterov"])), float(self.grad_scale),
                                                     _lib.stream_ptr(p.device)), "sgd_step_ranges")


# ---- group builders -------------------------------------------------------------------------------------------------------------
def _as_groups(module):
    if isinstance(module, torch.nn.Module):
        return [{"params": list(module.parameters())}]
    items = list(module)
    if all(isinstance(m, torch.nn.Module) for m in items):
        return [{"params": [p for m in items for p in m.parameters()]}]
    return [dict(g) for g in items]            # already parameter groups: each is split, its other keys kept


def no_decay_groups(module, weight_decay, **kw):
    """The usual "no weight decay on BatchNorm and biases" split: tensors with dim() >= 2 (convolution and linear weights) get
    `weight_decay`, 1-D tensors (BatchNorm affine, biases) get 0. `module` is a module (or several) -> two groups; or a list of
    parameter groups (layerwise_lr_groups) -> each split in two, keeping its other keys. `kw` (e.g. lr=) goes into every group.
    Empty groups are left out."""
    out = []
    for g in _as_groups(module):
        ps = list(g["params"])
        rest = {k: v for k, v in g.items() if k != "params"}
        for decay, sel in ((weight_decay, [p for p in ps if p.dim() >= 2]), (0.0, [p for p in ps if p.dim() < 2])):
            if sel:
                out.append({**rest, **kw, "params": sel, "weight_decay": decay})
    return out


def layerwise_lr_groups(convnet, lr, decay):
    """Layer-wise learning-rate decay over a ResNet encoder: five groups, the stem (conv1, bn1) and layer1..layer4, group k with
    lr * decay ** (4 - k): layer4 trains with `lr`, every stage below it `decay` times slower."""
    stages = [[] for _ in range(5)]
    for name, p in convnet.named_parameters():
        head = name.split(".", 1)[0]
        stages[int(head[5:]) if head.startswith("layer") and head[5:].isdigit() else 0].append(p)
    return [{"params": ps, "lr": lr * decay ** (4 - k)} for k, ps in enumerate(stages)]
