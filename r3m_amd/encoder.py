"""ResNet-18/34/50 frame encoder on the HIP engine (libr3m_hip.so), behind an nn.Module that has the state-dict of
torchvision.models.resnet{18,34,50} with fc = Identity — what the reference builds at
/root/reference/r3m/models/models_r3m.py:44-52,62-63 and calls at :99.

Design (MI355X-first, not a translation of torchvision's module graph):
  * the network is ONE native plan in C++ (r3m_amd/csrc/engine.hip): forward and backward are single C calls that enqueue
    the whole kernel sequence on the current HIP stream; Python owns only memory (torch allocator) and autograd glue;
  * parameters are views into ONE flat fp32 buffer (torchvision order), gradients views into a second one (flat_grads.py keeps
    the rule for what it holds): the fused Adam step and the RCCL gradient all-reduce work on contiguous slices, no per-tensor
    loops, no bucket copies;
  * conv weights are logical OIHW tensors with channels_last strides == the OHWI image the kernels read, so
    load_state_dict()/state_dict() interchange with reference checkpoints needs no layout conversion.

There is no CPU or eager fallback: forward() on a non-CUDA tensor raises.
"""
import ctypes as C
import math

import weakref
import torch
import torch.nn as nn

from . import _lib
from .flat_grads import GradLedger, flat_view


class _Node(nn.Module):
    """Anonymous container: exists only so parameter names nest like torchvision's (layer1.0.downsample.0.weight)."""


def _tensor_table(size):
    """[(name, kind, offset, shape)] from the native plan (torchvision state-dict order)."""
    L = _lib.lib()
    h = L.r3m_resnet_create(size, 1)
    if not h:
        raise ValueError(_lib.last_error())
    try:
        out = []
        name = C.create_string_buffer(128)
        kind, ndim = C.c_int(), C.c_int()
        off = C.c_longlong()
        shape = (C.c_int * 4)()
        for i in range(L.r3m_resnet_num_tensors(h)):
            _lib.check(L.r3m_resnet_tensor_info(h, i, name, 128, C.byref(kind), C.byref(off), C.byref(ndim), shape), "tensor_info")
            out.append((name.value.decode(), kind.value, off.value, tuple(shape[k] for k in range(ndim.value))))
        return out, L.r3m_resnet_num_params(h), L.r3m_resnet_num_buffers(h), L.r3m_resnet_out_dim(h)
    finally:
        L.r3m_resnet_destroy(h)


FEATURE_LAYERS = ("layer1", "layer2", "layer3", "layer4")   # torchvision's stages: feature map k is convnet.layerk's output


class _EncoderFn(torch.autograd.Function):
    """h = encoder(x), or (h, *maps) with the stage outputs `layers` (indices into FEATURE_LAYERS) as fp32 NCHW tensors. Backward
    writes the gradients of the parameters that require grad straight into the module's flat gradient buffer (none when no parameter
    does) and returns d/dx when x requires grad."""

    @staticmethod
    def forward(ctx, x, anchor, module, training, crop, layers):
        if layers is not None:
            ctx.set_materialize_grads(False)     # an output the loss did not use arrives as None -> a null pointer, not a zero tensor
        h, maps, ctx.slot, ctx.generation = module._run_forward(x, training, crop, saved=True, layers=layers)
        ctx.module, ctx.layers = module, layers
        if 0 <= ctx.slot < len(module._ring):
            module._ring[ctx.slot].hold(ctx)
        return h if layers is None else (h,) + tuple(maps[k] for k in layers)

    @staticmethod
    def backward(ctx, dh, *dmaps):
        m = ctx.module
        # The data-parallel stage hook starts an ASYNC all-reduce on a slice of the flat gradient buffer. With several live forwards
        # ((h1 + h2).backward()) every backward accumulates into the same buffer, so only the LAST outstanding one may fire it: an
        # earlier one would hand RCCL a slice the next backward is still adding to. "Outstanding" = ring slots whose autograd node is
        # still alive and has not run (weak references: a forward whose graph was dropped — an eval call without no_grad, an
        # exception before backward — stops counting when its node is collected; round 5 kept a manual counter that such a forward
        # left raised for good, silently costing every later step its comm / compute overlap: ADVICE r5).
        others = sum(1 for sl in m._ring if sl.live and sl.waiting() is not ctx)
        grads = None
        if ctx.layers is not None:
            grads = [None] * 4
            for k, d in zip(ctx.layers, dmaps):
                if d is not None:
                    grads[k] = d.float().contiguous()
        dx = m._run_backward(None if dh is None else dh.contiguous(), ctx.generation, ctx.slot, fire_hooks=others == 0,
                             params=any(p.requires_grad for p in m.parameters()), input_grad=ctx.needs_input_grad[0], dmaps=grads)
        if 0 <= ctx.slot < len(m._ring):
            m._ring[ctx.slot].release(ctx)
        return dx, None, None, None, None, None


PRECISIONS = {"fp32": 0, "bf16": 1}   # R3M_DT_F32 / R3M_DT_BF16 (include/r3m_hip.h)


class _LiveSlot:
    """Saved state of one forward pass: native plans (per frame count; a plan also carries the staged-backward state), the HBM
    arena holding that forward's activations, and a generation counter that tells a late backward its activations are gone."""
    __slots__ = ("plans", "arena", "generation", "F", "hw", "waiting")

    def __init__(self):
        self.plans, self.arena, self.generation, self.F, self.hw = {}, None, 0, None, (224, 224)
        self.waiting = None      # weakref to the autograd node whose backward will read this slot's activations (None: nobody)

    @property
    def live(self):
        return self.waiting is not None and self.waiting() is not None

    def hold(self, node):
        """the slot stays live while autograd node `node` exists and has not run its backward: forwards that need no backward
        (no_grad / eval calls between a training forward and its backward) must not take it (_pick_slot)"""
        self.waiting = weakref.ref(node)

    def release(self, node):
        """node's backward has run; a slot that a later forward took over stays that forward's"""
        if self.waiting is not None and self.waiting() is node:
            self.waiting = None


def _pick_slot(live, pos, saved):
    """Which slot the next forward writes its activations to. live[i]: slot i holds a forward whose backward is still to come;
    pos: round-robin cursor; saved: this forward goes through autograd (a backward will read it). Returns (slot, new cursor);
    slot -1 = the scratch slot (forwards nobody differentiates, when every ring slot is live).
      * a free slot is always preferred (cursor order), so an inference call between a training forward and its backward never
        evicts the training forward;
      * a SAVED forward with every slot live evicts the oldest (the cursor): the evicted forward's backward raises and names the
        remedy (max_live_forwards) — unchanged behaviour;
      * an UNSAVED forward with every slot live runs in the scratch slot (its arena is allocated on first use and kept;
        HipResNet.release_scratch() hands the HBM back)."""
    k = len(live)
    order = [(pos + i) % k for i in range(k)]
    for i in order:
        if not live[i]:
            return i, ((i + 1) % k if saved else pos)
    if saved:
        return order[0], (order[0] + 1) % k
    return -1, pos


class HipResNet(nn.Module):
    """precision="fp32": everything fp32 (the reference's arithmetic). precision="bf16": activations and their gradients are
    stored in bf16 and the convolutions run on the bf16 MFMA with fp32 accumulation; parameters, their gradients, BatchNorm
    statistics and the output embedding stay fp32 (what torch.autocast(bfloat16) around the reference's encoder would do)."""

    def __init__(self, size, precision="fp32", max_live_forwards=1):
        """max_live_forwards: how many forward passes may be waiting for their backward at once. The reference module is a plain
        autograd graph (/root/reference/r3m/models/models_r3m.py:84-100): h1 = enc(x1); h2 = enc(x2); (h1 + h2).sum().backward()
        works there. Here a forward's saved activations live in ONE preallocated HBM arena per slot (141 GB for ResNet-50 fp32 at
        1280 frames), so the default of 1 — all `Trainer.update` needs — makes a second forward invalidate the first one's backward
        (it raises, it never computes on overwritten activations); k > 1 keeps a ring of k arenas + plans, forwards take them
        round-robin, and any k consecutive forwards can be backpropagated in any order."""
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"HipResNet: precision {precision!r} (expected one of {sorted(PRECISIONS)})")
        if int(max_live_forwards) < 1:
            raise ValueError("HipResNet: max_live_forwards must be >= 1")
        self.max_live_forwards = int(max_live_forwards)
        self.precision = precision
        table, n_params, n_buffers, out_dim = _tensor_table(size)
        self.size = size
        self.outdim = out_dim
        self._n_params = n_params
        self._n_buffers = n_buffers
        self._table = table
        self._slots = []        # (tensor, kind, offset, shape) in table order, for re-flattening
        flat_p = torch.zeros(n_params, dtype=torch.float32)
        flat_b = torch.zeros(n_buffers, dtype=torch.float32)
        n_bn = sum(1 for t in table if t[1] == 1)
        flat_nbt = torch.zeros(n_bn, dtype=torch.int64)
        bn_i = 0
        for name, kind, off, shape in table:
            parent, leaf = self._resolve(name)
            if kind <= 2:
                parent.register_parameter(leaf, nn.Parameter(flat_view(flat_p, off, shape)))
            else:
                parent.register_buffer(leaf, flat_view(flat_b, off, shape))
                if kind == 4:
                    parent.register_buffer("num_batches_tracked", flat_nbt[bn_i])
                    bn_i += 1
        self.fc = nn.Identity()   # models_r3m.py:62
        self._flat_p, self._flat_b, self._flat_nbt = flat_p, flat_b, flat_nbt
        # the flat gradient buffer and what it holds, per parameter tensor in flat-buffer order
        self._grads = GradLedger([(off, int(math.prod(shape))) for _, kind, off, shape in table if kind <= 2])
        self._ring = [_LiveSlot() for _ in range(self.max_live_forwards)]   # _plans / _arena below are slot 0's
        self._ring_pos = 0
        self._scratch = None          # _LiveSlot for forwards without a backward while every ring slot is live (_pick_slot)
        self._plan_masks = {}     # native handle -> the trainable mask it was last given (absent: all trainable, the plan's default)
        self._stage_hook = None   # callable(stage, offset, count) after each backward stage (data-parallel wrapper)
        self._epoch = 0           # moves whenever the project itself writes the flat buffers (params_written); InferenceSession compares it
        self.reset_parameters()

    @property
    def _plans(self):             # F -> native handle (slot 0)
        return self._ring[0].plans

    @_plans.setter
    def _plans(self, v):
        self._ring[0].plans = v

    @property
    def _arena(self):
        return self._ring[0].arena

    @_arena.setter
    def _arena(self, v):
        self._ring[0].arena = v

    @property
    def _flat_g(self):            # the flat gradient buffer, None until somebody asked for it (flat_grads)
        return self._grads.buffer

    def _drop_arenas(self):
        """release every slot's activation arena (re-flatten / device move)"""
        for sl in self._ring + ([self._scratch] if self._scratch is not None else []):
            sl.arena = None

    # ---- structure -------------------------------------------------------------------------------------------
    def _resolve(self, dotted):
        parts = dotted.split(".")
        mod = self
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, _Node())
            mod = mod._modules[p]
        return mod, parts[-1]

    def _named_slots(self):
        """(name, kind, offset, shape, tensor) following the native table."""
        sd_p = dict(self.named_parameters())
        sd_b = dict(self.named_buffers())
        for name, kind, off, shape in self._table:
            yield name, kind, off, shape, (sd_p[name] if kind <= 2 else sd_b[name])

    def reset_parameters(self):
        """torchvision ResNet init: kaiming_normal_(fan_out, relu) on convs, BN weight 1 / bias 0.
        Draws from the global torch RNG in state-dict order, like torchvision's `for m in self.modules()` loop."""
        with torch.no_grad():
            for name, kind, off, shape, t in self._named_slots():
                if kind == 0:
                    w = torch.empty(shape, dtype=torch.float32)
                    nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")
                    t.copy_(w)
                elif kind == 1 or kind == 4:
                    t.fill_(1.0)
                else:
                    t.zero_()
            self._flat_nbt.zero_()

    @property
    def _awaiting(self):
        """forwards through autograd whose backward has not run yet (see _EncoderFn.backward)"""
        return sum(1 for sl in self._ring if sl.live)

    # ---- flat storage ----------------------------------------------------------------------------------------
    def _is_flat(self):
        base = self._flat_p.data_ptr()
        dev = self._flat_p.device
        for name, kind, off, shape, t in self._named_slots():
            if kind <= 2 and (t.device != dev or t.data_ptr() != base + off * 4):
                return False
            if kind > 2 and (t.device != self._flat_b.device or t.data_ptr() != self._flat_b.data_ptr() + off * 4):
                return False
        return True

    def _reflatten(self):
        """Re-establish 'every tensor is a view of the flat buffers' after .to()/.cuda()/deepcopy/load with assign."""
        slots = list(self._named_slots())
        dev = slots[0][4].device
        for _, _, _, _, t in slots:
            if t.dtype != torch.float32:
                raise TypeError("r3m_amd.HipResNet keeps fp32 master parameters; dtype conversion is not supported")
        flat_p = torch.zeros(self._n_params, dtype=torch.float32, device=dev)
        flat_b = torch.zeros(self._n_buffers, dtype=torch.float32, device=dev)
        flat_nbt = torch.zeros_like(self._flat_nbt, device=dev)
        bn_i = 0
        with torch.no_grad():
            for name, kind, off, shape, t in slots:
                v = flat_view(flat_p if kind <= 2 else flat_b, off, shape)
                v.copy_(t)
                if kind <= 2:
                    t.data = v
                    t.grad = None
                else:
                    parent, leaf = self._resolve(name)
                    parent._buffers[leaf] = v
                    if kind == 4:
                        old = parent._buffers["num_batches_tracked"]
                        flat_nbt[bn_i] = old.to(dev)
                        parent._buffers["num_batches_tracked"] = flat_nbt[bn_i]
                        bn_i += 1
        self._flat_p, self._flat_b, self._flat_nbt = flat_p, flat_b, flat_nbt
        self._grads.drop()          # (every .grad was cleared above)
        self._drop_arenas()
        self.params_written()

    def _apply(self, fn, *a, **k):
        super()._apply(fn, *a, **k)
        self._reflatten()
        return self

    def params_written(self):
        """Every writer of the flat parameter / running-statistics buffers that the project owns calls this: the fused optimizers' steps,
        a train-mode forward, load_state_dict, _apply / re-flatten. What an InferenceSession derived from the buffers (eval-mode BatchNorm
        coefficients, the bf16 weight image) is rebuilt when the epoch has moved. Foreign writers (a raw in-place write through a
        parameter's .data, a hand-written optimizer) call it too, or InferenceSession.refresh()."""
        self._epoch += 1

    def _load_from_state_dict(self, *a, **k):
        # runs once per load_state_dict that reaches this module, called on it or on any parent (R3M, SingleDevice)
        super()._load_from_state_dict(*a, **k)
        self.params_written()

    def inference_session(self):
        """A low-latency frozen-encoder caller for one image or a handful of frames per call: see inference.InferenceSession."""
        from .inference import InferenceSession
        return InferenceSession(self)

    def flat_params(self):
        self._ensure()
        return self._flat_p

    def _params_in_order(self):
        """the parameter tensors in flat-buffer order (the order of param_ranges() / grads_written())"""
        return [t for _, kind, _, _, t in self._named_slots() if kind <= 2]

    def flat_grads(self):
        """The flat gradient buffer. `.grad` views into it are attached to the parameters that require grad (whoever fills the buffer
        by hand sees the values through them) or whose gradient a backward has written since zero_grad(); a frozen parameter's .grad
        stays None (unless the user left one there), as torch leaves it. Ranges no backward wrote hold zeros."""
        self._ensure()
        return self._grads.grads(self._flat_p, self._params_in_order)

    def param_ranges(self):
        """[(offset, count)] of every parameter tensor in the flat buffers, ascending and gap-free (optimizers: the units that can be
        frozen one by one)"""
        return self._grads.ranges

    def grads_written(self):
        """per param_ranges() entry: a backward wrote this tensor's gradient since zero_grad() (torch: `p.grad is not None` after
        zero_grad(set_to_none=True))"""
        return self._grads.written

    def _ensure(self):
        if not self._is_flat():
            self._reflatten()

    def mark_grads_stale(self):
        """Called by the optimizer's zero_grad(): the next backward overwrites instead of accumulating, and until one arrives no
        parameter has a gradient."""
        self._grads.mark_stale()

    def _send_trainable(self, h, req):
        """Before stage 0 of a backward that writes parameter gradients: hand plan h the trainable mask (req: requires_grad of every
        parameter, flat-buffer order) when it changed. Returns whether some tensor is frozen."""
        mask = None
        if not all(req):
            it = iter(req)
            mask = bytes((1 if next(it) else 0) if kind <= 2 else 0 for _, kind, _, _ in self._table)
        if self._plan_masks.get(h) != mask:
            _lib.check(_lib.lib().r3m_resnet_set_trainable(h, mask, 0 if mask is None else len(mask)), "resnet_set_trainable")
            if mask is None:
                self._plan_masks.pop(h, None)
            else:
                self._plan_masks[h] = mask
        return mask is not None

    def stage_range(self, stage):
        L = _lib.lib()
        h = self._plan(1)
        off, cnt = C.c_longlong(), C.c_longlong()
        _lib.check(L.r3m_resnet_stage_range(h, stage, C.byref(off), C.byref(cnt)), "stage_range")
        return off.value, cnt.value

    # ---- execution -------------------------------------------------------------------------------------------
    def _slot(self, si):
        if si >= 0:
            return self._ring[si]
        if self._scratch is None:
            self._scratch = _LiveSlot()
        return self._scratch

    def release_scratch(self):
        """Drop the scratch arena (HBM held by no_grad forwards that ran while every saved forward was still awaiting its backward)."""
        if self._scratch is not None:
            self._scratch.arena = None

    def _plan(self, F, slot=0, hw=(224, 224)):
        """the slot's native plan for F frames of hw = (H, W); cached under F for 224 x 224 frames, under (F, H, W) otherwise"""
        plans = self._slot(slot).plans
        hw = (int(hw[0]), int(hw[1]))
        key = F if hw == (224, 224) else (F,) + hw
        h = plans.get(key)
        if h is None:
            if hw == (224, 224):
                h = _lib.lib().r3m_resnet_create_dt(self.size, F, PRECISIONS[self.precision])
                if not h:
                    raise RuntimeError(_lib.last_error())
            else:
                h = _lib.lib().r3m_resnet_create_hw(self.size, F, PRECISIONS[self.precision], hw[0], hw[1])
                if not h:
                    raise ValueError(f"r3m_amd: {F} frames of {hw[0]}x{hw[1]}: {_lib.last_error()}")
            plans[key] = h
        return h

    _HW_OK = set()

    @classmethod
    def check_input_hw(cls, H, W):
        """ValueError with the engine's message when no plan takes [F,3,H,W] frames (sizes outside 32..512). Checked before a forward
        takes a ring slot, so a refused size never evicts a live forward."""
        hw = (int(H), int(W))
        if hw in cls._HW_OK:
            return
        L = _lib.lib()
        h = L.r3m_resnet_create_hw(18, 1, 0, hw[0], hw[1])
        if not h:
            raise ValueError(f"r3m_amd: frames of {hw[0]}x{hw[1]}: {_lib.last_error()}")
        L.r3m_resnet_destroy(h)
        cls._HW_OK.add(hw)

    def __del__(self):
        try:
            L = _lib.lib()
            for sl in self._ring + ([self._scratch] if self._scratch is not None else []):
                for h in sl.plans.values():
                    L.r3m_resnet_destroy(h)
        except Exception:
            pass

    def __getstate__(self):
        """copy.deepcopy / pickle: native plan handles, the activation arena, the flat gradient buffer and the data-parallel
        hook belong to THIS object (a copied integer handle would be destroyed twice); the copy re-creates them lazily. The
        reference R3M deep-copies cleanly (plain nn.Module), so must this."""
        st = self.__dict__.copy()
        st.update(_ring=[_LiveSlot() for _ in self._ring], _ring_pos=0, _scratch=None, _stage_hook=None, _plan_masks={},
                  _grads=GradLedger(self._grads.ranges))
        return st

    def __setstate__(self, st):
        super().__setstate__(st)
        for p in self.parameters():      # gradients were views of the dropped flat buffer
            p.grad = None

    def _run_forward(self, x, training, crop=None, saved=False, layers=None):
        """x: [F,3,H,W] fp32 frames, or None with crop = augment.CroppedClips (raw clips + boxes, resampled in the stem pre-pass).
        saved: the call comes from autograd (_EncoderFn) and a backward will read this forward's activations.
        layers: the stage outputs wanted as well (indices 0..3 = layer1..layer4; frames only), or None.
        Returns (h, {index: [F,C,H,W] fp32} or None, slot, the slot's generation)."""
        L = _lib.lib()
        src = crop.raw if crop is not None else x
        F = src.shape[0]
        hw = (224, 224) if crop is not None else (x.shape[2], x.shape[3])
        si, pos = _pick_slot([sl.live for sl in self._ring], self._ring_pos, saved)
        h = self._plan(F, si, hw)                        # a refused (F, H, W) raises here, before the slot's live forward is dropped
        self._ring_pos = pos
        slot = self._slot(si)
        slot.waiting = None                              # whatever forward was saved here is gone now
        need = L.r3m_resnet_arena_bytes(h)
        if slot.arena is None or slot.arena.numel() < need or slot.arena.device != src.device:
            slot.arena = None   # release first: the arena is the dominant HBM allocation
            slot.arena = torch.empty(need, dtype=torch.uint8, device=src.device)
        arena = slot.arena
        out = torch.empty((F, self.outdim), dtype=torch.float32, device=src.device)
        # 1 train / 0 eval with the activations kept for a backward / 2 inference: eval statistics and nothing kept — BatchNorm, residual
        # join and ReLU ride in the convolutions' stores (what load_r3m(...).eval() under no_grad runs, /root/reference/r3m/__init__.py:72-75)
        mode = 1 if training else (0 if saved else 2)
        maps = ptrs = None
        with _lib.on(src):
            if crop is not None:
                _lib.check(L.r3m_resnet_forward_crop(h, crop.raw.data_ptr(), 1 if crop.raw.dtype == torch.uint8 else 0,
                                                     crop.boxes.data_ptr(), crop.frames_per_box, crop.raw.shape[-2], crop.raw.shape[-1],
                                                     self._flat_p.data_ptr(), self._flat_b.data_ptr(), arena.data_ptr(),
                                                     out.data_ptr(), mode, _lib.stream_ptr(src.device)),
                           "resnet_forward_crop")
            else:
                if layers is not None:
                    maps = {k: torch.empty((F,) + self._feature_shape(h, k), dtype=torch.float32, device=x.device) for k in layers}
                    ptrs = (C.c_void_p * 4)(*[_lib.ptr(maps.get(k)) for k in range(4)])
                _lib.check(L.r3m_resnet_forward_features(h, x.data_ptr(), self._flat_p.data_ptr(), self._flat_b.data_ptr(),
                                                         arena.data_ptr(), out.data_ptr(), ptrs, mode, _lib.stream_ptr(x.device)),
                           "resnet_forward_features")
        if training:
            self._flat_nbt += 1
            self.params_written()       # the running statistics moved
        slot.generation += 1
        slot.F, slot.hw = F, hw
        return out, maps, si, slot.generation

    def _run_backward(self, dh, generation, si, fire_hooks, params, input_grad, dmaps=None):
        """dh: gradient of the embedding, or None when the loss did not use it (then dmaps has an entry: zeros flow down from the
        pool instead of a zero tensor through a kernel). dmaps: [4] gradients of the stage outputs (fp32 NCHW, None = none), or None.
        params: write the gradients of the parameters that require grad into the flat gradient buffer (False: frozen encoder — no
        weight-gradient launch, the buffer is neither created nor touched, no stage hook fires). With some parameters frozen the
        engine runs only what the trainable ones (and the input gradient) need; all four stage hooks still fire, in order.
        input_grad: return d/d(frames) [F,3,H,W] fp32."""
        slot = self._slot(si)
        if generation != slot.generation or slot.arena is None:
            raise RuntimeError(f"r3m_amd: the encoder ran {len(self._ring)} other forward(s) before this backward; its saved "
                               f"activations (one HBM arena per live forward) were overwritten. Construct the encoder with "
                               f"max_live_forwards=k (R3M(..., max_live_forwards=k)) to keep k forwards alive at once")
        L = _lib.lib()
        h = self._plan(slot.F, si, slot.hw)
        g, accumulate, partial = None, 0, False
        if params:
            g = self.flat_grads()
            ps = self._params_in_order()
            req = [t.requires_grad for t in ps]
            partial = self._send_trainable(h, req)
            accumulate = self._grads.begin(ps, req)
        lead = dh if dh is not None else next(d for d in dmaps if d is not None)
        dev = lead.device
        dx = torch.empty((slot.F, 3) + tuple(slot.hw), dtype=torch.float32, device=dev) if input_grad else None
        if dmaps is not None:                        # every stage carries the same array; the stage that owns an entry reads it
            dmaps = (C.c_void_p * 4)(*[_lib.ptr(d) for d in dmaps])
        with _lib.on(lead):
            for stage in range(4):
                _lib.check(L.r3m_resnet_backward_features(h, _lib.ptr(dh), dmaps, self._flat_p.data_ptr(), _lib.ptr(g),
                                                          slot.arena.data_ptr(), stage, stage + 1, accumulate,
                                                          # (frozen tensors: stage 0 plans the backward and must know dx is wanted)
                                                          _lib.ptr(dx) if stage == 3 or partial else None, 0,
                                                          _lib.stream_ptr(dev)), "resnet_backward_features")
                if g is not None and self._stage_hook is not None and fire_hooks:
                    off, cnt = self.stage_range(stage)
                    self._stage_hook(stage, off, cnt)
        if g is not None:
            self._grads.finish()
        return dx

    @staticmethod
    def _feature_shape(h, k):
        """(C, H, W) of stage output k (0..3 = layer1..layer4) of native plan h"""
        c, hh, ww = C.c_int(), C.c_int(), C.c_int()
        _lib.check(_lib.lib().r3m_resnet_feature_info(h, k + 1, C.byref(c), C.byref(hh), C.byref(ww)), "resnet_feature_info")
        return c.value, hh.value, ww.value

    def forward_features(self, x, layers=FEATURE_LAYERS):
        """forward(x) plus the spatial feature maps: returns (h, {name: [F, C_k, H_k, W_k] fp32 NCHW}) for the requested `layers`
        (names out of layer1..layer4) — the outputs of torchvision's convnet.layerk, what a forward hook on the reference's
        convnet.layer4 or nn.Sequential(*list(convnet.children())[:-2]) gives (models_r3m.py:44-52). Differentiable like forward():
        a loss on any mix of h and the maps backpropagates into the parameters that require grad and into x. Train, eval with grad,
        and no_grad inference; both precisions (bf16 maps are the stored activations widened, exactly). x as for forward(), except
        that CroppedClips input is not supported."""
        layers = tuple(layers)
        for i, name in enumerate(layers):
            if name not in FEATURE_LAYERS:
                raise ValueError(f"forward_features: unknown layer {name!r} (expected names out of {FEATURE_LAYERS})")
            if name in layers[:i]:
                raise ValueError(f"forward_features: layer {name!r} requested twice")
        from .augment import CroppedClips
        if isinstance(x, CroppedClips):
            raise TypeError("forward_features: CroppedClips input is not supported (the crop-fed forward exports no feature maps); "
                            "resample the clips first and pass [F,3,H,W] frames")
        x, _ = self._prepare_frames(x)
        idx = tuple(FEATURE_LAYERS.index(name) for name in layers)
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or x.requires_grad):
            h, *maps = _EncoderFn.apply(x, self._anchor(), self, self.training, None, idx)
        else:
            h, got, _, _ = self._run_forward(x, self.training, layers=idx)
            maps = [got[k] for k in idx]
        return h, dict(zip(layers, maps))

    def _prepare_frames(self, x):
        """What every forward starts with: refuse what the engine cannot take, re-flatten if needed, coerce. x: [F,3,H,W] frames or
        augment.CroppedClips. Returns (contiguous fp32 frames, None) or (None, the clips)."""
        if not x.is_cuda:
            raise RuntimeError("r3m_amd: the encoder runs on MI355X through libr3m_hip.so only; got a CPU tensor "
                               "(no CPU / eager fallback exists — the CPU oracle lives under oracle/ for tests)")
        from .augment import CroppedClips
        crop = isinstance(x, CroppedClips)
        if crop:
            if tuple(x.out_hw) != (224, 224):
                raise ValueError(f"CroppedClips must resample to 224x224, got {x.out_hw}")
        else:
            if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1:
                raise ValueError(f"expected [F,3,H,W] frames, got {tuple(x.shape)}")
            if tuple(x.shape[2:]) != (224, 224):
                self.check_input_hw(x.shape[2], x.shape[3])
        self._ensure()
        if self._flat_p.device != x.device:
            raise RuntimeError(f"encoder parameters on {self._flat_p.device}, input on {x.device}")
        return (None, x) if crop else (x.contiguous().float(), None)

    def _anchor(self):
        """what makes autograd record the node: a parameter that requires grad, when there is one — the first may be frozen"""
        p = next((p for p in self.parameters() if p.requires_grad), None)
        return p if p is not None else next(self.parameters())

    def forward(self, x):
        """x: [F,3,H,W] float32 CUDA tensor with values in 0..255, any H and W in 32..512 (torchvision's ResNet takes any size; 224 x 224
        runs the specialised stem kernels, other sizes the general ones). The /255 and Normalize of R3M.forward are fused into the stem
        kernel. Returns [F, outdim]."""
        x, crop = self._prepare_frames(x)
        # a graph is recorded when anything upstream wants a gradient: the parameters (training) or the frames (obs.grad: the
        # encoder as a differentiable reward / perceptual loss, parameters frozen or not)
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or (crop is None and x.requires_grad)):
            return _EncoderFn.apply(x, self._anchor(), self, self.training, crop, None)
        return self._run_forward(x, self.training, crop)[0]
