"""InferenceSession: the frozen encoder on one image or a handful of frames per call (a policy's visual features, a language reward,
a perceptual loss: what /root/reference/r3m/example.py:19-33 does with ONE image).

`HipResNet.forward` under no_grad recomputes per call what only changes with the parameters: the eval-mode BatchNorm coefficients of
every layer (one launch per convolution) and, on a bf16 encoder, the bf16 image of all weights. A session keeps both in its own arena
(r3m_resnet_inference_prepare, one launch) and runs r3m_resnet_forward_prepared, which on fp32 encoders also sends the convolutions of few
GEMM rows to the split-K kernel of csrc/conv_small.hip.

    sess = encoder.inference_session()          # or R3M.inference_session(obs_shape), load_r3m(...).inference_session()
    with torch.no_grad():
        h = sess(frames)                        # [F,3,H,W] in 0..255 -> [F, outdim]

Freshness: the fp32 weights are read live. What the session derived from the flat buffers is rebuilt when the encoder's integer epoch
has moved since the last call; every writer the project owns moves it (FusedAdam / FusedSGD steps, a train-mode forward,
load_state_dict, .to() / re-flatten). Anybody else who writes parameters or running statistics in place calls sess.refresh() (or
encoder.params_written()); until then the session keeps answering from the old coefficients. The check is one integer comparison per
call.

The session owns its plans (one per (F, H, W), created lazily), ONE arena and ONE split-K workspace, each grown to the largest need;
it takes no slot of the encoder's live-forward ring and touches no forward saved for a backward. No autograd: inputs or parameters that
require grad under enabled grad raise.
"""
import ctypes as C

import torch

from . import _lib
from .encoder import FEATURE_LAYERS, PRECISIONS


class InferenceSession:
    def __init__(self, encoder, resize=False):
        self.encoder = encoder
        self.resize = bool(resize)      # Resize(256) + CenterCrop(224) in front (R3M.forward with another obs_shape)
        self.use_small_kernel = True    # False: every convolution runs the kernel HipResNet.forward runs (bit-identical results)
        self._plans = {}                # (F, H, W) -> native handle
        self._arena = None
        self._workspace = None
        self._ready = None              # (handle, epoch, arena pointer, flat parameter pointer) of the last preparation
        self.prepares = 0               # how often the coefficients were (re)built

    def refresh(self):
        """the parameters or running statistics were written by somebody the encoder's epoch does not see: prepare again at the next call"""
        self._ready = None

    def __del__(self):
        try:
            L = _lib.lib()
            for h in self._plans.values():
                L.r3m_resnet_destroy(h)
        except Exception:
            pass

    def _plan(self, F, H, W):
        key = (int(F), int(H), int(W))
        h = self._plans.get(key)
        if h is None:
            enc = self.encoder
            h = _lib.lib().r3m_resnet_create_hw(enc.size, key[0], PRECISIONS[enc.precision], key[1], key[2])
            if not h:
                raise ValueError(f"r3m_amd: {F} frames of {H}x{W}: {_lib.last_error()}")
            self._plans[key] = h
        return h

    @staticmethod
    def _grown(buf, need, device):
        if need <= 0:
            return buf
        if buf is None or buf.numel() < need or buf.device != device:
            buf = None                  # release first
            buf = torch.empty(need, dtype=torch.uint8, device=device)
        return buf

    def _run(self, x, layers):
        enc = self.encoder
        from .augment import CroppedClips
        if isinstance(x, CroppedClips):
            raise TypeError("InferenceSession: CroppedClips input is not supported; resample the clips first and pass [F,3,H,W] frames")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in enc.parameters())):
            raise RuntimeError("InferenceSession records no autograd graph: call it under torch.no_grad() with frozen inputs, or use "
                               "forward() for a differentiable pass")
        if self.resize:
            from .augment import resize_center_crop
            x = resize_center_crop(x.reshape(-1, *x.shape[-3:]))
        x, _ = enc._prepare_frames(x)
        L = _lib.lib()
        F, H, W = x.shape[0], x.shape[2], x.shape[3]
        h = self._plan(F, H, W)
        dev = x.device
        self._arena = self._grown(self._arena, L.r3m_resnet_arena_bytes(h), dev)
        self._workspace = self._grown(self._workspace, L.r3m_resnet_inference_workspace_bytes(h), dev)
        out = torch.empty((F, enc.outdim), dtype=torch.float32, device=dev)
        maps = ptrs = None
        if layers is not None:
            maps = {k: torch.empty((F,) + enc._feature_shape(h, k), dtype=torch.float32, device=dev) for k in layers}
            ptrs = (C.c_void_p * 4)(*[_lib.ptr(maps.get(k)) for k in range(4)])
        stamp = (h, enc._epoch, self._arena.data_ptr(), enc._flat_p.data_ptr())
        with _lib.on(x):
            st = _lib.stream_ptr(dev)
            if self._ready != stamp:    # another plan laid the arena out differently, or the buffers were written since
                _lib.check(L.r3m_resnet_inference_prepare(h, enc._flat_p.data_ptr(), enc._flat_b.data_ptr(), self._arena.data_ptr(), st),
                           "resnet_inference_prepare")
                self._ready = stamp
                self.prepares += 1
            _lib.check(L.r3m_resnet_forward_prepared(h, x.data_ptr(), enc._flat_p.data_ptr(), self._arena.data_ptr(),
                                                     _lib.ptr(self._workspace), out.data_ptr(), ptrs, 0 if self.use_small_kernel else 1, st),
                       "resnet_forward_prepared")
        return out, maps

    def __call__(self, x):
        """x: [F,3,H,W] frames in 0..255 on the encoder's device -> [F, outdim]"""
        return self._run(x, None)[0]

    def forward_features(self, x, layers=FEATURE_LAYERS):
        """-> (h, {name: [F, C_k, H_k, W_k] fp32 NCHW}) as HipResNet.forward_features, without autograd"""
        layers = tuple(layers)
        for i, name in enumerate(layers):
            if name not in FEATURE_LAYERS:
                raise ValueError(f"forward_features: unknown layer {name!r} (expected names out of {FEATURE_LAYERS})")
            if name in layers[:i]:
                raise ValueError(f"forward_features: layer {name!r} requested twice")
        idx = tuple(FEATURE_LAYERS.index(name) for name in layers)
        h, got = self._run(x, idx)
        return h, {name: got[k] for name, k in zip(layers, idx)}
