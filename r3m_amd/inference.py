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

RewardSession (below) puts the language reward behind such a session: R3M.reward_session().
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


class RewardSession:
    """The language-conditioned reward of R3M.get_reward, once per control step: the counterpart of InferenceSession for the head.

        rs = model.reward_session(obs_shape=[3, 224, 224])
        with torch.no_grad():
            rs.reset(first_frames, sentences_or_features)     # [E,3,H,W] and E sentences (or [E,768] features): e0 and le computed ONCE
            r, h = rs.step(frames)                            # [R,3,H,W] -> reward [R], embedding [R, outdim]; R == E, or any R when E == 1

    reset embeds the first frames through the encoder session and takes the sentence features from the model's LangEncoder
    (precomputed features, its cache, or its backend — one transformer pass at most; a native backend is asked for its few-row Linears
    for this call only). step runs the encoder session and ONE r3m_langrew_infer call (csrc/lang.hip): concat (which broadcasts the one
    first frame and instruction when E == 1), one ticket memset, the four hidden Linears on the few-row split-K kernel of
    csrc/conv_small.hip, the final GEMV. Nothing is kept for a backward.

    `encoder_session` is public: encoder_session.use_small_kernel = False gives the embedding of forward() bit for bit. On a bf16
    model the encoder session is bf16 and the head is fp32, as in get_reward.

    Freshness: the head's parameters are read live. e0 depends on the encoder, so reset records the encoder's epoch and step raises
    once it has moved (one integer comparison per step): call reset() again. No autograd, the errors of InferenceSession; no slot of the
    encoder's live-forward ring."""

    def __init__(self, model, obs_shape=(3, 224, 224)):
        if not getattr(model, "langweight", 0.0) > 0.0 or not hasattr(model, "lang_rew") or not hasattr(model, "lang_enc"):
            raise ValueError("RewardSession: this model has no language head (langweight == 0, or a model from load_r3m, which strips the "
                             "head for use as a visual representation); build R3M(..., langweight > 0) and load lang_rew's weights")
        self.model = model
        self.encoder_session = model.inference_session(obs_shape)
        self._e0 = self._le = None
        self._E = 0
        self._epoch = None
        self._ws = None

    def _check_grad(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.model.lang_rew.parameters())
                                        or any(p.requires_grad for p in self.model.convnet.parameters())):
            raise RuntimeError("RewardSession records no autograd graph: call it under torch.no_grad() with frozen inputs, or use "
                               "forward() and get_reward() for a differentiable pass")

    def reset(self, first_frames, sentences_or_features):
        """first_frames [E,3,H,W] in 0..255; E sentences, or [E, lang_dim] features"""
        self._check_grad(first_frames)
        head, enc = self.model.lang_rew, self.model.lang_enc
        e0 = self.encoder_session(first_frames)
        E = e0.shape[0]
        if torch.is_tensor(sentences_or_features):
            le = sentences_or_features
        else:
            was = enc.few_rows
            enc.few_rows = True                       # a native backend: its few-row Linears, for this call only
            try:
                le = enc(sentences_or_features)
            finally:
                enc.few_rows = was
        le = le.detach().to(device=e0.device, dtype=torch.float32).reshape(-1, head.lang_dim).contiguous()
        if le.shape[0] != E:
            raise ValueError(f"RewardSession.reset: {E} first frames and {le.shape[0]} instructions")
        self._e0, self._le, self._E = e0.contiguous(), le, E
        self._epoch = self.model.convnet._epoch
        return self

    def step(self, frames):
        """frames [R,3,H,W] in 0..255 -> (reward [R], embedding [R, outdim])"""
        if self._e0 is None:
            raise RuntimeError("RewardSession.step: call reset() with the first frames and the instructions first")
        if self.model.convnet._epoch != self._epoch:
            raise RuntimeError("RewardSession.step: the encoder's parameters or statistics were written since reset(); the cached first-frame "
                               "embedding is stale — call reset() again")
        self._check_grad(frames)
        head = self.model.lang_rew
        h = self.encoder_session(frames)
        R, E = h.shape[0], self._E
        if R != E and E != 1:
            raise ValueError(f"RewardSession.step: {R} frames against the {E} first frames of reset() (R must equal E, or E must be 1)")
        L = _lib.lib()
        D, H, LD = head.im_dim, head.hidden_dim, head.lang_dim
        need = L.r3m_langrew_infer_workspace_bytes(R, D, H, LD)
        if need == 0:
            raise ValueError(f"RewardSession.step: {_lib.last_error()}")
        self._ws = InferenceSession._grown(self._ws, need, h.device)
        score = torch.empty((R,), dtype=torch.float32, device=h.device)
        with _lib.on(h):
            _lib.check(L.r3m_langrew_infer(self._e0.data_ptr(), h.data_ptr(), self._le.data_ptr(), head.flat_params().data_ptr(),
                                           score.data_ptr(), self._ws.data_ptr(), self._ws.numel(), R, E, D, H, LD,
                                           _lib.stream_ptr(h.device)), "langrew_infer")
        return score, h
