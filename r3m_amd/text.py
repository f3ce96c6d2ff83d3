"""DistilBERT forward on the HIP path (csrc/text.hip, C ABI r3m_text_*): the frozen text model behind LangEncoder
(the reference's r3m/models/models_language.py:13-35) without transformers or eager torch on the device.

    HipDistilBert.from_state_dict(sd, n_heads, device)      HuggingFace names, bare or with a `distilbert.` prefix
    HipDistilBert.from_hf(model, device)                    from a transformers.DistilBertModel
    .features(input_ids, attention_mask, mask_padding=False, few_rows=False) -> [B, dim]   pooled on the device
                                                            few_rows: the Linears of few B * T rows on the split-K kernel
    .__call__(input_ids, attention_mask=None).last_hidden_state            drops into LangEncoder.use_backend

Inference only, fp32, no dropout; the tokenizer stays on the host."""
import ctypes as C
from types import SimpleNamespace

import torch

from . import _lib

MAX_TOKENS = 128      # the attention kernel's limit (include/r3m_hip.h)


def _dims6(dims):
    return (C.c_int * 6)(*dims)


def tensor_table(dims):
    """[(name, offset, count, shape)] of the flat parameter buffer for dims = (vocab, max_pos, dim, n_layers, n_heads, ffn_dim)."""
    L = _lib.lib()
    d = _dims6(dims)
    n = L.r3m_text_num_tensors(d)
    if n < 0:
        raise ValueError(f"r3m_amd.text: {_lib.last_error()}")
    out = []
    name = C.create_string_buffer(128)
    off, cnt, nd, shape = C.c_longlong(), C.c_longlong(), C.c_int(), (C.c_int * 2)()
    for i in range(n):
        _lib.check(L.r3m_text_tensor_info(d, i, name, 128, C.byref(off), C.byref(cnt), C.byref(nd), shape), "text_tensor_info")
        out.append((name.value.decode(), off.value, cnt.value, tuple(shape[:nd.value])))
    return out


class HipDistilBert:
    """One flat fp32 device buffer and the six ints that describe it. Not an nn.Module: frozen, no parameters to register."""

    def __init__(self, dims, params):
        self.dims = tuple(int(v) for v in dims)
        self.vocab, self.max_pos, self.dim, self.n_layers, self.n_heads, self.ffn_dim = self.dims
        self.params = params              # flat fp32, requires_grad False
        self.device = params.device
        self.launches_per_call = 2 + 8 * self.n_layers
        self._dims_c = _dims6(self.dims)
        self._ws = {}                     # (B, T, few_rows) -> (workspace tensor, bytes)

    # ---- construction ----
    @classmethod
    def from_state_dict(cls, sd, n_heads, device):
        if torch.device(device).type != "cuda":
            raise RuntimeError("r3m_amd.text.HipDistilBert runs on the HIP path only (no CPU fallback)")
        sd = {k: torch.as_tensor(v) for k, v in sd.items()}          # tensors, or numpy arrays
        sd = {(k[len("distilbert."):] if k.startswith("distilbert.") else k): v for k, v in sd.items() if v.is_floating_point()}
        try:
            vocab, dim = sd["embeddings.word_embeddings.weight"].shape
            max_pos = sd["embeddings.position_embeddings.weight"].shape[0]
            ffn = sd["transformer.layer.0.ffn.lin1.weight"].shape[0]
        except KeyError as e:
            raise ValueError(f"HipDistilBert.from_state_dict: not a DistilBERT state dict (no {e.args[0]})") from None
        n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.layer."))
        dims = (int(vocab), int(max_pos), int(dim), n_layers, int(n_heads), int(ffn))
        L = _lib.lib()
        n = L.r3m_text_num_params(_dims6(dims))
        if n < 0:
            raise ValueError(f"HipDistilBert.from_state_dict: {_lib.last_error()}")
        flat = torch.empty(n, dtype=torch.float32)
        for name, off, cnt, shape in tensor_table(dims):
            if name not in sd:
                raise ValueError(f"HipDistilBert.from_state_dict: the state dict has no {name}")
            if tuple(sd[name].shape) != shape:
                raise ValueError(f"HipDistilBert.from_state_dict: {name} is {tuple(sd[name].shape)}, expected {shape}")
            flat[off:off + cnt].view(shape).copy_(sd[name].detach())
        return cls(dims, flat.to(device).requires_grad_(False))

    @classmethod
    def from_hf(cls, model, device):
        return cls.from_state_dict(model.state_dict(), model.config.n_heads, device)

    # ---- compute ----
    def _upload(self, input_ids, attention_mask):
        ids = torch.as_tensor(input_ids)
        if ids.dim() != 2:
            raise ValueError(f"HipDistilBert: input_ids must be [B, T], got {tuple(ids.shape)}")
        B, T = ids.shape
        if T > MAX_TOKENS:
            raise ValueError(f"HipDistilBert: T={T} tokens, the HIP path supports at most {MAX_TOKENS}")
        if T > self.max_pos:
            raise ValueError(f"HipDistilBert: T={T} tokens, the model has max_pos={self.max_pos} positions")
        mask = torch.ones_like(ids) if attention_mask is None else torch.as_tensor(attention_mask)
        if mask.shape != ids.shape:
            raise ValueError(f"HipDistilBert: attention_mask {tuple(mask.shape)} does not match input_ids {tuple(ids.shape)}")
        if not ids.is_cuda:               # the usual case: a tokenizer's host tensors; validated before the upload
            if B * T and (int(ids.min()) < 0 or int(ids.max()) >= self.vocab):
                raise ValueError(f"HipDistilBert: token ids must lie in [0, {self.vocab}), got {int(ids.min())}..{int(ids.max())}")
        if self.device.type != "cuda":
            raise RuntimeError("r3m_amd.text.HipDistilBert runs on the HIP path only (no CPU fallback)")
        ids = _lib.upload_small(ids, self.device, torch.int32).contiguous()
        mask = _lib.upload_small(mask, self.device, torch.int32).contiguous()
        return ids, mask, B, T

    def _forward(self, input_ids, attention_mask, pool, want_hidden, few_rows=False):
        L = _lib.lib()
        ids, mask, B, T = self._upload(input_ids, attention_mask)
        few_rows = bool(few_rows)
        key = (B, T, few_rows)
        if key not in self._ws:
            nbytes = (L.r3m_text_small_workspace_bytes if few_rows else L.r3m_text_workspace_bytes)(self._dims_c, B, T)
            if nbytes == 0:
                raise ValueError(f"HipDistilBert: {_lib.last_error()}")
            self._ws[key] = (torch.empty(nbytes, dtype=torch.uint8, device=self.device), nbytes)
        ws, nbytes = self._ws[key]
        run, what = (L.r3m_text_forward_small, "text_forward_small") if few_rows else (L.r3m_text_forward, "text_forward")
        feats = torch.empty((B, self.dim), dtype=torch.float32, device=self.device)
        hidden = torch.empty((B, T, self.dim), dtype=torch.float32, device=self.device) if want_hidden else None
        with _lib.on(self.params):
            _lib.check(run(ids.data_ptr(), mask.data_ptr(), self.params.data_ptr(), feats.data_ptr(), _lib.ptr(hidden), ws.data_ptr(), nbytes,
                           B, T, self._dims_c, int(pool), _lib.stream_ptr(self.device)), what)
        return feats, hidden

    def features(self, input_ids, attention_mask, mask_padding=False, few_rows=False):
        """[B, dim] sentence features: the mean of the last hidden state over ALL positions (the reference, padding included), or
        with mask_padding over the positions with attention_mask != 0. few_rows: r3m_text_forward_small, which runs every Linear that
        the few-row plan takes at B * T rows on the split-K kernel of csrc/conv_small.hip (same arithmetic per product, another
        summation order: results agree to fp32 rounding, not bit for bit)."""
        return self._forward(input_ids, attention_mask, 1 if mask_padding else 0, False, few_rows)[0]

    def hidden_and_pools(self, input_ids, attention_mask, mask_padding=False, few_rows=False):
        """(last hidden state [B,T,dim], features [B,dim]) of ONE call (tests, parity reports)"""
        feats, hidden = self._forward(input_ids, attention_mask, 1 if mask_padding else 0, True, few_rows)
        return hidden, feats

    def __call__(self, input_ids, attention_mask=None):
        return SimpleNamespace(last_hidden_state=self._forward(input_ids, attention_mask, 0, True)[1])

    # the slice of nn.Module's surface LangEncoder.use_backend touches: already on its device, always in eval mode, nothing to freeze
    def to(self, device):
        if torch.device(device).type != "cuda":
            raise RuntimeError("r3m_amd.text.HipDistilBert runs on the HIP path only (no CPU fallback)")
        if torch.device(device) != self.device and torch.device(device).index is not None:
            return HipDistilBert(self.dims, self.params.to(device))
        return self

    def eval(self):
        return self

    def parameters(self):
        return iter(())
