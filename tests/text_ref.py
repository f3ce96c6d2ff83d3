"""Shared by the text tests: a numpy restatement of the DistilBERT forward (HuggingFace DistilBertModel in eval mode, as the
reference's LangEncoder runs it, r3m/models/models_language.py:29-34) and detgen-built weights under HuggingFace's
tensor names. Needs neither transformers nor a GPU. Evaluated in float64 it is the reference of the GPU tests; evaluated in float32
it is their witness: what a plain fp32 implementation of the same formulas loses against float64 on the same case."""
import math

import numpy as np

from oracle import detgen

G7_DIMS = dict(vocab=59, max_pos=32, dim=768, n_layers=1, n_heads=4, ffn=256)     # oracle/tiny_text.py


def tensor_shapes(vocab, max_pos, dim, n_layers, ffn):
    """(name, shape) in HuggingFace's state-dict order."""
    out = [("embeddings.word_embeddings.weight", (vocab, dim)), ("embeddings.position_embeddings.weight", (max_pos, dim)),
           ("embeddings.LayerNorm.weight", (dim,)), ("embeddings.LayerNorm.bias", (dim,))]
    for l in range(n_layers):
        p = f"transformer.layer.{l}."
        for lin in ("q_lin", "k_lin", "v_lin", "out_lin"):
            out += [(p + f"attention.{lin}.weight", (dim, dim)), (p + f"attention.{lin}.bias", (dim,))]
        out += [(p + "sa_layer_norm.weight", (dim,)), (p + "sa_layer_norm.bias", (dim,)),
                (p + "ffn.lin1.weight", (ffn, dim)), (p + "ffn.lin1.bias", (ffn,)),
                (p + "ffn.lin2.weight", (dim, ffn)), (p + "ffn.lin2.bias", (dim,)),
                (p + "output_layer_norm.weight", (dim,)), (p + "output_layer_norm.bias", (dim,))]
    return out


def detgen_state_dict(tag, vocab, max_pos, dim, n_layers, ffn, **_):
    """{name: float32 array}: LayerNorm gains in 0.8..1.2, everything else in -0.08..0.08 (the rule of oracle/tiny_text.py; tag "tt"
    with G7_DIMS gives tiny_text.tiny_distilbert()'s weights)."""
    sd = {}
    for name, shape in tensor_shapes(vocab, max_pos, dim, n_layers, ffn):
        gain = name.endswith("LayerNorm.weight") or name.endswith("layer_norm.weight")
        sd[name] = detgen.uniform(tag + name, shape, *((0.8, 1.2) if gain else (-0.08, 0.08)))
    return sd


def g7_state_dict():
    return detgen_state_dict("tt", **G7_DIMS)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def layernorm(x, gamma, beta, eps=1e-12):
    mean = x.mean(-1, keepdims=True, dtype=x.dtype)
    var = ((x - mean) ** 2).mean(-1, keepdims=True, dtype=x.dtype)
    return (x - mean) / np.sqrt(var + x.dtype.type(eps)) * gamma + beta


def gelu(x):
    """exact erf form; erf itself is evaluated in float64 and rounded to x's type (a correctly rounded erf)"""
    return (x * x.dtype.type(0.5) * (x.dtype.type(1.0) + _erf(x.astype(np.float64) / math.sqrt(2.0)).astype(x.dtype)))


def attention(q, k, v, mask, n_heads):
    """q, k, v [B,T,dim], mask [B,T] -> [B,T,dim]. Keys with mask == 0 score the most negative finite number of the working type;
    every query row, padded ones included, is computed."""
    B, T, dim = q.shape
    hd = dim // n_heads
    dt = q.dtype

    def heads(x):
        return x.reshape(B, T, n_heads, hd).transpose(0, 2, 1, 3)
    s = np.matmul(heads(q), heads(k).transpose(0, 1, 3, 2)) / dt.type(math.sqrt(hd))
    s = np.where((np.asarray(mask) != 0)[:, None, None, :], s, np.finfo(dt).min).astype(dt)
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True, dtype=dt)
    return np.matmul(p, heads(v)).transpose(0, 2, 1, 3).reshape(B, T, dim)


def pool(hidden, mask, mode):
    """mode 0: mean over all positions; 1: mean over mask != 0, the count clamped to at least 1"""
    if mode == 0:
        return hidden.mean(1, dtype=hidden.dtype)
    w = (np.asarray(mask) != 0).astype(hidden.dtype)[:, :, None]
    return (hidden * w).sum(1, dtype=hidden.dtype) / np.maximum(w.sum(1), 1).astype(hidden.dtype)


def forward(sd, ids, mask, n_heads, dtype=np.float64):
    """last hidden state [B,T,dim] of the model `sd` (float32 arrays or tensors' numpy images) evaluated in `dtype`"""
    P = {k: np.asarray(v).astype(dtype, copy=False) for k, v in sd.items()}     # a state dict already in `dtype` is used as it is
    ids = np.asarray(ids)
    B, T = ids.shape
    n_layers = 1 + max(int(k.split(".")[2]) for k in P if k.startswith("transformer.layer."))
    x = P["embeddings.word_embeddings.weight"][ids] + P["embeddings.position_embeddings.weight"][None, :T]
    x = layernorm(x, P["embeddings.LayerNorm.weight"], P["embeddings.LayerNorm.bias"])

    def lin(x, name):
        return x @ P[name + ".weight"].T + P[name + ".bias"]
    for l in range(n_layers):
        p = f"transformer.layer.{l}."
        ctx = attention(lin(x, p + "attention.q_lin"), lin(x, p + "attention.k_lin"), lin(x, p + "attention.v_lin"), mask, n_heads)
        sa = layernorm(lin(ctx, p + "attention.out_lin") + x, P[p + "sa_layer_norm.weight"], P[p + "sa_layer_norm.bias"])
        h = gelu(lin(sa, p + "ffn.lin1"))
        x = layernorm(lin(h, p + "ffn.lin2") + sa, P[p + "output_layer_norm.weight"], P[p + "output_layer_norm.bias"])
    return x


def tokenize(sentences):
    """oracle.tiny_text.WhitespaceTokenizer as numpy: (ids, mask) int64 [B,T]"""
    from oracle import tiny_text
    enc = tiny_text.WhitespaceTokenizer()(list(sentences))
    return enc["input_ids"].numpy(), enc["attention_mask"].numpy()


def ragged_mask(B, T, seed):
    """[B,T] 0/1: sentence b keeps its first n_b tokens, n_b from 1 to T, the longest sentence full"""
    n = 1 + (detgen.unit(f"raggedmask{seed}", B) * T).astype(np.int64)
    n[B // 2] = T
    return (np.arange(T)[None, :] < n[:, None]).astype(np.int64)
