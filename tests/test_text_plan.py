"""not gpu: the host side of the native text model (csrc/text.hip, r3m_amd/text.py): the numpy restatement of DistilBERT the GPU tests
are judged by (tests/text_ref.py) against the reference's own LangEncoder output (G7) and against transformers, the flat parameter
layout, every refusal of the C ABI (dummy pointers: a refusal returns before any HIP call), and the Python surface's errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import text_ref
from util import rel_err

BASE = (30522, 512, 768, 6, 12, 3072)      # distilbert-base-uncased
G7 = (59, 32, 768, 1, 4, 256)


def _d(dims):
    return (ctypes.c_int * 6)(*dims)


def _hf_tiny():
    pytest.importorskip("transformers")
    from oracle import tiny_text
    return tiny_text.tiny_distilbert()


# ---- the restatement ----
def test_restatement_matches_the_reference_lang_encoder(golden_dir):
    from oracle import tiny_text
    g = np.load(os.path.join(golden_dir, "lang_encoder_tiny.npz"))
    sd = text_ref.g7_state_dict()
    for key, sentences in (("feats_all", tiny_text.SENTENCES), ("feats_short", [tiny_text.SENTENCES[0], tiny_text.SENTENCES[3]]),
                           ("feats_array_input", tiny_text.SENTENCES[3:6])):
        ids, mask = text_ref.tokenize(sentences)
        feats = text_ref.pool(text_ref.forward(sd, ids, mask, 4), mask, 0)
        assert rel_err(feats, g[key])[0] < 1e-5, key
        feats32 = text_ref.pool(text_ref.forward(sd, ids, mask, 4, np.float32), mask, 0)     # the witness evaluates the same model
        assert feats32.dtype == np.float32 and rel_err(feats32, g[key])[0] < 1e-5, key


def test_restatement_matches_transformers_in_float64_on_every_position():
    from oracle import tiny_text
    model = _hf_tiny()
    sd = text_ref.g7_state_dict()
    hf = {k: v for k, v in model.state_dict().items() if v.is_floating_point()}
    assert list(hf) == [n for n, _ in text_ref.tensor_shapes(59, 32, 768, 1, 256)]
    for k, v in hf.items():
        assert np.array_equal(v.numpy(), sd[k]), k
    ids, mask = text_ref.tokenize(tiny_text.SENTENCES)
    with torch.no_grad():
        out = model.double()(torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).last_hidden_state.numpy()
    assert mask.min() == 0                                   # padded rows are part of the comparison
    assert np.abs(text_ref.forward(sd, ids, mask, 4) - out).max() < 1e-12


def test_pool_modes_of_the_restatement():
    h = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    mask = np.array([[1, 1, 0], [0, 0, 0]])
    assert np.array_equal(text_ref.pool(h, mask, 0), h.mean(1))
    assert np.array_equal(text_ref.pool(h, mask, 1)[0], h[0, :2].mean(0)) and not text_ref.pool(h, mask, 1)[1].any()


# ---- flat layout ----
def test_num_params_of_distilbert_base():
    from r3m_amd import _lib
    L = _lib.lib()
    assert L.r3m_text_num_params(_d(BASE)) == 66362880
    assert L.r3m_text_num_tensors(_d(BASE)) == 4 + 16 * 6
    assert L.r3m_text_num_params(_d(G7)) == sum(int(np.prod(s)) for _, s in text_ref.tensor_shapes(59, 32, 768, 1, 256))


ONE_LAYER = [
    ("embeddings.word_embeddings.weight", (59, 768)), ("embeddings.position_embeddings.weight", (32, 768)),
    ("embeddings.LayerNorm.weight", (768,)), ("embeddings.LayerNorm.bias", (768,)),
    ("transformer.layer.0.attention.q_lin.weight", (768, 768)), ("transformer.layer.0.attention.k_lin.weight", (768, 768)),
    ("transformer.layer.0.attention.v_lin.weight", (768, 768)), ("transformer.layer.0.attention.q_lin.bias", (768,)),
    ("transformer.layer.0.attention.k_lin.bias", (768,)), ("transformer.layer.0.attention.v_lin.bias", (768,)),
    ("transformer.layer.0.attention.out_lin.weight", (768, 768)), ("transformer.layer.0.attention.out_lin.bias", (768,)),
    ("transformer.layer.0.sa_layer_norm.weight", (768,)), ("transformer.layer.0.sa_layer_norm.bias", (768,)),
    ("transformer.layer.0.ffn.lin1.weight", (256, 768)), ("transformer.layer.0.ffn.lin1.bias", (256,)),
    ("transformer.layer.0.ffn.lin2.weight", (768, 256)), ("transformer.layer.0.ffn.lin2.bias", (768,)),
    ("transformer.layer.0.output_layer_norm.weight", (768,)), ("transformer.layer.0.output_layer_norm.bias", (768,)),
]


@pytest.mark.parametrize("dims", [G7, BASE, (64, 128, 256, 2, 4, 512)])
def test_tensor_table_is_disjoint_aligned_and_covers_the_buffer(dims):
    from r3m_amd import _lib, text
    table = text.tensor_table(dims)
    assert len(table) == 4 + 16 * dims[3]
    expect = dict(text_ref.tensor_shapes(dims[0], dims[1], dims[2], dims[3], dims[5]))
    assert {n: s for n, _, _, s in table} == expect                      # HuggingFace's names and shapes, each once
    end = 0
    for name, off, cnt, shape in sorted(table, key=lambda t: t[1]):
        assert off == end, f"{name}: gap or overlap at {off} (previous tensor ends at {end})"
        assert (off * 4) % 16 == 0 and cnt == int(np.prod(shape)), name
        end = off + cnt
    assert end == _lib.lib().r3m_text_num_params(_d(dims))
    # q, k, v of a layer adjacent, weights then biases: QKV is one [3 dim, dim] Linear on the flat buffer
    by = {n: o for n, o, _, _ in table}
    D = dims[2]
    for l in range(dims[3]):
        p = f"transformer.layer.{l}.attention."
        w, b = by[p + "q_lin.weight"], by[p + "q_lin.bias"]
        assert [by[p + f"{x}_lin.weight"] for x in "kv"] == [w + D * D, w + 2 * D * D] and b == w + 3 * D * D
        assert [by[p + f"{x}_lin.bias"] for x in "kv"] == [b + D, b + 2 * D]


def test_tensor_table_of_one_layer_by_name():
    from r3m_amd import text
    assert [(n, s) for n, _, _, s in text.tensor_table(G7)] == ONE_LAYER


def test_tensor_table_matches_the_huggingface_state_dict():
    from r3m_amd import text
    hf = {k: tuple(v.shape) for k, v in _hf_tiny().state_dict().items() if v.is_floating_point()}
    assert {n: s for n, _, _, s in text.tensor_table(G7)} == hf


# ---- refusals ----
def _forward_rc(L, dims, B, T, ws_bytes=None, pool=0):
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf) // 16 * 16 + 16
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return L.r3m_text_forward(p, p, p, p, None, p, ws_bytes, B, T, _d(dims), pool, None)


@pytest.mark.parametrize("what,dims,B,T,message", [
    ("T = 0", G7, 2, 0, b"T=0"),
    ("T = 129", (64, 512, 768, 1, 12, 256), 2, 129, b"T=129"),
    ("T > max_pos", G7, 2, 33, b"max_pos=32"),
    ("head_dim = 48", (64, 32, 192, 1, 4, 256), 2, 8, b"head_dim"),
    ("dim = 96", (64, 32, 96, 1, 3, 256), 2, 8, b"dim=96"),
    ("ffn = 96", (64, 32, 128, 1, 4, 96), 2, 8, b"ffn_dim=96"),
    ("B = 0", G7, 0, 8, b"B=0"),
    ("LDS", (64, 128, 768, 1, 4, 256), 2, 128, b"bytes of LDS"),
    ("2^31", BASE, 1 << 16, 16, b"2^31"),
])
def test_refusals_come_back_before_any_gpu_work(what, dims, B, T, message):
    from r3m_amd import _lib
    L = _lib.lib()
    assert _forward_rc(L, dims, B, T) != 0, what
    assert message in L.r3m_last_error() and b"text_forward" in L.r3m_last_error(), (what, L.r3m_last_error())
    assert L.r3m_text_workspace_bytes(_d(dims), B, T) == 0


def test_workspace_and_argument_refusals():
    from r3m_amd import _lib
    L = _lib.lib()
    need = L.r3m_text_workspace_bytes(_d(G7), 2, 8)
    assert need >= 4 * 2 * 8 * (4 * 768 + 3 * 768)                       # x, sa, tmp, ctx and the qkv rows at the least
    assert _forward_rc(L, G7, 2, 8, ws_bytes=need - 1) != 0 and b"workspace too small" in L.r3m_last_error()
    assert _forward_rc(L, G7, 2, 8, pool=2) != 0 and b"pool=2" in L.r3m_last_error()
    buf = (ctypes.c_int * 16)()
    p = ctypes.addressof(buf)
    assert L.r3m_text_forward(None, p, p, p, None, p, 1 << 40, 2, 8, _d(G7), 0, None) != 0 and b"null" in L.r3m_last_error()
    assert L.r3m_text_num_params(_d((59, 32, 96, 1, 3, 256))) == -1 and b"dim=96" in L.r3m_last_error()
    # the stand-alone kernels refuse on the host too
    assert L.r3m_attention_fwd(p, p, p, 1, 129, 2, 64, None) != 0 and b"T=129" in L.r3m_last_error()
    assert L.r3m_attention_fwd(p, p, p, 1, 8, 2, 48, None) != 0 and b"head_dim=48" in L.r3m_last_error()
    assert L.r3m_attention_fwd(p, p, p, 1, 128, 2, 192, None) != 0 and b"bytes of LDS" in L.r3m_last_error()
    assert L.r3m_layernorm_fwd(p, None, p, p, p, 4, 6, 1e-12, None) != 0 and b"C=6" in L.r3m_last_error()
    assert L.r3m_layernorm_fwd(p, None, p, p, p, 0, 64, 1e-12, None) != 0 and b"rows=0" in L.r3m_last_error()
    assert L.r3m_bias_gelu(p, p, 4, 6, None) != 0 and b"C=6" in L.r3m_last_error()
    assert L.r3m_text_embed(p, p, p, p, p, p, 0, 4, 64, 8, 1e-12, None) != 0 and b"B=0" in L.r3m_last_error()
    assert L.r3m_text_pool(p, p, p, 2, 4, 64, 3, None) != 0 and b"pool=3" in L.r3m_last_error()
    assert L.r3m_text_pool(p, p, p, 0, 4, 64, 0, None) != 0 and b"B=0" in L.r3m_last_error()


# ---- Python surface ----
def test_no_cpu_fallback():
    from oracle import tiny_text
    from r3m_amd.models_language import LangEncoder
    from r3m_amd.text import HipDistilBert
    sd = {k: torch.from_numpy(v) for k, v in text_ref.g7_state_dict().items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HipDistilBert.from_state_dict(sd, 4, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LangEncoder("cpu", 0, 0).use_native(tiny_text.WhitespaceTokenizer(), sd, n_heads=4)
    with pytest.raises(ValueError, match="n_heads"):
        LangEncoder("cpu", 0, 0).use_native(tiny_text.WhitespaceTokenizer(), sd)


def test_bad_ids_and_lengths_raise_on_the_host():
    from r3m_amd.text import HipDistilBert
    m = HipDistilBert(G7, torch.zeros(4))            # no device work is reached: every check below is on the host
    ok = torch.ones(2, 5, dtype=torch.long)
    for bad in (59, -1):
        ids = ok.clone()
        ids[1, 2] = bad
        with pytest.raises(ValueError, match=r"\[0, 59\)"):
            m.features(ids, torch.ones_like(ids))
    with pytest.raises(ValueError, match="at most 128"):
        HipDistilBert((64, 512, 768, 1, 12, 256), torch.zeros(4)).features(torch.ones(1, 129, dtype=torch.long), None)
    with pytest.raises(ValueError, match="max_pos=32"):
        m.features(torch.ones(1, 33, dtype=torch.long), None)
    with pytest.raises(ValueError, match="attention_mask"):
        m.features(ok, torch.ones(2, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.features(ok, torch.ones_like(ok))


def test_state_dict_loader_refuses_what_it_cannot_place():
    from r3m_amd.text import HipDistilBert
    with pytest.raises(ValueError, match="not a DistilBERT state dict"):
        HipDistilBert.from_state_dict({"foo.weight": torch.zeros(3)}, 4, "cuda")


def test_module_tree_is_unchanged_by_the_native_text_model():
    """state_dict keys, parameters and the optimizer's owners with native_text, and after a native model is plugged in, are those of
    today's default: the text model stays off the module tree."""
    from r3m_amd import R3M
    from r3m_amd.text import HipDistilBert

    def view(m):
        return list(m.state_dict().keys()), [n for n, _ in m.named_parameters()], [type(o).__name__ for o in m.encoder_opt.owners]
    base = R3M("cpu", 1e-4, 64, size=18, langweight=1.0)
    assert base.lang_enc.native is False
    native = R3M("cpu", 1e-4, 64, size=18, langweight=1.0, native_text=True)
    assert native.lang_enc.native is True and view(native) == view(base)
    assert not any("lang_enc" in k for k in view(base)[0])
    base.lang_enc._hf = (None, HipDistilBert(G7, torch.zeros(4)))         # what use_native leaves behind
    base.train()
    assert view(base) == view(native) and list(base.lang_enc.state_dict()) == []
