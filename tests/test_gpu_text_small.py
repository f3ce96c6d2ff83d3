"""gpu: r3m_text_forward_small (HipDistilBert.features(..., few_rows=True)): the text model's sequence with every Linear that the
few-row plan takes at B * T rows on the split-K kernel of csrc/conv_small.hip (QKV, the output Linear and lin2 with the bias store, lin1
with bias + exact GELU in the store). The models `a` and `b` and the float64 / float32-witness scheme of
tests/test_gpu_text.py::test_deep_model_against_float64: hidden state and both pools at most 4 x the witness's distance from float64,
measured per case and printed in that test's format (profiles/text_encoder_parity.txt). Two calls give equal bits, and the default path
(few_rows=False) gives the same bits before and after a few_rows call."""
import numpy as np
import pytest
import torch

import text_ref
from util import DEV, rel_err

pytestmark = pytest.mark.gpu

MODELS = {"a": dict(vocab=64, max_pos=128, dim=768, n_layers=6, n_heads=12, ffn=3072),
          "b": dict(vocab=64, max_pos=128, dim=256, n_layers=2, n_heads=4, ffn=512)}
SHAPES = [(1, 2), (3, 5), (5, 17)]


@pytest.fixture(scope="module")
def deep_models():
    """name -> (float32 state dict, its float64 image, the HipDistilBert): built once, never modified"""
    from r3m_amd.text import HipDistilBert
    out = {}
    for name, d in MODELS.items():
        sd = text_ref.detgen_state_dict("deeptext_" + name, **d)
        sd64 = {k: v.astype(np.float64) for k, v in sd.items()}
        out[name] = (sd, sd64, HipDistilBert.from_state_dict(sd, d["n_heads"], DEV))
    return out


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("name", ["a", "b"])
def test_few_rows_against_float64(hip, deep_models, name, B, T):
    from oracle import detgen
    d = MODELS[name]
    sd, sd64, model = deep_models[name]
    ids = (detgen.unit(f"deeptext_ids_{name}_{B}_{T}", B * T) * d["vocab"]).astype(np.int64).reshape(B, T)
    mask = text_ref.ragged_mask(B, T, 3)
    ref = text_ref.forward(sd64, ids, mask, d["n_heads"], np.float64)
    wit = text_ref.forward(sd, ids, mask, d["n_heads"], np.float32)
    t_ids, t_mask = torch.from_numpy(ids), torch.from_numpy(mask)
    default_before = model.features(t_ids, t_mask)
    got, exp = {}, {}
    for mode in (0, 1):
        hidden, feats = model.hidden_and_pools(t_ids, t_mask, mask_padding=bool(mode), few_rows=True)
        hidden2, feats2 = model.hidden_and_pools(t_ids, t_mask, mask_padding=bool(mode), few_rows=True)
        assert torch.equal(feats, feats2) and torch.equal(hidden, hidden2)                        # two calls, the same bits
        assert torch.equal(feats, model.features(t_ids, t_mask, mask_padding=bool(mode), few_rows=True))
        assert hidden.shape == (B, T, d["dim"])
        got["hidden"], exp["hidden"] = hidden.cpu().numpy(), (ref, wit)
        got[f"feats pool={mode}"] = feats.cpu().numpy()
        exp[f"feats pool={mode}"] = (text_ref.pool(ref, mask, mode), text_ref.pool(wit, mask, mode))
    assert torch.equal(model.features(t_ids, t_mask), default_before), "the default path changed across a few_rows call"
    bad = []
    for what, (r, w) in exp.items():
        assert np.isfinite(got[what]).all(), what
        e_hip, e_wit = rel_err(got[what], r), rel_err(w, r)
        ratios = [e_hip[i] / max(e_wit[i], 1e-30) for i in range(2)]
        print(f"PARITY few_rows model {name} B={B} T={T} {what}: hip max-rel {e_hip[0]:.3e} l2-rel {e_hip[1]:.3e} | witness max-rel "
              f"{e_wit[0]:.3e} l2-rel {e_wit[1]:.3e} | ratio max {ratios[0]:.2f} l2 {ratios[1]:.2f}")
        if not (e_hip[0] <= 4 * e_wit[0] and e_hip[1] <= 4 * e_wit[1]):
            bad.append((what, e_hip, e_wit))
    assert not bad, bad


def test_g7_features_and_the_untouched_default(hip):
    """the tiny model of the reference's golden: few_rows features within the project's 1e-5 of the default ones, through LangEncoder's
    attribute; the default is torch.equal before and after"""
    from oracle import tiny_text
    from r3m_amd.models_language import LangEncoder
    enc = LangEncoder(DEV, 0, 0).use_native(tiny_text.WhitespaceTokenizer(), text_ref.g7_state_dict(), n_heads=4)
    assert enc.few_rows is False
    before = enc(tiny_text.SENTENCES)
    enc.few_rows = True
    few = enc(tiny_text.SENTENCES)
    assert torch.equal(few, enc(tiny_text.SENTENCES))
    enc.few_rows = False
    after = enc(tiny_text.SENTENCES)
    assert torch.equal(before, after)
    assert enc.encoder_calls == 4
    e = rel_err(few.cpu().numpy(), before.cpu().numpy())[0]
    print(f"G7 few_rows against the default features: max-rel {e:.3e}")
    assert e < 1e-5
    on = LangEncoder(DEV, 0, 0).use_native(tiny_text.WhitespaceTokenizer(), text_ref.g7_state_dict(), n_heads=4, few_rows=True)
    assert on.few_rows is True and torch.equal(on(tiny_text.SENTENCES), few)
    L = hip
    dims = (59, 32, 768, 1, 4, 256)
    import ctypes as C
    d6 = (C.c_int * 6)(*dims)
    assert L.r3m_text_small_workspace_bytes(d6, 8, 7) >= L.r3m_text_workspace_bytes(d6, 8, 7) > 0
    assert L.r3m_text_small_workspace_bytes(d6, 1, 129) == 0 and b"T=129" in L.r3m_last_error()     # the refusals of r3m_text_forward
