"""gpu: the native DistilBERT forward (csrc/text.hip through r3m_amd/text.py and LangEncoder.use_native) as a whole: against the
reference's own LangEncoder output on the tiny model (tests/golden/lang_encoder_tiny.npz, G7), against the float64 restatement of
tests/text_ref.py on deeper models, and inside one Trainer.update."""
import os

import numpy as np
import pytest
import torch

import text_ref
from util import DEV, rel_err

pytestmark = pytest.mark.gpu


def _g7_encoder(**kw):
    from oracle import tiny_text
    from r3m_amd.models_language import LangEncoder
    return LangEncoder(DEV, 0, 0, **kw).use_native(tiny_text.WhitespaceTokenizer(), text_ref.g7_state_dict(), n_heads=4)


# ---- G7: the reference's LangEncoder on the tiny model ----
def test_features_match_the_reference_lang_encoder(hip, golden_dir):
    from oracle import tiny_text
    g = np.load(os.path.join(golden_dir, "lang_encoder_tiny.npz"))
    enc = _g7_encoder()
    assert list(enc.state_dict()) == [] and list(enc.parameters()) == []
    f_all = enc(tiny_text.SENTENCES)
    assert f_all.shape == (8, 768) and f_all.is_cuda and not f_all.requires_grad and enc.encoder_calls == 1
    assert rel_err(f_all.cpu().numpy(), g["feats_all"])[0] < 1e-5
    # the padding quirk (models_language.py:34): the same sentence gets another feature next to a longer neighbour
    f_short = enc([tiny_text.SENTENCES[0], tiny_text.SENTENCES[3]])
    assert rel_err(f_short.cpu().numpy(), g["feats_short"])[0] < 1e-5
    assert float((f_short[0] - f_all[0]).abs().max()) > 0.1
    assert rel_err(enc(np.array(tiny_text.SENTENCES[3:6])).cpu().numpy(), g["feats_array_input"])[0] < 1e-5
    t = torch.randn(3, 768)
    assert enc(t) is t


def test_mask_padding_makes_features_batch_independent(hip):
    from oracle import tiny_text
    enc = _g7_encoder(mask_padding=True)
    f_all = enc(tiny_text.SENTENCES).cpu().numpy()
    f_short = enc([tiny_text.SENTENCES[0], tiny_text.SENTENCES[3]]).cpu().numpy()
    assert rel_err(f_short[0], f_all[0])[0] < 1e-5 and rel_err(f_short[1], f_all[3])[0] < 1e-5
    ref = _g7_encoder()([tiny_text.SENTENCES[0], tiny_text.SENTENCES[3]]).cpu().numpy()     # un-padded batch: both poolings agree
    assert rel_err(f_short, ref)[0] < 1e-5


def test_call_count_cache_and_precompute(hip):
    from oracle import tiny_text
    enc = _g7_encoder()
    enc.train()
    once = enc(tiny_text.SENTENCES)
    assert enc.encoder_calls == 1
    for _ in range(3):
        assert torch.equal(enc(tiny_text.SENTENCES), once)           # bit-identical from call to call
    assert enc.encoder_calls == 4
    with pytest.raises(ValueError, match="mask_padding"):
        enc.precompute(tiny_text.SENTENCES)
    cached = _g7_encoder(mask_padding=True)
    n = cached.precompute(tiny_text.SENTENCES + tiny_text.SENTENCES[:3], batch_size=3)
    assert n == len(set(tiny_text.SENTENCES)) and cached.encoder_calls == 3
    cached._hf = None                                                # cache hits must not touch the text model
    got = cached([tiny_text.SENTENCES[5], tiny_text.SENTENCES[0]])
    assert cached.encoder_calls == 3
    direct = _g7_encoder(mask_padding=True)([tiny_text.SENTENCES[5], tiny_text.SENTENCES[0]])
    assert rel_err(got.cpu().numpy(), direct.cpu().numpy())[0] < 1e-5


def test_old_backend_plug_gives_the_same_features(hip):
    """HipDistilBert through LangEncoder.use_backend (the HuggingFace calling convention: .last_hidden_state, pooled by torch) against
    use_native (pooled by the kernel), both pooling modes"""
    from oracle import tiny_text
    from r3m_amd.models_language import LangEncoder
    from r3m_amd.text import HipDistilBert
    model = HipDistilBert.from_state_dict(text_ref.g7_state_dict(), 4, DEV)
    for mp in (False, True):
        old = LangEncoder(DEV, 0, 0, mask_padding=mp).use_backend(tiny_text.WhitespaceTokenizer(), model)
        new = LangEncoder(DEV, 0, 0, mask_padding=mp).use_native(tiny_text.WhitespaceTokenizer(), model)
        a, b = old(tiny_text.SENTENCES), new(tiny_text.SENTENCES)
        assert old.encoder_calls == 1 and new.encoder_calls == 1
        assert rel_err(a.cpu().numpy(), b.cpu().numpy())[0] < 1e-6


def test_native_flag_converts_the_locally_found_huggingface_model(hip, golden_dir, monkeypatch):
    """LangEncoder(native=True) / R3M(native_text=True): what _load_hf finds locally is converted and the HuggingFace model dropped.
    The pretrained files are not in the image, so the two from_pretrained calls are pointed at the tiny stand-ins."""
    transformers = pytest.importorskip("transformers")
    from oracle import tiny_text
    from r3m_amd.models_language import LangEncoder
    from r3m_amd.text import HipDistilBert
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", lambda *a, **k: tiny_text.WhitespaceTokenizer())
    monkeypatch.setattr(transformers.AutoModel, "from_pretrained", lambda *a, **k: tiny_text.tiny_distilbert())
    enc = LangEncoder(DEV, 0, 0, native=True)
    feats = enc(tiny_text.SENTENCES)
    assert isinstance(enc._hf[1], HipDistilBert) and enc.encoder_calls == 1
    g = np.load(os.path.join(golden_dir, "lang_encoder_tiny.npz"))
    assert rel_err(feats.cpu().numpy(), g["feats_all"])[0] < 1e-5


def test_python_surface_refuses_on_the_host(hip):
    from r3m_amd.text import HipDistilBert
    model = HipDistilBert.from_state_dict({"distilbert." + k: v for k, v in text_ref.g7_state_dict().items()}, 4, DEV)
    assert model.dims == (59, 32, 768, 1, 4, 256) and not model.params.requires_grad
    assert model.params.numel() == sum(int(np.prod(s)) for _, s in text_ref.tensor_shapes(59, 32, 768, 1, 256))
    with pytest.raises(ValueError, match=r"\[0, 59\)"):
        model.features(torch.tensor([[1, 59]]), torch.ones(1, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="max_pos=32"):
        model.features(torch.ones(1, 33, dtype=torch.long), None)


# ---- deeper models against the float64 restatement ----
MODELS = {"a": dict(vocab=64, max_pos=128, dim=768, n_layers=6, n_heads=12, ffn=3072),
          "b": dict(vocab=64, max_pos=128, dim=256, n_layers=2, n_heads=4, ffn=512)}
SHAPES = [(1, 2), (3, 5), (5, 17), (2, 33), (1, 128)]


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
def test_deep_model_against_float64(hip, deep_models, name, B, T):
    """hidden state at EVERY position (padded rows included) and the features of both pool modes. The bound is measured, not fixed: the
    float32 evaluation of the restatement on the same case is the witness of what fp32 arithmetic loses through these layers, and the
    HIP result may be at most 4 x as far from float64 (the factor covers the MFMA summation order, which is not numpy's).
    Measured on an MI355X: see profiles/text_encoder_parity.txt."""
    from oracle import detgen
    d = MODELS[name]
    sd, sd64, model = deep_models[name]
    ids = (detgen.unit(f"deeptext_ids_{name}_{B}_{T}", B * T) * d["vocab"]).astype(np.int64).reshape(B, T)
    mask = text_ref.ragged_mask(B, T, 3)
    ref = text_ref.forward(sd64, ids, mask, d["n_heads"], np.float64)
    wit = text_ref.forward(sd, ids, mask, d["n_heads"], np.float32)
    assert wit.dtype == np.float32
    t_ids, t_mask = torch.from_numpy(ids), torch.from_numpy(mask)
    hidden = model(t_ids, t_mask).last_hidden_state
    assert hidden.shape == (B, T, d["dim"])
    got = {"hidden": hidden.cpu().numpy()}
    exp = {"hidden": (ref, wit)}
    for mode in (0, 1):
        feats = model.features(t_ids, t_mask, mask_padding=bool(mode))
        assert torch.equal(feats, model.features(t_ids, t_mask, mask_padding=bool(mode)))       # two calls, the same bits
        got[f"feats pool={mode}"] = feats.cpu().numpy()
        exp[f"feats pool={mode}"] = (text_ref.pool(ref, mask, mode), text_ref.pool(wit, mask, mode))
    bad = []
    for what, (r, w) in exp.items():
        assert np.isfinite(got[what]).all(), what
        e_hip, e_wit = rel_err(got[what], r), rel_err(w, r)
        ratios = [e_hip[i] / max(e_wit[i], 1e-30) for i in range(2)]
        print(f"PARITY model {name} B={B} T={T} {what}: hip max-rel {e_hip[0]:.3e} l2-rel {e_hip[1]:.3e} | witness max-rel {e_wit[0]:.3e} "
              f"l2-rel {e_wit[1]:.3e} | ratio max {ratios[0]:.2f} l2 {ratios[1]:.2f}")
        if not (e_hip[0] <= 4 * e_wit[0] and e_hip[1] <= 4 * e_wit[1]):
            bad.append((what, e_hip, e_wit))
    assert not bad, bad


# ---- inside a training step ----
def test_step_with_sentences_through_the_native_encoder(hip):
    """one Trainer.update (langweight = 1, ResNet-18, B = 2) fed sentence strings through a native G7 encoder gives the metrics of the same
    step fed the precomputed features"""
    from oracle import detgen, tiny_text
    from r3m_amd import R3M
    from r3m_amd.parallel import SingleDevice
    from r3m_amd.trainer import Trainer
    B = 2
    sents = [tiny_text.SENTENCES[0], tiny_text.SENTENCES[1]]
    res = {}
    for mode in ("strings", "features"):
        torch.manual_seed(3)
        m = R3M("cuda", 1e-4, 1024, size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=1.0)
        shapes = [(k, tuple(v.shape)) for k, v in m.convnet.state_dict().items()]
        m.convnet.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes).items()})
        keys = list(m.state_dict().keys())
        model = SingleDevice(m).to(DEV)
        m.lang_enc.device = DEV
        m.lang_enc.use_native(tiny_text.WhitespaceTokenizer(), text_ref.g7_state_dict(), n_heads=4)
        assert list(m.state_dict().keys()) == keys
        frames = torch.from_numpy(detgen.frames("textstep", (B, 5, 3, 224, 224))).to(DEV)
        torch.manual_seed(5)
        if mode == "strings":
            met, _ = Trainer(1).update(model, (frames, sents), 0)
            assert m.lang_enc.encoder_calls == 1
        else:
            feats = m.lang_enc(sents)
            torch.manual_seed(5)
            met, _ = Trainer(1).update(model, (frames, (feats, torch.ones(B))), 0)
        res[mode] = met
    assert res["strings"].keys() == res["features"].keys()
    for k in res["strings"]:
        a, b = res["strings"][k], res["features"][k]
        if isinstance(a, (int, float)):
            assert abs(a - b) <= 1e-6 * max(abs(a), abs(b)), (k, a, b)
