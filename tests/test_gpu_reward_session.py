"""-m gpu: RewardSession (r3m_amd/inference.py, R3M.reward_session): reset caches the first-frame embedding and the sentence features,
step runs the encoder session and r3m_langrew_infer. ResNet-18, hidden_dim = 64, 64 x 64 frames.

The reward's ceiling is the one of test_langrew_c_abi_vs_torch: max|d| <= 2e-5 of the float64 MLP's range over the rows of the call.
Where two session results are compared with each other (the same pair through E = 1 and through E = R), each is within that ceiling of
the float64 MLP on ITS OWN embeddings, so they may differ by the two ceilings plus the distance of the two float64 values."""
import functools

import numpy as np
import pytest
import torch

import text_ref
from util import DEV, rel_err

pytestmark = pytest.mark.gpu
CEIL = 2e-5
HW = (64, 64)


@functools.lru_cache(maxsize=None)
def _encoder_state():
    from oracle import detgen
    from r3m_amd.encoder import HipResNet
    shapes = [(k, tuple(v.shape)) for k, v in HipResNet(18).state_dict().items()]
    return {k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes, "w").items()}


def _model(train=False, **kw):
    from r3m_amd import R3M
    torch.manual_seed(11)
    m = R3M("cuda", 1e-4, 64, size=18, langweight=1.0, **kw)
    m.convnet.load_state_dict(_encoder_state())
    m = m.to(DEV)
    m.lang_enc.device = DEV
    m.train(train)
    return m


def _frames(tag, F):
    from oracle import detgen
    return torch.from_numpy(detgen.smooth_frames(tag, (F, 3) + HW, 7)).to(DEV)


def _feats(n, seed=2):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand((n, 768), generator=g) * 1.2 - 0.6)).to(DEV)


def _mlp64(m, e0, h, le):
    """float64 LanguageReward.pred on cat(e0, h, le) (models_language.py:43-55), on the CPU"""
    sd = {k: v.detach().cpu().double() for k, v in m.lang_rew.state_dict().items()}
    R = h.shape[0]
    x = torch.cat([e0.cpu().double().expand(R, -1), h.cpu().double(), le.cpu().double().expand(R, -1)], -1)
    for li in (0, 2, 4, 6):
        x = torch.relu(x @ sd[f"pred.{li}.weight"].t() + sd[f"pred.{li}.bias"])
    return (x @ sd["pred.8.weight"].t() + sd["pred.8.bias"]).view(-1)


def _assert_reward(what, r, ref, rng=None):
    rng = float(ref.abs().max()) if rng is None else rng
    err = float((r.cpu().double() - ref).abs().max()) / rng
    print(f"{what}: max|d| / range {err:.3e} (range {rng:.3e})")
    assert rng > 0 and err <= CEIL, (what, err)


def test_equivalence_with_the_kernels_forward_runs(hip):
    m = _model()
    first, frames, feats = _frames("rs_first", 1), _frames("rs_step", 5), _feats(1)
    rs = m.reward_session()
    rs.encoder_session.use_small_kernel = False
    with torch.no_grad():
        rs.reset(first, feats)
        r, h = rs.step(frames)
        h_ref, h0 = m(frames), m(first)
    torch.cuda.synchronize()
    assert r.shape == (5,) and h.shape == (5, 512)
    assert torch.equal(h, h_ref)
    _assert_reward("exact kernels, R = 5", r, _mlp64(m, h0, h, feats))


def test_default_kernels(hip):
    m = _model()
    first, frames, feats = _frames("rs_first", 1), _frames("rs_step", 5), _feats(1)
    rs = m.reward_session()
    assert rs.encoder_session.use_small_kernel
    with torch.no_grad():
        rs.reset(first, feats)
        r, h = rs.step(frames)
        r2, h2 = rs.step(frames)
        h_ref = m(frames)
        e0 = rs.encoder_session(first)
    torch.cuda.synchronize()
    assert torch.equal(r, r2) and torch.equal(h, h2)
    e = rel_err(h.cpu().numpy(), h_ref.cpu().numpy())[0]
    print(f"session embedding against forward(): max-rel {e:.3e}")
    assert e <= 1e-4                                    # tests/test_gpu_inference_session.py, the same comparison
    _assert_reward("default kernels, R = 5", r, _mlp64(m, e0, h, feats))


def test_shapes_one_first_frame_or_one_per_row(hip):
    m = _model()
    firsts, frames16, feats4 = _frames("rs_first4", 4), _frames("rs_step16", 16), _feats(4, seed=7)
    assert float((feats4[0] - feats4[1]).abs().max()) > 0.1
    rs = m.reward_session()
    with torch.no_grad():
        for R in (1, 4, 16):                            # E = 1, any R
            rs.reset(firsts[:1], feats4[:1])
            r, h = rs.step(frames16[:R])
            assert r.shape == (R,) and h.shape == (R, 512)
            e0 = rs.encoder_session(firsts[:1])
            ref16 = _mlp64(m, e0, rs.encoder_session(frames16), feats4[:1])
            _assert_reward(f"E = 1, R = {R}", r, _mlp64(m, e0, h, feats4[:1]), float(ref16.abs().max()))
        rs.reset(firsts, feats4)                        # E = R = 4, four different instructions
        r4, h4 = rs.step(frames16[:4])
        e04 = rs.encoder_session(firsts)
        ref4 = torch.stack([_mlp64(m, e04[i:i + 1], h4[i:i + 1], feats4[i:i + 1])[0] for i in range(4)])
        rng = float(ref4.abs().max())
        _assert_reward("E = R = 4", r4, ref4)
        assert r4.shape == (4,) and float((r4.max() - r4.min()).abs()) > 0
        for i in range(4):                              # each row against the E = 1 session of its own pair
            rs.reset(firsts[i:i + 1], feats4[i:i + 1])
            r1, h1 = rs.step(frames16[i:i + 1])
            ref1 = _mlp64(m, rs.encoder_session(firsts[i:i + 1]), h1, feats4[i:i + 1])[0]
            d = abs(float(r1[0]) - float(r4[i]))
            print(f"row {i}: E = 1 {float(r1[0]):.7f} E = 4 {float(r4[i]):.7f} float64 {float(ref1):.7f} / {float(ref4[i]):.7f}")
            assert abs(float(r1[0]) - float(ref1)) <= CEIL * rng
            assert d <= 2 * CEIL * rng + abs(float(ref1) - float(ref4[i]))
        with pytest.raises(ValueError, match="R must equal E"):
            rs.reset(firsts, feats4)
            rs.step(frames16[:3])
        with pytest.raises(ValueError, match="instructions"):
            rs.reset(firsts, feats4[:3])
    assert all(sl.arena is None for sl in m.convnet._ring), "the session took a slot of the encoder's live-forward ring"


def test_staleness_and_refusals(hip):
    from r3m_amd import R3M
    m = _model()
    first, frames, feats = _frames("rs_first", 1), _frames("rs_step", 2), _feats(1)
    rs = m.reward_session()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"reset\(\)"):
            rs.step(frames)                             # before any reset
        rs.reset(first, feats)
        r, _ = rs.step(frames)
        m.convnet.params_written()
        with pytest.raises(RuntimeError, match=r"reset\(\)"):
            rs.step(frames)
        with pytest.raises(RuntimeError, match=r"reset\(\)"):
            rs.step(frames)                             # until reset
        rs.reset(first, feats)
        assert torch.equal(rs.step(frames)[0], r)
    with pytest.raises(RuntimeError, match=r"forward\(\)"):
        rs.step(frames)                                 # grad enabled, trainable parameters
    with pytest.raises(RuntimeError, match=r"forward\(\)"):
        rs.reset(first, feats)
    for p in m.parameters():
        p.requires_grad_(False)
    assert torch.equal(rs.step(frames)[0], r)           # frozen parameters: fine without no_grad
    with pytest.raises(ValueError, match="language head"):
        R3M("cuda", 1e-4, 64, size=18, langweight=0.0).reward_session()


def test_sentences_through_the_native_encoder(hip):
    from oracle import tiny_text
    m = _model()
    m.lang_enc.use_native(tiny_text.WhitespaceTokenizer(), text_ref.g7_state_dict(), n_heads=4)
    first, frames = _frames("rs_first", 1), _frames("rs_step", 5)
    sent = [tiny_text.SENTENCES[2]]
    rs = m.reward_session()
    with torch.no_grad():
        feats = m.lang_enc(sent)
        calls = m.lang_enc.encoder_calls
        rs.reset(first, feats)
        assert m.lang_enc.encoder_calls == calls
        r_feat, _ = rs.step(frames)
        rs.reset(first, sent)
        assert m.lang_enc.encoder_calls == calls + 1 and m.lang_enc.few_rows is False
        r_sent, _ = rs.step(frames)
        rs.step(frames)
        assert m.lang_enc.encoder_calls == calls + 1
        rs.reset(first, sent)
        assert m.lang_enc.encoder_calls == calls + 2
        m.lang_enc.feature_cache[sent[0]] = feats[0].clone()          # a cache hit: no transformer pass
        rs.reset(first, sent)
        assert m.lang_enc.encoder_calls == calls + 2
        assert torch.equal(rs.step(frames)[0], r_feat)
    e = rel_err(r_sent.cpu().numpy(), r_feat.cpu().numpy())[0]
    print(f"reward from sentences (few-row text model) against the features path: max-rel {e:.3e}")
    assert e <= 1e-5


def test_a_forward_awaiting_its_backward_survives_the_session(hip):
    x, first, frames, feats = _frames("rs_saved", 2), _frames("rs_first", 1), _frames("rs_step", 3), _feats(1)
    cw = torch.linspace(0.5, 1.5, 2 * 512, device=DEV).view(2, 512)
    got = []
    for with_session in (True, False):
        m = _model(train=True)
        xg = x.clone().requires_grad_(True)
        h = m(xg)
        if with_session:
            rs = m.reward_session()
            with torch.no_grad():
                rs.reset(first, feats)
                for _ in range(3):
                    r, _ = rs.step(frames)
                assert r.shape == (3,)
        (h * cw).sum().backward()
        torch.cuda.synchronize()
        got.append((h.detach().clone(), xg.grad.clone(), m.convnet.flat_grads().clone()))
    for a, b in zip(*got):
        assert torch.equal(a, b)
