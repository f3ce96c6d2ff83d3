"""-m gpu: prepared inference (r3m_resnet_inference_prepare / r3m_resnet_forward_prepared) and InferenceSession.

(a) with flags bit 0 (no split-K kernel) the prepared forward is torch.equal to the existing no_grad forward — embedding and all four
    maps, ResNet-18 / -50, fp32 / bf16, 1 and 3 frames, 224 x 224 and 64 x 96 — and the prepared coefficient blocks are
    r3m_bn_eval_coeffs per layer bit for bit;
(b) with the split-K kernel on (fp32) the embedding meets the ceiling tests/test_gpu_encoder.py applies to the eval embedding against
    tests/golden/encoder_r{18,34,50}.npz (max|d| / max|ref| <= 1e-4, on the same goldens) and is torch.equal across two calls;
(c) freshness: load_state_dict moves the epoch; a raw in-place write does not, until refresh();
(d) a session call between a saved forward and its backward changes no gradient bit;
(e) inputs that require grad raise and name forward();
(f) one arena and one workspace across (F, H, W) changes; the engine refuses what the header says it refuses."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from util import DEV, rel_err

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _state(size, tag="w"):
    from oracle import detgen
    from r3m_amd.encoder import HipResNet
    shapes = [(k, tuple(v.shape)) for k, v in HipResNet(size).state_dict().items()]
    return {k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes, tag).items()}


def _encoder(size, precision="fp32", train=False, sd=None, **kw):
    from r3m_amd.encoder import HipResNet
    m = HipResNet(size, precision=precision, **kw)
    m.load_state_dict(sd if sd is not None else _state(size))
    m = m.to(DEV)
    m.train(train)
    return m


def _frames(tag, F, H, W):
    from oracle import detgen
    return torch.from_numpy(detgen.smooth_frames(tag, (F, 3, H, W), 7)).to(DEV)


def _other_statistics(size):
    sd = dict(_state(size))
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = sd[k] * 0.5 + 0.01
        elif k.endswith("running_var"):
            sd[k] = sd[k] * 1.7 + 0.05
    return sd


@pytest.mark.parametrize("hw", [(224, 224), (64, 96)])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [18, 50])
def test_prepared_forward_without_small_kernel_is_bit_identical(hip, size, precision, F, hw):
    m = _encoder(size, precision)
    x = _frames(f"sess{F}", F, *hw)
    sess = m.inference_session()
    sess.use_small_kernel = False
    with torch.no_grad():
        h_ref, maps_ref = m.forward_features(x)
        h, maps = sess.forward_features(x)
        h2 = sess(x)
    torch.cuda.synchronize()
    assert torch.equal(h, h_ref) and torch.equal(h2, h_ref)
    for k in maps_ref:
        assert torch.equal(maps[k], maps_ref[k]), k
    assert sess.prepares == 1
    # the coefficient blocks against r3m_bn_eval_coeffs, layer by layer
    plan = sess._plans[(F,) + hw]
    arena = sess._arena.view(torch.float32)
    st = torch.cuda.current_stream().cuda_stream
    for i in range(hip.r3m_resnet_num_convs(plan)):
        (_, _, g_off, shp), (_, _, b_off, _), (_, _, rm_off, _), (_, _, rv_off, _) = m._table[5 * i + 1:5 * i + 5]
        Co = shp[0]
        coef = torch.full((4, Co), float("nan"), device=DEV)
        p, b = m._flat_p, m._flat_b
        assert hip.r3m_bn_eval_coeffs(p[g_off:].data_ptr(), p[b_off:].data_ptr(), b[rm_off:].data_ptr(), b[rv_off:].data_ptr(), 1e-5,
                                      coef.data_ptr(), Co, st) == 0, hip.r3m_last_error()
        off = hip.r3m_debug_resnet_coef_offset(plan, i)
        assert off >= 0 and off % 4 == 0
        assert torch.equal(arena[off // 4: off // 4 + 4 * Co].view(4, Co), coef), f"coefficient block of convolution {i}"


@pytest.mark.parametrize("size", [18, 34, 50])
def test_session_with_small_kernel_meets_the_golden_ceiling(hip, golden_dir, size):
    from oracle import detgen
    from r3m_amd import R3M
    g = np.load(os.path.join(golden_dir, f"encoder_r{size}.npz"))
    m = R3M("cuda", 1e-4, 1024, size=size, langweight=0.0, tcnweight=1.0)
    m.convnet.load_state_dict(_state(size))
    m = m.to(DEV)
    m.eval()
    x = torch.from_numpy(detgen.frames("frames8", (8, 3, 224, 224))).to(DEV)
    sess = m.inference_session()
    with torch.no_grad():
        h = sess(x)
        again = sess(x)
    e_max, e_l2 = rel_err(h.cpu().numpy(), g["h_eval"])
    print(f"r{size} session eval: max-rel {e_max:.3e} l2-rel {e_l2:.3e}")
    assert hip.r3m_resnet_inference_workspace_bytes(sess._plans[(8, 224, 224)]) > 0, "no launch of this plan reaches the split-K kernel"
    assert e_max <= 1e-4
    assert torch.equal(h, again)
    # one frame, where every layer behind layer1 runs the split-K kernel, against the existing forward. The ceiling: 1e-4 is what the
    # project accepts between two fp32 evaluation orders of this network (the engine and the reference's CPU run that made the golden);
    # the session and forward() are two such orders again
    with torch.no_grad():
        h1, h1_again, ref1 = sess(x[:1]), sess(x[:1]), m(x[:1])
    e1 = rel_err(h1.cpu().numpy(), ref1.cpu().numpy())[0]
    print(f"r{size} session, one frame, against forward(): max-rel {e1:.3e}")
    assert e1 <= 1e-4 and torch.equal(h1, h1_again)


def test_freshness_epoch_and_refresh(hip):
    m = _encoder(18)
    x = _frames("fresh", 2, 224, 224)
    sess = m.inference_session()
    sess.use_small_kernel = False
    with torch.no_grad():
        h0 = sess(x)
        assert torch.equal(h0, m(x))
        sd2 = _other_statistics(18)
        m.load_state_dict(sd2)
        h1 = sess(x)
        fresh = _encoder(18, sd=sd2)
        want1 = fresh(x)
        assert torch.equal(h1, want1) and not torch.equal(h1, h0)
        assert sess.prepares == 2
        # a writer the epoch does not see: the session keeps answering from the old coefficients until refresh()
        for name, buf in m.named_buffers():
            if name.endswith("running_var"):
                buf.mul_(1.5)
        h2 = sess(x)
        assert torch.equal(h2, h1) and sess.prepares == 2
        sess.refresh()
        h3 = sess(x)
        want3 = m(x)
        assert torch.equal(h3, want3) and not torch.equal(h3, h1) and sess.prepares == 3
        # the project's own writers move the epoch: a train-mode forward (running statistics), an optimizer step
        e = m._epoch
        m.train()
        m(x)
        m.eval()
        assert m._epoch > e
        assert torch.equal(sess(x), m(x)) and sess.prepares == 4
    from r3m_amd.optim import FusedSGD
    opt = FusedSGD([m], lr=1e-3)
    xg = x.clone()
    m(xg).sum().backward()
    e = m._epoch
    opt.step()
    assert m._epoch > e
    with torch.no_grad():
        assert torch.equal(sess(x), m(x)) and sess.prepares == 5
    e = m._epoch
    m.to(DEV)
    assert m._epoch > e


def test_session_between_a_saved_forward_and_its_backward(hip):
    x = _frames("saved", 2, 224, 224)
    x2 = _frames("other", 1, 224, 224)
    cw = torch.linspace(0.5, 1.5, 2 * 512, device=DEV).view(2, 512)
    got = []
    for with_session in (True, False):
        m = _encoder(18, train=True)
        xg = x.clone().requires_grad_(True)
        h = m(xg)
        if with_session:
            for p in m.parameters():
                assert p.requires_grad
            with torch.no_grad():
                m.inference_session()(x2)
        (h * cw).sum().backward()
        torch.cuda.synchronize()
        got.append((h.detach().clone(), xg.grad.clone(), m.flat_grads().clone()))
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_session_refuses_autograd_and_clips(hip):
    m = _encoder(18)
    sess = m.inference_session()
    x = _frames("grad", 1, 64, 96)
    with pytest.raises(RuntimeError, match=r"forward\(\)"):
        sess(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match=r"forward\(\)"):
        sess(x)                                        # grad enabled and the parameters require grad
    for p in m.parameters():
        p.requires_grad_(False)
    assert sess(x).shape == (1, 512)                   # frozen parameters, plain input: fine without no_grad
    from r3m_amd.augment import CroppedClips
    raw = torch.zeros((1, 3, 240, 320), dtype=torch.uint8, device=DEV)
    boxes = torch.tensor([[0, 0, 224, 224]], dtype=torch.int32, device=DEV)
    with torch.no_grad(), pytest.raises(TypeError):
        sess(CroppedClips(raw, boxes, 1))


def test_one_arena_across_shapes_and_engine_refusals(hip):
    from r3m_amd import _lib
    m = _encoder(18)
    exact, fast = m.inference_session(), m.inference_session()
    exact.use_small_kernel = False
    seq = [((224, 224), 3), ((128, 128), 2), ((96, 160), 1), ((128, 128), 3), ((224, 224), 3), ((96, 160), 2)]
    with torch.no_grad():
        for i, ((H, W), F) in enumerate(seq):
            x = _frames(f"mix{i}", F, H, W)
            a, b, c, c2 = exact(x), _encoder(18)(x), fast(x), fast(x)
            torch.cuda.synchronize()
            assert torch.equal(a, b), (H, W, F)
            assert torch.equal(c, c2) and rel_err(c.cpu().numpy(), b.cpu().numpy())[0] <= 1e-4, (H, W, F)
            if i == 0:
                arena, ws = exact._arena.data_ptr(), fast._workspace.data_ptr()
    # the first shape is the largest: everything after it reused the same two buffers, each plan switch prepared again
    assert exact._arena.data_ptr() == arena and fast._workspace.data_ptr() == ws
    assert exact.prepares == len(seq) and len(exact._plans) == 5
    assert all(sl.arena is None for sl in m._ring), "the session took a slot of the encoder's live-forward ring"
    # the engine: a backward after a prepared forward, and a prepared forward after any other forward of the plan
    L, st = hip, torch.cuda.current_stream().cuda_stream
    F, H, W = 2, 96, 160
    h = exact._plans[(F, H, W)]
    x = _frames("mix5", F, H, W)
    out = torch.empty((F, 512), device=DEV)
    p, b, ar = m._flat_p.data_ptr(), m._flat_b.data_ptr(), exact._arena.data_ptr()
    assert L.r3m_resnet_backward(h, out.data_ptr(), p, p, ar, 0, 4, 0, st) != 0 and "inference mode" in _lib.last_error()
    assert L.r3m_resnet_forward(h, x.data_ptr(), p, b, ar, out.data_ptr(), 2, st) == 0, _lib.last_error()
    assert L.r3m_resnet_forward_prepared(h, x.data_ptr(), p, ar, None, out.data_ptr(), None, 1, st) != 0
    assert "not prepared" in _lib.last_error()
    assert L.r3m_resnet_inference_prepare(h, p, b, ar, st) == 0, _lib.last_error()
    assert L.r3m_resnet_forward_prepared(h, x.data_ptr(), p, ar, None, out.data_ptr(), None, 1, st) == 0, _lib.last_error()
    assert L.r3m_resnet_forward_prepared(h, x.data_ptr(), p, ar, None, out.data_ptr(), None, 2, st) != 0      # unknown flag bit
    torch.cuda.synchronize()
