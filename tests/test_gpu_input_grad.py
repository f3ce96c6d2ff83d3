"""Gradients w.r.t. the input frames (obs.grad) through the HIP encoder: the stem input-gradient operator, the adjoint of the
resize + center-crop gather, r3m_resnet_backward_ex (optional parameter gradients, optional input gradient) and the autograd
surface (HipResNet / R3M.forward / LanguageReward on top). The reference's R3M is a plain autograd graph
(/root/reference/r3m/models/models_r3m.py:84-100): obs.requires_grad_(True); r3m(obs).sum().backward() fills obs.grad there.

Comparators: the pinned oracle encoder (oracle/resnet_ref.py) in float64 on the CPU, with /255 and Normalize written out. The input
gradient crosses every ReLU and max-pool, so the encoder-level gates are G8-style: err(X) = ||X - fp64|| / ||fp64||, and the median over
three (weights, frames) draws of err(HIP) / err(torch CPU fp32 of the same graph) must be <= 2, every draw <= 4 (an error below 1e-4
always passes)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64).view(1, 3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64).view(1, 3, 1, 1)
DRAWS = [("w", "smooth"), ("wb", "smoothb"), ("wc", "smoothc")]     # (weight tag, frame tag) of oracle/detgen.py


def report(line):
    print(line, flush=True)


def l2rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _stream():
    from r3m_amd import _lib
    return _lib.stream_ptr(torch.device(DEV))


def _stem_ref(dz_nhwc, w_ohwi):
    """float64 d/d(frames 0..255) of x/255 -> Normalize -> conv1 for conv1's output gradient dz: conv_transpose2d, then 1/(255 std)."""
    dz = dz_nhwc.double().cpu().permute(0, 3, 1, 2)
    w = w_ohwi.double().cpu().permute(0, 3, 1, 2)            # OIHW
    dxn = Fn.conv_transpose2d(dz, w, stride=2, padding=3, output_padding=1)
    return dxn / (255.0 * STD)


# ---- 1. the stem operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("F", [1, 3, 8, 64])
def test_stem_input_grad_operator(hip, F, dtype):
    g = torch.Generator().manual_seed(100 + F)
    w = (torch.randn(64, 7, 7, 3, generator=g) * 0.1).to(DEV)
    dz = torch.randn(F, 112, 112, 64, generator=g)
    dt = 0
    if dtype == "bf16":
        dz, dt = dz.to(torch.bfloat16), 1
    dz = dz.to(DEV)
    ref = _stem_ref(dz.float(), w)                             # float64 of the (bf16-rounded) dz
    dx = torch.full((F, 3, 224, 224), float("nan"), device=DEV)
    assert hip.r3m_stem_input_grad(dz.data_ptr(), dt, w.data_ptr(), dx.data_ptr(), F, 0, _stream()) == 0
    torch.cuda.synchronize()
    e = l2rel(dx, ref)
    report(f"stem input grad {dtype} F={F}: l2-rel vs float64 {e:.3e}")
    assert torch.isfinite(dx).all() and e <= 1e-5, e
    base = torch.randn(F, 3, 224, 224, generator=g).to(DEV)
    acc = base.clone()
    assert hip.r3m_stem_input_grad(dz.data_ptr(), dt, w.data_ptr(), acc.data_ptr(), F, 1, _stream()) == 0
    torch.cuda.synchronize()
    e_acc = l2rel(acc, base.double().cpu() + ref)
    assert e_acc <= 1e-5, e_acc


# ---- 2. frame indexing at the largest frame count --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stem_input_grad_large_frame_count(hip, dtype):
    """A 1280-frame call (the pre-training frame count): frames 0, 637 and 1279 are bit-identical to 1-frame calls on the same data."""
    F = 1280
    torch.manual_seed(7)
    dz = torch.randn(F, 112, 112, 64, device=DEV, dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
    dt = 1 if dtype == "bf16" else 0
    w = torch.randn(64, 7, 7, 3, device=DEV) * 0.1
    dx = torch.empty(F, 3, 224, 224, device=DEV)
    assert hip.r3m_stem_input_grad(dz.data_ptr(), dt, w.data_ptr(), dx.data_ptr(), F, 0, _stream()) == 0
    for f in (0, 637, 1279):
        one = torch.empty(1, 3, 224, 224, device=DEV)
        src = dz[f:f + 1].contiguous()
        assert hip.r3m_stem_input_grad(src.data_ptr(), dt, w.data_ptr(), one.data_ptr(), 1, 0, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(dx[f:f + 1], one), f
    del dz, dx
    torch.cuda.empty_cache()


# ---- 3. the adjoint of resize + center crop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(500, 500), (480, 640), (640, 480), (256, 341)])
def test_resize_crop_backward(hip, hw):
    from r3m_amd.augment import resize_center_crop, resize_center_crop_geometry
    H, W = hw
    nh, nw, top, left = resize_center_crop_geometry(H, W)
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.rand(2, 3, H, W, generator=g) * 255
    dout = torch.randn(2, 3, 224, 224, generator=g)
    # autograd of F.interpolate + crop in float64, and in float32 (whose source indices are computed in float32, as the forward's)
    grads = []
    for dtype in (torch.float64, torch.float32):
        xr = x.detach().to(dtype).clone().requires_grad_(True)
        yr = Fn.interpolate(xr, size=(nh, nw), mode="bilinear", align_corners=False)[:, :, top:top + 224, left:left + 224]
        (yr * dout.to(dtype)).sum().backward()
        grads.append(xr.grad.double())
    xg = x.detach().to(DEV).clone().requires_grad_(True)
    y = resize_center_crop(xg)
    y.backward(dout.to(DEV))
    e, e_cpu = l2rel(xg.grad, grads[0]), l2rel(grads[1], grads[0])
    report(f"resize-crop adjoint {H}x{W}: l2-rel vs float64 autograd {e:.3e} (torch-cpu-fp32 {e_cpu:.3e})")
    assert e <= max(1e-5, 2.0 * e_cpu), (e, e_cpu)
    # adjoint identity <R x, y> = <x, R^T y>
    lhs = float((y.detach().double() * dout.double().to(DEV)).sum())
    rhs = float((x.double().to(DEV) * xg.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    # deterministic: the same bits on a repeat (a gather, no atomics)
    din2 = torch.empty_like(xg.grad)
    d = dout.to(DEV).contiguous()
    assert hip.r3m_resize_crop_backward(d.data_ptr(), din2.data_ptr(), 2, 3, H, W, nh, nw, top, left, 224, 224, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(din2, xg.grad)


# ---- encoder helpers ---------------------------------------------------------------------------------------------------------------
def _enc(m, v):
    z = m.maxpool(m.relu(m.bn1(m.conv1(v))))
    return m.layer4(m.layer3(m.layer2(m.layer1(z)))).mean((2, 3))


def _state(size, wtag):
    from oracle import detgen, resnet_ref
    ref0 = getattr(resnet_ref, f"resnet{size}")()
    shapes = [(k, tuple(v.shape)) for k, v in ref0.state_dict().items() if not k.startswith("fc.")]
    return {k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict_small_residual(shapes, size, 0.1, tag=wtag).items()}


def _cpu_obs_grad(size, sd, x, cw, train, dtype, autocast=False):
    """obs.grad of sum(encoder(Normalize(x / 255)) * cw) through the pinned oracle on the CPU."""
    from oracle import resnet_ref
    m = getattr(resnet_ref, f"resnet{size}")().to(dtype)
    m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, strict=False)
    m.train(train)
    xv = x.detach().to(dtype).clone().requires_grad_(True)
    xn = (xv / 255.0 - MEAN.to(dtype)) / STD.to(dtype)
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            h = _enc(m, xn)
        h = h.float()
    else:
        h = _enc(m, xn)
    (h * cw.to(h.dtype)).sum().backward()
    return xv.grad.detach().double()


def _hip_encoder(size, sd, train, precision="fp32", frozen=False, max_live_forwards=1):
    from r3m_amd.encoder import HipResNet
    m = HipResNet(size, precision=precision, max_live_forwards=max_live_forwards)
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV)
    m.train(train)
    if frozen:
        for p in m.parameters():
            p.requires_grad_(False)
    return m


def _hip_obs_grad(m, x, cw):
    xg = x.detach().to(DEV).clone().requires_grad_(True)
    h = m(xg)
    (h * cw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return xg.grad.detach()


def _gate(name, pairs):
    """pairs: [(err hip, err torch-cpu)] over the draws -> median ratio <= 2, max <= 4 (err <= 1e-4 always passes)"""
    ratios = [0.0 if eh <= 1e-4 else eh / max(ec, 1e-12) for eh, ec in pairs]
    med = sorted(ratios)[len(ratios) // 2]
    report(f"{name}: obs.grad err hip / torch-cpu per draw " + ", ".join(f"{eh:.2e}/{ec:.2e}" for eh, ec in pairs)
           + f"  ratios {', '.join(f'{r:.2f}' for r in ratios)} median {med:.2f}")
    assert med <= 2.0 and max(ratios) <= 4.0, (name, pairs, ratios)


# ---- 4. encoder obs.grad, fp32 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("size", [18, 34, 50])
def test_encoder_obs_grad_fp32(hip, size, train):
    """obs.grad with trainable parameters (today's code leaves it None). The three draws use F = 1, 3 and 8 frames in eval mode. In
    train mode a single frame leaves layer4's batch statistics 49 samples per channel, and one fp32 ReLU / max-pool decision that
    flips against float64 there moved the error 14x on one side only (ResNet-34, draw 0: hip 1.6e-3, torch 1.2e-4; draw 1: both
    1.76e-3): train mode takes F = 3, 8, 8."""
    from oracle import detgen
    pairs = []
    for (wtag, ftag), F in zip(DRAWS, (1, 3, 8) if not train else (3, 8, 8)):
        sd = _state(size, wtag)
        x = torch.from_numpy(detgen.smooth_frames(ftag, (F, 3, 224, 224), 7))
        cw = torch.from_numpy(detgen.uniform("cw" + ftag, (F, 512 * (4 if size == 50 else 1)), 0.5, 1.5))
        g64 = _cpu_obs_grad(size, sd, x, cw, train, torch.float64)
        g32 = _cpu_obs_grad(size, sd, x, cw, train, torch.float32)
        m = _hip_encoder(size, sd, train)
        gh = _hip_obs_grad(m, x, cw)
        assert torch.isfinite(gh).all()
        assert m.conv1.weight.grad is not None        # trainable parameters still get their gradients
        pairs.append((l2rel(gh, g64), l2rel(g32, g64)))
    _gate(f"r{size} {'train' if train else 'eval'} fp32", pairs)


# ---- 5. frozen encoder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_frozen_encoder_obs_grad(hip, train):
    from oracle import detgen
    size, F = 18, 3
    sd = _state(size, "w")
    x = torch.from_numpy(detgen.smooth_frames("smooth", (F, 3, 224, 224), 7))
    cw = torch.from_numpy(detgen.uniform("cwfrozen", (F, 512), 0.5, 1.5))
    mt = _hip_encoder(size, sd, train)
    g_trainable = _hip_obs_grad(mt, x, cw)
    mf = _hip_encoder(size, sd, train, frozen=True)
    g_frozen = _hip_obs_grad(mf, x, cw)
    assert torch.equal(g_frozen, g_trainable)
    assert all(p.grad is None for p in mf.parameters())
    assert mf._flat_g is None
    for (k, bt), (k2, bf) in zip(mt.named_buffers(), mf.named_buffers()):
        assert k == k2 and torch.equal(bt, bf), k      # running statistics (train mode) move exactly as with trainable parameters
    if train:
        assert not torch.equal(mf.bn1.running_mean.cpu(), sd["bn1.running_mean"].float())


# ---- 6. the weight path is unchanged ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_param_grads_unchanged_by_obs_grad(hip, precision):
    from oracle import detgen
    size, F = 50, 4
    sd = _state(size, "w")
    x = torch.from_numpy(detgen.smooth_frames("smooth", (F, 3, 224, 224), 7)).to(DEV)
    cw = torch.from_numpy(detgen.uniform("cwreg", (F, 2048), 0.5, 1.5)).to(DEV)
    grads = []
    for with_obs in (False, True):
        m = _hip_encoder(size, sd, True, precision=precision)
        xi = x.clone().requires_grad_(with_obs)
        (m(xi) * cw).sum().backward()
        torch.cuda.synchronize()
        grads.append(m.flat_grads().clone())
        if with_obs:
            g1 = xi.grad.clone()
    assert torch.equal(grads[0], grads[1])
    # obs.grad accumulates across two backwards of one forward, as torch's does
    m = _hip_encoder(size, sd, False, precision=precision)
    xi = x.clone().requires_grad_(True)
    loss = (m(xi) * cw).sum()
    loss.backward(retain_graph=True)
    first = xi.grad.clone()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(xi.grad, first + first)
    assert torch.isfinite(g1).all()


# ---- 7. bf16 plans against torch.autocast -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [18, 50])
def test_encoder_obs_grad_bf16_against_autocast(hip, size):
    from oracle import detgen
    N = 4 if size == 50 else 8
    pairs = []
    for wtag, ftag in DRAWS:
        sd = _state(size, wtag)
        x = torch.from_numpy(detgen.smooth_frames(ftag, (N, 3, 224, 224), 7))
        cw = torch.from_numpy(detgen.uniform("cw" + ftag, (N, 512 * (4 if size == 50 else 1)), 0.5, 1.5))
        g64 = _cpu_obs_grad(size, sd, x, cw, True, torch.float64)
        gac = _cpu_obs_grad(size, sd, x, cw, True, torch.float32, autocast=True)
        m = _hip_encoder(size, sd, True, precision="bf16")
        gh = _hip_obs_grad(m, x, cw)
        pairs.append((l2rel(gh, g64), l2rel(gac, g64)))
    _gate(f"r{size} bf16 vs autocast", pairs)


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------
def _r3m(size, sd, frozen=True, max_live_forwards=1):
    from r3m_amd import R3M
    m = R3M(DEV, 1e-4, 1024, size=size, l2weight=1e-5, l1weight=1e-5, langweight=0.0, tcnweight=1.0,
            max_live_forwards=max_live_forwards)
    m.convnet.load_state_dict(sd, strict=False)
    m = m.to(DEV)
    m.convnet.eval()
    if frozen:
        for p in m.convnet.parameters():
            p.requires_grad_(False)
    return m


def _resize_ref(x, H, W):
    from r3m_amd.augment import resize_center_crop_geometry
    nh, nw, top, left = resize_center_crop_geometry(H, W)
    v = Fn.interpolate(x / 255.0, size=(nh, nw), mode="bilinear", align_corners=False)[:, :, top:top + 224, left:left + 224]
    return (v - MEAN.to(x.dtype)) / STD.to(x.dtype)


def test_r3m_forward_other_size_obs_grad(hip):
    """R3M.forward(obs, obs_shape=[3,240,320]) on float frames: Resize(256) + CenterCrop(224) + x/255 + Normalize + encoder, all
    differentiable; obs.grad against the float64 chain."""
    from oracle import detgen, resnet_ref
    size, F, H, W = 18, 2, 240, 320
    sd = _state(size, "w")
    x = torch.from_numpy(detgen.smooth_frames("smooth", (F, 3, H, W), 7))
    cw = torch.from_numpy(detgen.uniform("cwe2e", (F, 512), 0.5, 1.5))
    m = _r3m(size, sd)
    xg = x.to(DEV).requires_grad_(True)
    (m(xg, obs_shape=[3, H, W]) * cw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    errs = []
    for dtype in (torch.float64, torch.float32):
        ref = resnet_ref.resnet18().to(dtype)
        ref.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}, strict=False)
        ref.eval()
        xv = x.detach().to(dtype).clone().requires_grad_(True)
        (_enc(ref, _resize_ref(xv, H, W)) * cw.to(dtype)).sum().backward()
        errs.append(xv.grad.double())
    e_hip, e_cpu = l2rel(xg.grad, errs[0]), l2rel(errs[1], errs[0])
    report(f"R3M.forward 240x320 obs.grad: l2-rel vs float64 hip {e_hip:.3e} torch-cpu-fp32 {e_cpu:.3e}")
    assert e_hip <= max(4.0 * e_cpu, 1e-4), (e_hip, e_cpu)


def test_language_reward_pixel_gradient(hip):
    """d get_reward(r3m(obs0), r3m(obs), language features) / d obs: pixel gradients of the language reward."""
    from oracle import detgen, r3m_ref, resnet_ref
    from r3m_amd.models_language import LanguageReward
    size, F = 18, 2
    sd = _state(size, "w")
    m = _r3m(size, sd, max_live_forwards=2)
    torch.manual_seed(11)
    rew = LanguageReward(None, 512, 64, 768)
    lsd = {k: v.clone() for k, v in rew.state_dict().items()}
    rew = rew.to(DEV)
    x0 = torch.from_numpy(detgen.smooth_frames("smooth", (F, 3, 224, 224), 7))
    x1 = torch.from_numpy(detgen.smooth_frames("smoothb", (F, 3, 224, 224), 7))
    le = torch.from_numpy(detgen.uniform("langfeat", (F, 768), -0.6, 0.6))
    xg = x1.to(DEV).requires_grad_(True)
    rew(m(x0.to(DEV)), m(xg), le.to(DEV))[0].sum().backward()
    torch.cuda.synchronize()
    out = []
    for dtype in (torch.float64, torch.float32):
        enc = resnet_ref.resnet18().to(dtype)
        enc.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}, strict=False)
        enc.eval()
        lr = r3m_ref.LanguageRewardRef(512, 64, 768).to(dtype)
        lr.load_state_dict({k: v.to(dtype) for k, v in lsd.items()})
        xv = x1.detach().to(dtype).clone().requires_grad_(True)
        norm = lambda v: (v / 255.0 - MEAN.to(dtype)) / STD.to(dtype)
        lr(_enc(enc, norm(x0.to(dtype))), _enc(enc, norm(xv)), le.to(dtype)).sum().backward()
        out.append(xv.grad.double())
    e_hip, e_cpu = l2rel(xg.grad, out[0]), l2rel(out[1], out[0])
    report(f"language reward pixel gradient: l2-rel vs float64 hip {e_hip:.3e} torch-cpu-fp32 {e_cpu:.3e}")
    assert e_hip <= max(4.0 * e_cpu, 1e-4), (e_hip, e_cpu)


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------------
def test_input_grad_errors(hip):
    from r3m_amd import _lib
    from r3m_amd.encoder import HipResNet
    enc = HipResNet(18).to(DEV)
    p = enc.flat_params()
    b = enc._flat_b
    h = hip.r3m_resnet_create(18, 1)
    assert h
    try:
        arena = torch.empty(hip.r3m_resnet_arena_bytes(h), dtype=torch.uint8, device=DEV)
        out = torch.empty(1, 512, device=DEV)
        dh = torch.ones(1, 512, device=DEV)
        dx = torch.empty(1, 3, 224, 224, device=DEV)
        x = torch.rand(1, 3, 224, 224, device=DEV) * 255
        s = _stream()
        # inference-mode forward: nothing kept
        assert hip.r3m_resnet_forward(h, x.data_ptr(), p.data_ptr(), b.data_ptr(), arena.data_ptr(), out.data_ptr(), 2, s) == 0
        assert hip.r3m_resnet_backward_ex(h, dh.data_ptr(), p.data_ptr(), None, arena.data_ptr(), 0, 4, 0, dx.data_ptr(), 0, s) != 0
        assert "inference" in _lib.last_error()
        # crop forward: no frames to differentiate
        raw = (torch.rand(1, 3, 240, 320, device=DEV) * 255).to(torch.uint8)
        boxes = torch.tensor([[0, 0, 240, 320]], dtype=torch.int32, device=DEV)
        assert hip.r3m_resnet_forward_crop(h, raw.data_ptr(), 1, boxes.data_ptr(), 1, 240, 320, p.data_ptr(), b.data_ptr(),
                                           arena.data_ptr(), out.data_ptr(), 1, s) == 0
        assert hip.r3m_resnet_backward_ex(h, dh.data_ptr(), p.data_ptr(), None, arena.data_ptr(), 0, 4, 0, dx.data_ptr(), 0, s) != 0
        assert "forward_crop" in _lib.last_error()
        # the same plan still runs a parameter-free backward without dx after the crop forward, and one with dx after a plain forward
        assert hip.r3m_resnet_backward_ex(h, dh.data_ptr(), p.data_ptr(), None, arena.data_ptr(), 0, 4, 0, None, 0, s) == 0
        assert hip.r3m_resnet_forward(h, x.data_ptr(), p.data_ptr(), b.data_ptr(), arena.data_ptr(), out.data_ptr(), 0, s) == 0
        assert hip.r3m_resnet_backward_ex(h, dh.data_ptr(), p.data_ptr(), None, arena.data_ptr(), 0, 4, 0, dx.data_ptr(), 0, s) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(dx).all()
    finally:
        hip.r3m_resnet_destroy(h)
