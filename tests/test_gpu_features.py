"""Differentiable spatial feature maps (the outputs of convnet.layer1..layer4 of the reference's torchvision ResNet,
models_r3m.py:44-52): the export / gradient-import kernels one by one, the engine's injection points through the C ABI, and the
autograd surface (HipResNet.forward_features / R3M.forward_features).

Comparators: the pinned oracle (oracle/resnet_ref.py) in float64 on the CPU with forward hooks on its layer1..layer4. The parity gate
is the one of tests/test_gpu_input_grad.py (_gate): err(X) = ||X - fp64|| / ||fp64||; the median over three (weights, frames) draws of
err(HIP) / err(torch CPU of the same graph) must be <= 2, every draw <= 4, an error at or below 1e-4 always passes. fp32 plans compare
against torch-CPU-fp32, bf16 plans against torch.autocast("cpu", bfloat16). Frames are 64 x 96, three per draw, unless a case says so.
The two kernels are checked bit for bit against the torch expressions they replace."""
import contextlib
import functools

import pytest
import torch

from test_gpu_input_grad import DEV, DRAWS, MEAN, STD, _enc, _gate, _hip_encoder, _state, _stream, l2rel, report

pytestmark = pytest.mark.gpu
ALL = ("layer1", "layer2", "layer3", "layer4")
# conv1, one weight per stage, one BatchNorm weight (at or below layer2, so that a layer2-only loss reaches it too)
PSAMPLE = ("conv1.weight", "layer1.0.conv1.weight", "layer2.0.conv1.weight", "layer3.0.conv1.weight", "layer4.0.conv1.weight",
           "layer2.0.bn1.weight")
F, HW = 3, (64, 96)


# ---- 1. the kernels one by one --------------------------------------------------------------------------------------------------
# the issue's shapes; 63 / 65 pixels: one below and one above the kernel's 64-pixel tile (65 -> two tiles of 33 and 32);
# 200 pixels with N = 2: four tiles of 50
KERNEL_SHAPES = [(1, 1, 1, 64), (3, 1, 1, 2048), (2, 7, 7, 512), (1, 7, 7, 2048), (2, 4, 5, 64), (1, 3, 5, 256), (1, 9, 15, 128),
                 (1, 7, 9, 64), (1, 5, 13, 64), (2, 10, 20, 128)]
GUARD = 64          # elements on either side of an output buffer


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill):
    ref = torch.full((GUARD,), fill, dtype=buf.dtype, device=DEV)
    return torch.equal(buf[:GUARD], ref) and torch.equal(buf[GUARD + n:], ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_feature_export_kernel(hip, shape, dtype):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    z = torch.randn(N, H, W, C, generator=g).to(dtype).to(DEV)
    n = z.numel()
    buf, out = _guarded(n, torch.float32, -7.25)
    assert hip.r3m_feature_export_dt(z.data_ptr(), out.data_ptr(), N, H, W, C, 1 if dtype == torch.bfloat16 else 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(N, C, H, W), z.permute(0, 3, 1, 2).float())
    assert _guards_intact(buf, n, -7.25)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_feature_grad_add_kernel(hip, shape, dtype):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(1000 + sum(shape))
    g0 = torch.randn(N, H, W, C, generator=g).to(dtype).to(DEV)
    d = torch.randn(N, C, H, W, generator=g).to(DEV)
    n = g0.numel()
    buf, gg = _guarded(n, dtype, 3.5)
    gg.copy_(g0.reshape(-1))
    expect = (g0.float() + d.permute(0, 2, 3, 1)).to(dtype)
    d_before = d.clone()
    assert hip.r3m_feature_grad_add_dt(d.data_ptr(), gg.data_ptr(), N, H, W, C, 1 if dtype == torch.bfloat16 else 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gg.view(N, H, W, C), expect)
    assert _guards_intact(buf, n, 3.5)
    assert torch.equal(d, d_before)


# ---- references ------------------------------------------------------------------------------------------------------------------
def _frames(ftag, hw=HW, frames=F):
    from oracle import detgen
    return torch.from_numpy(detgen.smooth_frames(ftag, (frames, 3) + tuple(hw), 7))


def _weights(ftag, name, shape):
    from oracle import detgen
    return torch.from_numpy(detgen.uniform(f"cw{name}{ftag}", tuple(shape), 0.5, 1.5))


def _loss(h, maps, ftag, use):
    """(h * cw).sum() + sum_k (map_k * cw_k).sum() over the terms named in `use` ("h", "layer1", ...)"""
    total = 0.0
    if "h" in use:
        total = total + (h * _weights(ftag, "h", h.shape).to(device=h.device, dtype=h.dtype)).sum()
    for name in ALL:
        if name in use:
            v = maps[name]
            v = v.float() if v.dtype == torch.bfloat16 else v
            total = total + (v * _weights(ftag, name, v.shape).to(device=v.device, dtype=v.dtype)).sum()
    return total


@functools.lru_cache(maxsize=None)
def _ref(size, wtag, ftag, train, mode, use, hw=HW, frames=F):
    """The oracle on the CPU: mode "f64" / "f32" / "autocast". Returns (h, {maps}, obs.grad, {sampled parameter gradients})."""
    from oracle import resnet_ref
    dtype = torch.float64 if mode == "f64" else torch.float32
    m = getattr(resnet_ref, f"resnet{size}")().to(dtype)
    m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in _state(size, wtag).items()}, strict=False)
    m.train(train)
    maps = {}
    for name in ALL:
        getattr(m, name).register_forward_hook(lambda mod, inp, out, name=name: maps.__setitem__(name, out))
    xv = _frames(ftag, hw, frames).to(dtype).requires_grad_(True)
    xn = (xv / 255.0 - MEAN.to(dtype)) / STD.to(dtype)
    with torch.autocast("cpu", dtype=torch.bfloat16) if mode == "autocast" else contextlib.nullcontext():
        h = _enc(m, xn)
    h = h.float() if mode == "autocast" else h
    _loss(h, maps, ftag, use).backward()
    params = dict(m.named_parameters())
    pg = {k: params[k].grad.detach().double() for k in PSAMPLE if params[k].grad is not None}
    return h.detach().double(), {k: v.detach().double() for k, v in maps.items()}, xv.grad.detach().double(), pg


USE_ALL = ("h",) + ALL


def _hip_run(m, ftag, use, layers=ALL, hw=HW, input_grad=True, frames=F):
    xg = _frames(ftag, hw, frames).to(DEV).requires_grad_(input_grad)
    h, maps = m.forward_features(xg, layers)
    _loss(h, maps, ftag, use).backward()
    torch.cuda.synchronize()
    return h.detach(), {k: v.detach() for k, v in maps.items()}, xg.grad


def _gate_all(name, per_key):
    for key, pairs in per_key.items():
        _gate(f"{name} {key}", pairs)


CASES = [(18, True, "fp32"), (18, False, "fp32"), (50, True, "fp32"), (50, False, "fp32"), (18, True, "bf16"), (50, True, "bf16")]
CASE_IDS = [f"r{s}-{'train' if t else 'eval'}-{p}" for s, t, p in CASES]


# ---- 2. forward parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,train,precision", CASES, ids=CASE_IDS)
def test_forward_parity(hip, size, train, precision):
    cmp_mode = "autocast" if precision == "bf16" else "f32"
    per = {k: [] for k in ALL}
    for wtag, ftag in DRAWS:
        sd = _state(size, wtag)
        m, twin = _hip_encoder(size, sd, train, precision=precision), _hip_encoder(size, sd, train, precision=precision)
        x = _frames(ftag).to(DEV)
        h, maps = m.forward_features(x)
        h2 = twin(x)
        torch.cuda.synchronize()
        assert torch.equal(h, h2)
        assert torch.equal(m._flat_b, twin._flat_b) and torch.equal(m._flat_nbt, twin._flat_nbt)     # running statistics
        _, m64, _, _ = _ref(size, wtag, ftag, train, "f64", USE_ALL)
        _, mcmp, _, _ = _ref(size, wtag, ftag, train, cmp_mode, USE_ALL)
        for k in ALL:
            assert maps[k].dtype == torch.float32 and tuple(maps[k].shape) == tuple(m64[k].shape) and maps[k].is_contiguous()
            per[k].append((l2rel(maps[k], m64[k]), l2rel(mcmp[k], m64[k])))
    _gate_all(f"features forward {size} {'train' if train else 'eval'} {precision}", per)


# ---- 3. inference and subsets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [18, 50])
def test_inference_maps(hip, size, precision):
    """no_grad in eval mode runs the fused inference forward, whose identity blocks overwrite their input: the maps are taken behind
    each stage's last block. fp32: the fused path is bit-identical to the eval forward; bf16: within the 1e-2 the project states."""
    m = _hip_encoder(size, _state(size, "w"), False, precision=precision)
    x = _frames("smooth").to(DEV)
    h, maps = m.forward_features(x)
    assert h.requires_grad and all(v.requires_grad for v in maps.values())
    with torch.no_grad():
        hi, mi = m.forward_features(x)
    torch.cuda.synchronize()
    assert not hi.requires_grad and not any(v.requires_grad for v in mi.values())
    for k in ALL:
        e = l2rel(mi[k], maps[k])
        report(f"inference maps r{size} {precision} {k}: l2-rel vs eval-with-grad {e:.3e}")
        if precision == "fp32":
            assert torch.equal(mi[k], maps[k]), k
        else:
            assert e <= 1e-2, (k, e)


@pytest.mark.parametrize("mode", ["train", "inference"])
def test_subset_request(hip, mode):
    m = _hip_encoder(50, _state(50, "w"), mode == "train")
    x = _frames("smooth").to(DEV)
    with torch.no_grad() if mode == "inference" else contextlib.nullcontext():
        _, four = m.forward_features(x)
        m.load_state_dict(_state(50, "w"), strict=False)        # (train mode moved the running statistics)
        h, one = m.forward_features(x, layers=("layer3",))
    torch.cuda.synchronize()
    assert list(one) == ["layer3"] and torch.equal(one["layer3"], four["layer3"])
    assert list(four) == list(ALL)


# ---- 4. backward -----------------------------------------------------------------------------------------------------------------
# ResNet-50, train mode, fp32 needs larger frames than 64 x 96. With a dense loss on the maps ONE fp32 ReLU decision that falls the
# other way in float64 moves obs.grad by 3e-4 .. 2e-3 at these sizes (torch-CPU-fp32 on draw 0 at 64 x 96: exactly one of the millions of
# ReLU inputs differs in sign, layer2.0, -2.8e-7 in float64 and +2.3e-7 in fp32, and the error is 3.4e-4 where the other draws have
# 5.7e-6 and 5.2e-6). Such a flip happens zero to a few times per draw on any small frame: the COMPARATOR's own worst error over the
# gated tensors, no HIP code involved, is 1.7e-3, 5.7e-6, 5.2e-6 (64 x 96), 5.8e-6, 3.9e-4, 7.0e-6 (64 x 64), 4.2e-3, 7.8e-6, 8.5e-6
# (48 x 64), and still one flip against none at 128 x 160 — a ratio of two such errors measures luck, not the code. The case
# therefore runs where tests/test_gpu_input_grad.py gates this network in train mode, for the reason its docstring gives: 224 x 224
# frames, 3, 8 and 8 of them on the three draws. There every draw has enough flips for the error to be a statistic: the comparator's
# obs.grad error is 8.8e-3, 7.4e-3, 5.3e-3 for the h + maps loss and 2.4e-3, 5.5e-3, 2.8e-3 for layer2 only, and on the 8-frame draws
# its parameter-gradient errors are 7.5e-5 .. 7.9e-4. (With 3 frames on every draw one flip more or less still decided single
# tensors: conv1.weight under the layer2-only loss, draw 1: HIP 1.12e-4 just above the 1e-4 floor, torch 6.6e-6, ratio 16.9, while
# obs.grad and the other tensors of that draw had ratios 0.9 .. 1.1.) ResNet-18 and eval mode are at 1e-6 on every draw at 64 x 96.
BACKWARD_SHAPE = {(50, True, "fp32"): ((224, 224), (3, 8, 8))}


@pytest.mark.parametrize("use", [USE_ALL, ("layer2",)], ids=["h+maps", "layer2-only"])
@pytest.mark.parametrize("size,train,precision", CASES[:5], ids=CASE_IDS[:5])
def test_backward_parity(hip, size, train, precision, use):
    """obs.grad and a sample of parameter gradients of (h * cw).sum() + sum_k (map_k * cw_k).sum(); layer2-only: the embedding gets no
    gradient (dh == NULL) and the stages above layer2 run on zeros."""
    cmp_mode = "autocast" if precision == "bf16" else "f32"
    hw, counts = BACKWARD_SHAPE.get((size, train, precision), (HW, (F, F, F)))
    per = {}
    for (wtag, ftag), n in zip(DRAWS, counts):
        m = _hip_encoder(size, _state(size, wtag), train, precision=precision)
        _, _, gx = _hip_run(m, ftag, use, hw=hw, frames=n)
        _, _, gx64, pg64 = _ref(size, wtag, ftag, train, "f64", use, hw, n)
        _, _, gxc, pgc = _ref(size, wtag, ftag, train, cmp_mode, use, hw, n)
        assert torch.isfinite(gx).all()
        per.setdefault("obs.grad", []).append((l2rel(gx, gx64), l2rel(gxc, gx64)))
        params = dict(m.named_parameters())
        for k in PSAMPLE:
            if k in pg64:
                per.setdefault(k, []).append((l2rel(params[k].grad, pg64[k]), l2rel(pgc[k], pg64[k])))
            else:                                   # above the only map the loss used: autograd leaves None, the engine ran on zeros
                assert float(params[k].grad.abs().max()) == 0.0, k
    assert len(per) >= 4
    _gate_all(f"features backward {size} {'train' if train else 'eval'} {precision} {'+'.join(use)}", per)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("input_grad", [False, True], ids=["params", "params+obs"])
def test_unused_maps_change_nothing(hip, precision, input_grad):
    """forward_features followed by a loss on h alone: the same bits in the flat gradient buffer as forward()"""
    sd = _state(18, "w")
    a, b = _hip_encoder(18, sd, True, precision=precision), _hip_encoder(18, sd, True, precision=precision)
    xa = _frames("smooth").to(DEV).requires_grad_(input_grad)
    xb = xa.detach().clone().requires_grad_(input_grad)
    _loss(a(xa), {}, "smooth", ("h",)).backward()
    h, maps = b.forward_features(xb)
    _loss(h, maps, "smooth", ("h",)).backward()
    torch.cuda.synchronize()
    assert torch.equal(a.flat_grads(), b.flat_grads())
    assert float(a.flat_grads().abs().max()) > 0
    if input_grad:
        assert torch.equal(xa.grad, xb.grad)


# ---- 5. partial freeze -----------------------------------------------------------------------------------------------------------
def test_frozen_prefix_drops_the_map_gradient(hip):
    """only layer4.* trainable, no input gradient: layer2's block has no work, so a layer2 term in the loss changes nothing"""
    sd = _state(18, "w")
    flats = []
    for use in (("h",), ("h", "layer2")):
        m = _hip_encoder(18, sd, True)
        for k, p in m.named_parameters():
            p.requires_grad_(k.startswith("layer4."))
        _hip_run(m, "smooth", use, input_grad=False)
        flats.append(m.flat_grads().clone())
        params = dict(m.named_parameters())
        assert params["conv1.weight"].grad is None and params["layer4.0.conv1.weight"].grad is not None
    assert torch.equal(flats[0], flats[1])
    assert float(flats[0].abs().max()) > 0


def test_frozen_encoder_layer2_only_obs_grad(hip):
    per = []
    for wtag, ftag in DRAWS:
        m = _hip_encoder(18, _state(18, wtag), False, frozen=True)
        _, _, gx = _hip_run(m, ftag, ("layer2",))
        _, _, gx64, _ = _ref(18, wtag, ftag, False, "f64", ("layer2",))
        _, _, gx32, _ = _ref(18, wtag, ftag, False, "f32", ("layer2",))
        assert all(p.grad is None for p in m.parameters()) and m._flat_g is None
        per.append((l2rel(gx, gx64), l2rel(gx32, gx64)))
    _gate("features frozen encoder, layer2-only loss", per)


# ---- 6. autograd semantics -------------------------------------------------------------------------------------------------------
def test_retain_graph_doubles_obs_grad(hip):
    m = _hip_encoder(18, _state(18, "w"), False)
    xg = _frames("smooth").to(DEV).requires_grad_(True)
    h, maps = m.forward_features(xg)
    loss = _loss(h, maps, "smooth", USE_ALL)
    loss.backward(retain_graph=True)
    first = xg.grad.clone()
    loss.backward()
    torch.cuda.synchronize()
    assert float(first.abs().max()) > 0 and torch.equal(xg.grad, first + first)


def test_max_live_forwards(hip):
    sd = _state(18, "w")
    m = _hip_encoder(18, sd, False, max_live_forwards=2)
    xa, xb = (_frames(t).to(DEV).requires_grad_(True) for t in ("smooth", "smoothb"))
    ha, ma = m.forward_features(xa)
    hb, mb = m.forward_features(xb, layers=("layer3",))
    (_loss(ha, ma, "smooth", USE_ALL) + _loss(hb, mb, "smoothb", ("h", "layer3"))).backward()
    torch.cuda.synchronize()
    solo = _hip_encoder(18, sd, False)
    _, _, ga = _hip_run(solo, "smooth", USE_ALL)
    assert torch.equal(xa.grad, ga) and float(xb.grad.abs().max()) > 0
    # one live forward: the second call overwrites the first one's activations, and its backward says so
    one = _hip_encoder(18, sd, False)
    h1, m1 = one.forward_features(xa)
    one.forward_features(xb)
    with pytest.raises(RuntimeError, match="max_live_forwards"):
        _loss(h1, m1, "smooth", USE_ALL).backward()


def test_cropped_clips_are_refused(hip):
    from r3m_amd.augment import CroppedClips
    m = _hip_encoder(18, _state(18, "w"), False)
    raw = (torch.rand(1, 3, 240, 320, device=DEV) * 255).to(torch.uint8)
    with pytest.raises(TypeError, match="CroppedClips"):
        m.forward_features(CroppedClips(raw, torch.tensor([[0, 0, 240, 320]], dtype=torch.int32), 1))


def test_r3m_forward_features(hip):
    """R3M.forward_features takes the Resize(256) + CenterCrop(224) branch of R3M.forward"""
    from test_gpu_input_grad import _r3m
    m = _r3m(18, _state(18, "w"), frozen=False)
    x = _frames("smooth", (240, 320), 2).to(DEV)
    h, maps = m.forward_features(x, layers=("layer4", "layer1"), obs_shape=[3, 240, 320])
    h2 = m(x, obs_shape=[3, 240, 320])
    torch.cuda.synchronize()
    assert torch.equal(h, h2)
    assert list(maps) == ["layer4", "layer1"] and maps["layer4"].shape == (2, 512, 7, 7) and maps["layer1"].shape == (2, 64, 56, 56)
    assert l2rel(maps["layer4"].mean((2, 3)), h) <= 1e-6


# ---- 7. the staged protocol through the C ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_staged_backward_carries_dfeats(hip, dtype):
    import ctypes as C
    from r3m_amd import _lib
    from r3m_amd.encoder import HipResNet
    Fr, H, W = 2, 64, 96
    enc = HipResNet(18)
    enc.load_state_dict(_state(18, "w"), strict=False)
    enc = enc.to(DEV)
    p, b = enc.flat_params(), enc._flat_b.clone()
    h = hip.r3m_resnet_create_hw(18, Fr, dtype, H, W)
    assert h
    try:
        arena = torch.empty(hip.r3m_resnet_arena_bytes(h), dtype=torch.uint8, device=DEV)
        x = _frames("smooth", (H, W), Fr).to(DEV)
        out = torch.empty(Fr, 512, device=DEV)
        shapes = [HipResNet._feature_shape(h, k) for k in range(4)]
        maps = [torch.empty((Fr,) + s, device=DEV) for s in shapes]
        g = torch.Generator().manual_seed(5)
        dmaps = [torch.randn((Fr,) + s, generator=g).to(DEV) if k != 2 else None for k, s in enumerate(shapes)]   # layer3: no gradient
        dh = torch.randn(Fr, 512, generator=g).to(DEV)
        feats = (C.c_void_p * 4)(*[t.data_ptr() for t in maps])
        dfeats = (C.c_void_p * 4)(*[_lib.ptr(t) for t in dmaps])
        s = _stream()
        args = (p.data_ptr(), b.data_ptr(), arena.data_ptr(), out.data_ptr())
        assert hip.r3m_resnet_forward_features(h, x.data_ptr(), *args, feats, 1, s) == 0, _lib.last_error()
        res = []
        for stages in ([(0, 4)], [(0, 1), (1, 2), (2, 3), (3, 4)]):
            grads, dx = torch.full_like(p, float("nan")), torch.full_like(x, float("nan"))
            for s0, s1 in stages:
                assert hip.r3m_resnet_backward_features(h, dh.data_ptr(), dfeats, p.data_ptr(), grads.data_ptr(), arena.data_ptr(), s0, s1, 0,
                                                        dx.data_ptr(), 0, s) == 0, _lib.last_error()
            torch.cuda.synchronize()
            assert torch.isfinite(grads).all() and torch.isfinite(dx).all()
            res.append((grads, dx))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        # the maps' gradients did arrive: without them the input gradient differs
        dx0 = torch.empty_like(x)
        assert hip.r3m_resnet_backward_features(h, dh.data_ptr(), None, p.data_ptr(), None, arena.data_ptr(), 0, 4, 0, dx0.data_ptr(), 0, s) == 0
        torch.cuda.synchronize()
        assert not torch.equal(dx0, res[0][1])
        # an inference-mode forward keeps nothing
        assert hip.r3m_resnet_forward_features(h, x.data_ptr(), *args, feats, 2, s) == 0, _lib.last_error()
        assert hip.r3m_resnet_backward_features(h, dh.data_ptr(), dfeats, p.data_ptr(), None, arena.data_ptr(), 0, 4, 0, dx0.data_ptr(), 0, s) != 0
        assert "inference mode" in _lib.last_error()
        torch.cuda.synchronize()
    finally:
        hip.r3m_resnet_destroy(h)


# ---- 8. native resolution --------------------------------------------------------------------------------------------------------
def test_native_resolution(hip):
    """97 x 130 frames: maps of 25 x 33, 13 x 17, 7 x 9 and 4 x 5 pixels (none a multiple of the kernels' tile)"""
    hw = (97, 130)
    per = {}
    for wtag, ftag in DRAWS:
        m = _hip_encoder(18, _state(18, wtag), True)
        _, maps, gx = _hip_run(m, ftag, USE_ALL, hw=hw)
        _, m64, gx64, _ = _ref(18, wtag, ftag, True, "f64", USE_ALL, hw)
        _, m32, gx32, _ = _ref(18, wtag, ftag, True, "f32", USE_ALL, hw)
        assert [tuple(maps[k].shape[2:]) for k in ALL] == [(25, 33), (13, 17), (7, 9), (4, 5)]
        for k in ALL:
            per.setdefault(k, []).append((l2rel(maps[k], m64[k]), l2rel(m32[k], m64[k])))
        per.setdefault("obs.grad", []).append((l2rel(gx, gx64), l2rel(gx32, gx64)))
    _gate_all("features 97x130 r18 train fp32", per)
