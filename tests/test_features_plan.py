"""not gpu: the host side of the spatial feature maps (convnet.layer1..layer4 of the reference's torchvision ResNet,
models_r3m.py:44-52): the geometry query, the new symbols, and every argument check that must answer before a launch."""
import ctypes as C

import pytest
import torch


def _lib():
    from r3m_amd import _lib
    return _lib, _lib.lib()


def _feature_info(L, h, layer):
    c, hh, ww = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = L.r3m_resnet_feature_info(h, layer, C.byref(c), C.byref(hh), C.byref(ww))
    return rc, (c.value, hh.value, ww.value)


def _conv_table(L, h):
    """[(Co, Ho, Wo)] of every convolution, and the index of the last convolution of the main path of each stage's last block"""
    name = C.create_string_buffer(128)
    convs = []           # names of the convolutions in r3m_resnet_conv_info order (tensor table: five tensors per convolution)
    for i in range(0, L.r3m_resnet_num_tensors(h), 5):
        assert L.r3m_resnet_tensor_info(h, i, name, 128, None, None, None, None) == 0
        convs.append(name.value.decode()[:-len(".weight")])
    geo = []
    for i in range(L.r3m_resnet_num_convs(h)):
        v = [C.c_int() for _ in range(9)]
        assert L.r3m_resnet_conv_info(h, i, *[C.byref(x) for x in v]) == 0
        geo.append((v[1].value, v[7].value, v[8].value))
    last = {}
    for i, n in enumerate(convs):
        if n.startswith("layer") and "downsample" not in n:
            last[int(n[5])] = i          # the highest-indexed main-path convolution of layerK: conv2 / conv3 of its last block
    return geo, last


@pytest.mark.parametrize("size", [18, 34, 50])
@pytest.mark.parametrize("hw", [(224, 224), (32, 32), (97, 130)])
def test_feature_info_matches_last_convolution(size, hw):
    _, L = _lib()
    h = L.r3m_resnet_create_hw(size, 3, 0, hw[0], hw[1])
    assert h
    try:
        geo, last = _conv_table(L, h)
        for layer in (1, 2, 3, 4):
            rc, got = _feature_info(L, h, layer)
            assert rc == 0
            assert got == geo[last[layer]], (layer, got, geo[last[layer]])
            assert got[0] == (64 << (layer - 1)) * (4 if size == 50 else 1)
        if hw == (32, 32):
            assert _feature_info(L, h, 4)[1][1:] == (1, 1)
        if hw == (224, 224):
            assert [_feature_info(L, h, k)[1][1:] for k in (1, 2, 3, 4)] == [(56, 56), (28, 28), (14, 14), (7, 7)]
    finally:
        L.r3m_resnet_destroy(h)


def test_feature_info_rejects_layers_outside_1_to_4():
    lib, L = _lib()
    h = L.r3m_resnet_create(18, 1)
    try:
        for layer in (0, 5):
            rc, _ = _feature_info(L, h, layer)
            assert rc != 0
            assert f"layer {layer}" in lib.last_error()
    finally:
        L.r3m_resnet_destroy(h)


def test_symbols_and_abi_version():
    lib, L = _lib()
    for name in ("r3m_resnet_feature_info", "r3m_resnet_forward_features", "r3m_resnet_backward_features", "r3m_feature_export_dt",
                 "r3m_feature_grad_add_dt"):
        assert hasattr(L, name) and name in lib.SIGNATURES, name
    assert L.r3m_abi_version() == 1


@pytest.mark.parametrize("fn", ["r3m_feature_export_dt", "r3m_feature_grad_add_dt"])
def test_kernel_entry_points_check_their_arguments(fn):
    """bad C, bad dtype, non-positive sizes: non-zero with a message, before any launch (the pointers are never read)"""
    lib, L = _lib()
    f = getattr(L, fn)
    a, b = 4096, 8192           # stand-ins for device pointers
    for (N, H, W, Cc, dt), word in [((1, 7, 7, 96, 0), "C=96"), ((1, 7, 7, 0, 0), "C=0"), ((1, 7, 7, 32, 1), "C=32"),
                                    ((1, 7, 7, 64, 2), "dtype"), ((1, 7, 7, 64, -1), "dtype"),
                                    ((0, 7, 7, 64, 0), "N=0"), ((1, 0, 7, 64, 1), "H=0"), ((1, 7, -3, 64, 0), "W=-3")]:
        assert f(a, b, N, H, W, Cc, dt, None) != 0, (N, H, W, Cc, dt)
        assert word in lib.last_error(), (word, lib.last_error())
    # alignment: the NHWC side moves 16 bytes at a time always, the NCHW side only when H * W = 1 (same bytes in both layouts)
    nhwc, nchw = (a, b) if fn == "r3m_feature_export_dt" else (b, a)
    order = (lambda x, y: (x, y)) if fn == "r3m_feature_export_dt" else (lambda x, y: (y, x))
    for x, y, hw in [(nhwc + 8, nchw, 7), (nhwc, nchw + 4, 1)]:
        assert f(*order(x, y), 1, hw, hw, 64, 0, None) != 0
        assert "16-byte aligned" in lib.last_error(), lib.last_error()


def test_forward_features_rejects_unknown_and_duplicate_layers():
    from r3m_amd.encoder import HipResNet
    m = HipResNet(18)
    x = torch.zeros(1, 3, 64, 96)        # never reaches the GPU: the names are checked first
    with pytest.raises(ValueError, match="unknown layer"):
        m.forward_features(x, layers=("layer2", "layer5"))
    with pytest.raises(ValueError, match="unknown layer"):
        m.forward_features(x, layers=("fc",))
    with pytest.raises(ValueError, match="twice"):
        m.forward_features(x, layers=("layer3", "layer1", "layer3"))


def test_r3m_module_exposes_forward_features():
    from r3m_amd import R3M
    m = R3M("cpu", 1e-4, 64, size=18, langweight=0.0)
    with pytest.raises(ValueError, match="unknown layer"):
        m.forward_features(torch.zeros(1, 3, 224, 224), layers=("layer0",))
