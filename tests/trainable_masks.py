"""Shared by the trainable-mask tests (CPU plan table, GPU engine and module tests): the plan's tensor table through the C ABI and the
trainable masks of the usual fine-tuning recipes, as sets of tensor names."""
import ctypes as C
import re


def tensors(lib, h):
    name = C.create_string_buffer(128)
    kind, ndim, off, shape = C.c_int(), C.c_int(), C.c_longlong(), (C.c_int * 4)()
    out = []
    for i in range(lib.r3m_resnet_num_tensors(h)):
        assert lib.r3m_resnet_tensor_info(h, i, name, 128, C.byref(kind), C.byref(off), C.byref(ndim), shape) == 0
        out.append((name.value.decode(), kind.value))
    return out


def conv_names(tensors):
    """convolutions in r3m_resnet_conv_info order = the kind-0 tensors in table order; (conv prefix, its BatchNorm prefix)"""
    convs = []
    for i, (n, k) in enumerate(tensors):
        if k == 0:
            conv = n[:-len(".weight")]
            bn = tensors[i + 1][0][:-len(".weight")]
            assert tensors[i + 1][1] == 1 and tensors[i + 2] == (bn + ".bias", 2)
            convs.append((conv, bn))
    return convs


def _param_names(tensors):
    return [n for n, k in tensors if k <= 2]


def _last_block(tensors):
    return sorted({re.match(r"(layer4\.\d+)\.", n).group(1) for n, k in tensors if n.startswith("layer4.")})[-1]


def masks(tensors):
    """name -> set of trainable tensor names (the masks the issue lists)"""
    P = _param_names(tensors)
    lb = _last_block(tensors)
    last_conv = sorted(n for n in P if n.startswith(lb + ".conv"))[-1][:-len(".weight")]     # e.g. layer4.1.conv2
    last_bn = last_conv.replace("conv", "bn")
    masks = {
        "all": set(P),
        "none": set(),
        "layer4": {n for n in P if n.startswith("layer4.")},
        "bn_only": {n for n, k in tensors if k in (1, 2)},
        "convs_only": {n for n, k in tensors if k == 0},
        "layer1.0.conv1": {"layer1.0.conv1.weight"},
        "stem_conv": {"conv1.weight"},
        "last_conv_and_bn": {last_conv + ".weight", last_bn + ".weight", last_bn + ".bias"},
    }
    for K in (2, 3, 4):      # from layerK.1 on: an identity frontier block
        masks[f"from_layer{K}.1"] = {n for n in P if re.match(r"layer(\d)\.(\d+)\.", n) and
                                     (int(n[5]), int(n.split(".")[1])) >= (K, 1)}
    return masks


def mask_bytes(tensors, trainable):
    # BatchNorm buffers (kinds 3, 4) get a 1 on purpose: their entries are ignored
    return bytes(1 if (k >= 3 or n in trainable) else 0 for n, k in tensors)


def tensor_ranges(lib, h):
    """[(name, kind, offset, count)] of the plan's tensors (offsets into the flat parameter / gradient buffer for kinds 0-2)"""
    name = C.create_string_buffer(128)
    kind, ndim, off, shape = C.c_int(), C.c_int(), C.c_longlong(), (C.c_int * 4)()
    out = []
    for i in range(lib.r3m_resnet_num_tensors(h)):
        assert lib.r3m_resnet_tensor_info(h, i, name, 128, C.byref(kind), C.byref(off), C.byref(ndim), shape) == 0
        n = 1
        for k in range(ndim.value):
            n *= shape[k]
        out.append((name.value.decode(), kind.value, off.value, n))
    return out
