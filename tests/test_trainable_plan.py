"""not gpu: the backward schedule under a trainable mask (partial-freeze fine-tuning). r3m_debug_backward_plan reports, per
convolution, the work bits computed by the predicate r3m_resnet_backward executes (BN_SUMS 1, BN_APPLY 2, DGRAD 4, WGRAD 8);
here they are checked against an independent restatement of the rules, written from the block structure that the tensor NAMES
spell out (not from the engine's block table), for ResNet-18/34/50 and the masks of the usual fine-tuning recipes, with and without
the input gradient. Also: argument errors of the mask entry points and the host-side rejects of the ranged optimizer steps."""
import ctypes as C
import re

import pytest

from trainable_masks import conv_names as _conv_names, mask_bytes as _mask_bytes, masks as _masks, tensors as _tensors

SUMS, APPLY, DGRAD, WGRAD = 1, 2, 4, 8
SIZES = [18, 34, 50]


@pytest.fixture(scope="module")
def lib():
    from r3m_amd import _lib
    return _lib.lib()


def _expected(tensors, trainable, want_dx):
    """The rules of the issue, restated over names. trainable: set of tensor names that want a gradient."""
    convs = _conv_names(tensors)
    T = lambda c: (c[0] + ".weight") in trainable
    Tg = lambda c: (c[1] + ".weight") in trainable or (c[1] + ".bias") in trainable
    any_t = lambda c: T(c) or Tg(c)

    def bits(c, dgrad):
        wgrad = T(c)
        apply = dgrad or wgrad
        sums = apply or Tg(c)
        return SUMS * sums + APPLY * apply + DGRAD * dgrad + WGRAD * wgrad

    # group into stem + blocks ("layerL.B")
    blocks, order = {}, []
    for ci, c in enumerate(convs):
        m = re.match(r"(layer\d+\.\d+)\.(conv(\d)|downsample\.0)$", c[0])
        key = m.group(1) if m else "stem"
        if key not in blocks:
            blocks[key] = {"main": [], "ds": None}
            order.append(key)
        if m and m.group(2).startswith("downsample"):
            blocks[key]["ds"] = ci
        else:
            blocks[key]["main"].append(ci)
    assert order[0] == "stem" and blocks["stem"]["main"] == [0]
    exp = [None] * len(convs)
    exp[0] = bits(convs[0], want_dx)
    seen_below = want_dx or any_t(convs[0])             # below(first block)
    for key in order[1:]:
        b = blocks[key]
        below = seen_below
        for j, ci in enumerate(b["main"]):
            earlier = any(any_t(convs[cj]) for cj in b["main"][:j])
            exp[ci] = bits(convs[ci], below or earlier)
        if b["ds"] is not None:
            exp[b["ds"]] = bits(convs[b["ds"]], below)
        members = b["main"] + ([b["ds"]] if b["ds"] is not None else [])
        seen_below = seen_below or any(any_t(convs[ci]) for ci in members)
    return exp


def _plan_flags(lib, h, want_dx):
    n = lib.r3m_resnet_num_convs(h)
    out = (C.c_int * n)()
    assert lib.r3m_debug_backward_plan(h, int(want_dx), out, n) == n
    return list(out)


@pytest.mark.parametrize("want_dx", [False, True], ids=["nodx", "dx"])
@pytest.mark.parametrize("size", SIZES)
def test_backward_plan_matches_the_rules(lib, size, want_dx):
    h = lib.r3m_resnet_create(size, 2)
    assert h
    try:
        tensors = _tensors(lib, h)
        convs = _conv_names(tensors)
        assert len(convs) == lib.r3m_resnet_num_convs(h)
        for name, trainable in _masks(tensors).items():
            mask = _mask_bytes(tensors, trainable)
            assert lib.r3m_resnet_set_trainable(h, mask, len(mask)) == 0, name
            got = _plan_flags(lib, h, want_dx)
            exp = _expected(tensors, trainable, want_dx)
            assert got == exp, (size, name, [(c[0], g, e) for c, g, e in zip(convs, got, exp) if g != e])
    finally:
        lib.r3m_resnet_destroy(h)


@pytest.mark.parametrize("size", SIZES)
def test_backward_plan_landmarks(lib, size):
    """The properties the recipes rely on, spelled out (not through the restated rules)."""
    h = lib.r3m_resnet_create(size, 2)
    assert h
    try:
        tensors = _tensors(lib, h)
        convs = [c[0] for c in _conv_names(tensors)]
        masks = _masks(tensors)
        at = lambda flags, name: flags[convs.index(name)]

        def flags_of(mask_name, want_dx=False):
            mask = _mask_bytes(tensors, masks[mask_name])
            assert lib.r3m_resnet_set_trainable(h, mask, len(mask)) == 0
            return _plan_flags(lib, h, want_dx)

        # everything trainable: all four bits everywhere, except the stem's dgrad (= dx)
        f = flags_of("all")
        assert f[0] == SUMS | APPLY | WGRAD and all(x == 15 for x in f[1:])
        assert flags_of("all", True) == [15] * len(convs)
        # nothing trainable: no work without dx; with dx the dgrad chain without any wgrad (today's grads == NULL backward)
        assert flags_of("none") == [0] * len(convs)
        assert flags_of("none", True) == [SUMS | APPLY | DGRAD] * len(convs)
        # layer4 only: everything below layer4 has no work; the frontier block's conv1 and downsample get wgrad without dgrad
        f = flags_of("layer4")
        assert all(x == 0 for c, x in zip(convs, f) if not c.startswith("layer4."))
        assert at(f, "layer4.0.conv1") == SUMS | APPLY | WGRAD
        assert at(f, "layer4.0.downsample.0") == SUMS | APPLY | WGRAD
        assert at(f, "layer4.0.conv2") == 15 and at(f, "layer4.1.conv1") == 15
        # identity frontier block: its conv1 has no dgrad (no residual add into the frozen block before it)
        f = flags_of("from_layer3.1")
        assert at(f, "layer3.1.conv1") == SUMS | APPLY | WGRAD and at(f, "layer3.1.conv2") == 15
        assert all(x == 0 for c, x in zip(convs, f) if c == "conv1" or c.startswith(("layer1.", "layer2.", "layer3.0.")))
        # mid-block frontier: one convolution with work, every other one has none
        f = flags_of("last_conv_and_bn")
        assert sorted(f)[:-1] == [0] * (len(convs) - 1) and max(f) == SUMS | APPLY | WGRAD
        # BatchNorm only: the whole dgrad chain (down to the first block; the stem only forms its sums), no wgrad anywhere
        f = flags_of("bn_only")
        assert f[0] == SUMS and all(x == SUMS | APPLY | DGRAD for x in f[1:])
        # convs only: as all trainable (the BatchNorm sums are needed for dz anyway)
        assert flags_of("convs_only") == flags_of("all")
        # only layer1.0.conv1.weight: wgrad + the BatchNorm passes there, the dgrad chain above it, nothing in the stem or the
        # first block's downsample branch
        f = flags_of("layer1.0.conv1")
        assert f[0] == 0 and at(f, "layer1.0.conv1") == SUMS | APPLY | WGRAD
        if size == 50:
            assert at(f, "layer1.0.downsample.0") == 0
        assert all(x == SUMS | APPLY | DGRAD for c, x in zip(convs, f) if c not in ("conv1", "layer1.0.conv1", "layer1.0.downsample.0"))
        # only the stem's conv: its wgrad and the full chain
        f = flags_of("stem_conv")
        assert f[0] == SUMS | APPLY | WGRAD and all(x == SUMS | APPLY | DGRAD for x in f[1:])
    finally:
        lib.r3m_resnet_destroy(h)


def test_all_ones_mask_equals_null_mask_and_bad_arguments(lib):
    from r3m_amd import _lib
    h = lib.r3m_resnet_create(50, 1)
    assert h
    try:
        n = lib.r3m_resnet_num_tensors(h)
        nc = lib.r3m_resnet_num_convs(h)
        assert lib.r3m_resnet_set_trainable(h, None, 0) == 0
        null = [_plan_flags(lib, h, dx) for dx in (0, 1)]
        assert lib.r3m_resnet_set_trainable(h, bytes([1] * n), n) == 0
        assert [_plan_flags(lib, h, dx) for dx in (0, 1)] == null
        # a frozen mask, then NULL again restores the default
        assert lib.r3m_resnet_set_trainable(h, bytes(n), n) == 0
        assert _plan_flags(lib, h, 0) == [0] * nc
        assert lib.r3m_resnet_set_trainable(h, None, 0) == 0
        assert _plan_flags(lib, h, 0) == null[0]
        # wrong n: error, the mask in force is kept
        for bad in (n - 1, n + 1, 0):
            assert lib.r3m_resnet_set_trainable(h, bytes(n + 1), bad) != 0
            assert "tensors" in _lib.last_error()
        assert _plan_flags(lib, h, 0) == null[0]
        # cap too small / null output
        out = (C.c_int * nc)()
        assert lib.r3m_debug_backward_plan(h, 0, out, nc - 1) == -1
        assert "cap" in _lib.last_error()
        assert lib.r3m_debug_backward_plan(h, 0, None, nc) == -1
        assert lib.r3m_resnet_set_trainable(None, None, 0) != 0
        assert lib.r3m_abi_version() == 1
    finally:
        lib.r3m_resnet_destroy(h)


def _ll(v):
    return (C.c_longlong * len(v))(*v)


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_ranged_steps_reject_bad_ranges_on_the_host(lib, opt):
    """Misaligned, overlapping, unsorted ranges and step < 1 fail before anything is launched: the buffer pointers are never
    dereferenced (this machine needs no GPU for the call to return)."""
    from r3m_amd import _lib
    fake = 4096      # never dereferenced

    def call(off, count, step):
        n = len(off)
        if opt == "adam":
            return lib.r3m_adam_step_ranges(fake, fake, fake, fake, _ll(off), _ll(count), _ll(step), n, 1e-3, 0.9, 0.999, 1e-8, 1.0, None)
        return lib.r3m_sgd_step_ranges(fake, fake, fake, _ll(off), _ll(count), _ll(step), n, 1e-3, 0.9, 0.0, 0.0, 0, 1.0, None)

    bad = {
        "offset not a multiple of 4": ([2], [8], [1]),
        "count not a multiple of 4": ([0], [6], [1]),
        "second offset misaligned": ([0, 9], [8, 4], [1, 1]),
        "overlapping": ([0, 4], [8, 8], [1, 1]),
        "unsorted": ([16, 0], [4, 4], [1, 1]),
        "step 0": ([0], [4], [0]),
        "step -1 in the second range": ([0, 8], [4, 4], [3, -1]),
        "negative offset": ([-4], [4], [1]),
    }
    for what, (off, count, step) in bad.items():
        assert call(off, count, step) != 0, what
        assert f"{opt}_ranges" in _lib.last_error(), (what, _lib.last_error())
    # no range: nothing to launch, success
    assert call([], [], []) == 0
