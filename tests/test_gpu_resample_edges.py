"""-m gpu: the resampling kernels element by element against float64 at their edges -- csrc/augment.hip crop_resize_kernel and
resize_crop_bwd_kernel (r3m_crop_resize, r3m_resize_crop, r3m_resize_crop_backward), csrc/augment_dev.h bilinear_sample, and the crop
pre-passes of the 224 stem (r3m_stem_prep_crop: csrc/stem_dev.h StemCrop, csrc/stem_bf16.hip stem_prep16_crop_u8_kernel).

The cases, the float64 references and the derived tolerances are tests/resample_cases.py's (forward: 8 fp32 roundings,
8 * 2^-24 * 255 absolute; adjoint: (n_y + n_x + 4) * 2^-24 * S per source pixel, exact zeros where S == 0);
tests/test_resample_cases.py checks them on the CPU. Every output buffer is pre-filled with NaN and carries a 64-element sentinel
band on each side; float sources and gradients sit inside a larger NaN-filled allocation, so a read outside them shows up as NaN.
Every comparison is element by element and names the first failing index. Measured figures and the mutation check:
profiles/resample_edges.txt."""
import numpy as np
import pytest
import torch

import resample_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = R.GUARD
NAN = float("nan")
SRC = ["u8", "f32"]


def report(line):
    print(line, flush=True)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dtype=torch.float32, fill=NAN, prefill=None):
    """(whole buffer, view of `shape` GUARD elements inside it, the sentinel value)"""
    n = int(np.prod(shape))
    sentinel = -7.25 if dtype == torch.float32 else 0x5a5a
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(*shape)
    if prefill is None:
        view.fill_(fill)
    else:
        view.copy_(torch.tensor(np.asarray(prefill)))
    return buf, view, sentinel


def _guards_intact(buf, sentinel):
    ref = torch.full((GUARD,), sentinel, dtype=buf.dtype, device=DEV)
    return torch.equal(buf[:GUARD], ref) and torch.equal(buf[-GUARD:], ref)


def _in_nan(a):
    """float array -> device view inside a larger NaN-filled allocation"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + 2 * GUARD,), NAN, dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + a.size].view(*a.shape)
    view.copy_(torch.tensor(a))
    return buf, view


def _source(x_u8, x_f, src):
    """(keep-alive, device tensor, is_u8, host array)"""
    if src == "u8":
        t = torch.tensor(np.asarray(x_u8)).to(DEV)
        return t, t, 1, x_u8
    buf, view = _in_nan(x_f)
    return buf, view, 0, x_f


def _check(got, ref, tol, what):
    """element by element: |got - ref| <= tol (NaN fails); reports the largest error and the bound it met"""
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    tol_b = np.broadcast_to(np.asarray(tol, dtype=np.float64), err.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(tol_b > 0, err / np.where(tol_b > 0, tol_b, 1.0), np.where(err > 0, np.inf, 0.0))
    if np.isnan(ratio).any():
        worst = np.unravel_index(int(np.argmax(np.isnan(ratio))), err.shape)
    else:
        worst = np.unravel_index(int(np.argmax(ratio)), err.shape)
    report(f"{what}: largest error {np.nanmax(err) if err.size else 0.0:.3e}; closest to its bound at {tuple(int(v) for v in worst)}: "
           f"error {err[worst]:.3e} bound {tol_b[worst]:.3e}")
    bad = R.first_bad(err, tol_b)
    assert bad is None, f"{what}: first failing index {bad[0]}: error {bad[1]:.3e} > bound {bad[2]:.3e}"


def _identity_bits(x):
    """fl32(fl32(p / 255) * 255)"""
    return (np.asarray(x).astype(np.float32) / np.float32(255.0)) * np.float32(255.0)


def _first_diff(a, b):
    d = (a != b).nonzero()
    return None if d.numel() == 0 else d[0].tolist()


# ---- r3m_resize_crop / r3m_resize_crop_backward over the axis classes -------------------------------------------------------------
def _resize_forward(hip, case, src):
    N, C, ay, ax = R.resize_case(case)
    x_u8, x_f, _, _ = R.resize_inputs(case)
    keep, x, is_u8, host = _source(x_u8, x_f, src)
    buf, out, sent = _guarded((N, C, ay[3], ax[3]))
    rc = hip.r3m_resize_crop(x.data_ptr(), is_u8, out.data_ptr(), N, C, ay[0], ax[0], ay[1], ax[1], ay[2], ax[2], ay[3], ax[3], _st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(buf, sent), "resize_crop wrote outside its output"
    return out, host


@pytest.mark.parametrize("src", SRC)
@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_resize_crop_forward(hip, case, src):
    N, C, ay, ax = R.resize_case(case)
    out, host = _resize_forward(hip, case, src)
    ref = R.resize_refs(case)[0 if src == "u8" else 1]
    _check(out, ref, R.FWD_BOUND, f"resize_crop {case[0]} x {case[1]} {src}")
    if R.AXES[case[0]][0] == "identity" and R.AXES[case[1]][0] == "identity":
        want = _identity_bits(host[:, :, ay[2]:ay[2] + ay[3], ax[2]:ax[2] + ax[3]])
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), ("identity", np.argwhere(got != want)[:1].tolist())


def _resize_backward(hip, case, accumulate, dout, prefill):
    N, C, ay, ax = R.resize_case(case)
    buf, din, sent = _guarded((N, C, ay[0], ax[0]), prefill=prefill if accumulate else None)
    rc = hip.r3m_resize_crop_backward(dout.data_ptr(), din.data_ptr(), N, C, ay[0], ax[0], ay[1], ax[1], ay[2], ax[2], ay[3], ax[3],
                                      accumulate, _st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(buf, sent), "resize_crop_backward wrote outside din"
    return din


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_resize_crop_backward(hip, case, accumulate):
    N, C, ay, ax = R.resize_case(case)
    _, x_f, dout_h, prefill = R.resize_inputs(case)
    adj = R.resize_refs(case)[2]
    keep, dout = _in_nan(dout_h)
    din = _resize_backward(hip, case, accumulate, dout, prefill)
    bound = R.adjoint_bound(adj)
    what = f"resize_crop_backward {case[0]} x {case[1]} accumulate={accumulate}"
    got = din.cpu().numpy()
    untapped = adj.S == 0
    if accumulate:
        # fl32(prefill + sum): the sum's bound, carried through the last rounding, plus that rounding of a result <= |prefill| + S
        pre = prefill.astype(np.float64)
        _check(din, pre + adj.din, bound * (1 + R.U) + R.U * (np.abs(pre) + adj.S), what)
        same = got.view(np.int32)[untapped] == prefill.view(np.int32)[untapped]
        assert same.all(), (what, "an untapped pixel changed", np.argwhere(untapped)[~same][:1].tolist())
    else:
        _check(din, adj.din, bound, what)
        zero = got.view(np.int32)[untapped] == 0
        assert zero.all(), (what, "an untapped pixel is not an exact zero", np.argwhere(untapped)[~zero][:1].tolist())
    if case[0].startswith("down5") or case[1].startswith("down5"):
        assert untapped.sum() > untapped.size // 2
    # the same bits on a second run (a gather, no atomics)
    again = _resize_backward(hip, case, accumulate, dout, prefill)
    assert torch.equal(again.view(torch.int32), din.view(torch.int32)), (what, "second run differs at", _first_diff(again, din))
    if not accumulate:
        # <R x, g> = <x, R^T g> in float64 from the two GPU results; each side is off by at most the sum of its elementwise bounds
        y, _ = _resize_forward(hip, case, "f32")
        g64, x64 = dout_h.astype(np.float64), x_f.astype(np.float64)
        lhs = float((y.cpu().numpy().astype(np.float64) * g64).sum())
        rhs = float((x64 * got.astype(np.float64)).sum())
        tol = float(np.abs(g64).sum() * R.FWD_BOUND + (np.abs(x64) * bound).sum())
        report(f"{what}: <Rx, g> - <x, R^T g> = {abs(lhs - rhs):.3e} bound {tol:.3e}")
        assert abs(lhs - rhs) <= tol, (what, lhs, rhs, tol)


# ---- r3m_crop_resize: output sizes, channel counts, frames per box, boxes at every edge, launch edges --------------------------------
@pytest.mark.parametrize("src", SRC)
@pytest.mark.parametrize("name", [c.name for c in R.CROP_CASES])
def test_crop_resize(hip, name, src):
    c = {c.name: c for c in R.CROP_CASES}[name]
    x_u8, x_f = R.crop_inputs(name)
    keep, x, is_u8, host = _source(x_u8, x_f, src)
    boxes = torch.tensor(c.boxes, dtype=torch.int32, device=DEV)
    buf, out, sent = _guarded((c.N, c.C, c.Ho, c.Wo))
    rc = hip.r3m_crop_resize(x.data_ptr(), is_u8, boxes.data_ptr(), out.data_ptr(), c.N, c.C, c.Hi, c.Wi, c.Ho, c.Wo, c.fpb, _st())
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(buf, sent), "crop_resize wrote outside its output"
    _check(out, R.crop_refs(name)[0 if src == "u8" else 1], R.FWD_BOUND, f"crop_resize {name} {src}")
    got = out.cpu().numpy()
    for n in range(c.N):                      # a box of exactly the output size is the identity
        t, l, h, w = c.boxes[n // c.fpb]
        if (h, w) == (c.Ho, c.Wo):
            want = _identity_bits(host[n, :, t:t + h, l:l + w])
            assert np.array_equal(got[n].view(np.int32), want.view(np.int32)), (name, "identity box, frame", n)


# ---- r3m_stem_prep_crop: its ABI contract, anchored to the CPU ------------------------------------------------------------------------
@pytest.mark.parametrize("src", SRC)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in R.STEM_CROP_CASES])
def test_stem_prep_crop(hip, name, dtype, src):
    c = {c.name: c for c in R.STEM_CROP_CASES}[name]
    x_u8, x_f = R.stem_crop_inputs(name)
    keep, x, is_u8, host = _source(x_u8, x_f, src)
    boxes = torch.tensor(c.boxes, dtype=torch.int32, device=DEV)
    F = c.F
    # crop_resize at the same boxes against float64: anchors the chain to the CPU
    cbuf, crop, csent = _guarded((F, 3, 224, 224))
    assert hip.r3m_crop_resize(x.data_ptr(), is_u8, boxes.data_ptr(), crop.data_ptr(), F, 3, c.Hi, c.Wi, 224, 224, c.fpb, _st()) == 0, \
        hip.r3m_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(cbuf, csent)
    _check(crop, R.stem_crop_ref(name, src == "u8"), R.FWD_BOUND, f"crop_resize for stem_prep_crop {name} {src}")
    # the contract: bit-identical to r3m_crop_resize followed by r3m_stem_prep / r3m_stem_prep_bf16
    if dtype == "fp32":
        shape, tdt, fill, dti = (F, 224, 224, 3), torch.float32, NAN, 0
    else:
        assert hip.r3m_stem_xn16_bytes(F) == F * 232 * 704 * 2
        shape, tdt, fill, dti = (F, 232, 704), torch.int16, 0x7fc0, 1          # 0x7fc0: a bf16 NaN
    bbuf, chain, bsent = _guarded(shape, tdt, fill)
    fbuf, fused, fsent = _guarded(shape, tdt, fill)
    prep = hip.r3m_stem_prep if dtype == "fp32" else hip.r3m_stem_prep_bf16
    assert prep(crop.data_ptr(), chain.data_ptr(), F, _st()) == 0, hip.r3m_last_error()
    assert hip.r3m_stem_prep_crop(x.data_ptr(), is_u8, boxes.data_ptr(), c.fpb, c.Hi, c.Wi, fused.data_ptr(), F, dti, _st()) == 0, \
        hip.r3m_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(bbuf, bsent) and _guards_intact(fbuf, fsent), "a stem pre-pass wrote outside its image"
    a, b = (fused.view(torch.int32), chain.view(torch.int32)) if dtype == "fp32" else (fused, chain)
    assert torch.equal(a, b), (name, dtype, src, "first differing element", _first_diff(a, b), int((a != b).sum()))
    if dtype == "fp32":
        assert not torch.isnan(fused).any()
    else:
        pad = torch.ones(232, 704, dtype=torch.bool, device=DEV)
        pad[3:227, 9:681] = False
        assert int((fused[:, pad] != 0).sum()) == 0, (name, "padding is not exact zeros", _first_diff(fused * pad, torch.zeros_like(fused)))
        # the picture itself holds no NaN left over from the pre-fill (exponent all ones, mantissa non-zero)
        pic = fused[:, 3:227, 9:681].to(torch.int32) & 0x7fff
        assert int((pic > 0x7f80).sum()) == 0
