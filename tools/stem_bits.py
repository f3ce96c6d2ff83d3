#!/usr/bin/env python
"""Bit record of the stem kernels (GPU only): one SHA-256 per case and operation over everything the library named by R3M_HIP_LIB
writes through the C ABI, into NaN-prefilled outputs. Two builds compute the same bits iff their listings are equal:
  R3M_HIP_LIB=r3m_amd/lib/libr3m_hip_base.so python tools/stem_bits.py > base.txt;  python tools/stem_bits.py > new.txt;  diff base.txt new.txt
224 x 224 sets (fp32 MFMA, bf16 MFMA) at F = 1, 3, 11 (11: every persistent loop takes a second trip), the _dt entry points with
bf16 output, the input gradient, the general stem at six (F, H, W), and the crop pre-passes from uint8 and float clips."""
import hashlib
import os
import sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from r3m_amd import _lib
from util import DEV, rnd

L = _lib.lib()
st = torch.cuda.current_stream().cuda_stream
F32, BF16 = torch.float32, torch.bfloat16


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        torch.cuda.synchronize()
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:32]


def ok(rc):
    assert rc == 0, L.r3m_last_error()


def nan(shape, dt=F32):
    return torch.full(shape, float("nan"), dtype=dt, device=DEV)


def frames(F, H, W):
    return torch.floor(rnd((F, 3, H, W), 5, 0.0, 256.0)).clamp(0, 255).to(DEV)


W147 = rnd((64, 7, 7, 3), 6, -0.1, 0.1).to(DEV)


def accumulate_both(tag, call, shape):
    """accumulate = 0 into a NaN-prefilled tensor, then accumulate = 1 on top of that result"""
    out = nan(shape)
    for acc in (0, 1):
        ok(call(out, acc))
        print(f"{tag} accumulate={acc} {sha(out)}")


# ---- 224 x 224: fp32 MFMA (fp32 and bf16 output / dY) and bf16 MFMA ----
for Fr in (1, 3, 11):
    x = frames(Fr, 224, 224)
    dy = rnd((Fr, 112, 112, 64), 7).to(DEV)
    xn = nan((Fr, 224, 224, 3))
    ok(L.r3m_stem_prep(x.data_ptr(), xn.data_ptr(), Fr, st))
    print(f"224 fp32 F={Fr} prep {sha(xn)}")
    for tdt, dti in ((F32, 0), (BF16, 1)) if Fr == 3 else ((F32, 0),):
        name = "fp32" if dti == 0 else "fp32-mfma/bf16-out"
        for want_stats in (1, 0):
            y, stats = nan((Fr, 112, 112, 64), tdt), nan((Fr * 49, 2, 64))
            ok(L.r3m_stem_conv_fwd_dt(xn.data_ptr(), W147.data_ptr(), y.data_ptr(), stats.data_ptr() if want_stats else None, Fr, dti, st))
            print(f"224 {name} F={Fr} fwd stats={want_stats} {sha(y, stats)}")
        wsb = L.r3m_stem_conv_wgrad_workspace_bytes()
        ws, dyt = torch.empty(wsb, dtype=torch.uint8, device=DEV), dy.to(tdt)
        accumulate_both(f"224 {name} F={Fr} wgrad", lambda dw, acc: L.r3m_stem_conv_wgrad_dt(
            xn.data_ptr(), dyt.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb, Fr, acc, dti, st), (64, 7, 7, 3))
    xn16 = nan((L.r3m_stem_xn16_bytes(Fr) // 2,), BF16)
    ok(L.r3m_stem_prep_bf16(x.data_ptr(), xn16.data_ptr(), Fr, st))
    print(f"224 bf16 F={Fr} prep {sha(xn16)}")
    for want_stats in (1, 0):
        y, stats = nan((Fr, 112, 112, 64), BF16), nan((Fr * 49, 2, 64))
        ok(L.r3m_stem_conv_fwd_bf16(xn16.data_ptr(), W147.data_ptr(), y.data_ptr(), stats.data_ptr() if want_stats else None, Fr, st))
        print(f"224 bf16 F={Fr} fwd stats={want_stats} {sha(y, stats)}")
    wsb = L.r3m_stem_conv_wgrad_bf16_workspace_bytes()
    ws, dy16 = torch.empty(wsb, dtype=torch.uint8, device=DEV), dy.to(BF16)
    accumulate_both(f"224 bf16 F={Fr} wgrad", lambda dw, acc: L.r3m_stem_conv_wgrad_bf16(
        xn16.data_ptr(), dy16.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb, Fr, acc, st), (64, 7, 7, 3))

# ---- 224 x 224 input gradient ----
for Fr in (1, 3):
    for tdt, dti in ((F32, 0), (BF16, 1)):
        dz = rnd((Fr, 112, 112, 64), 8).to(DEV).to(tdt)
        accumulate_both(f"224 dz={'fp32' if dti == 0 else 'bf16'} F={Fr} input_grad", lambda dx, acc: L.r3m_stem_input_grad(
            dz.data_ptr(), dti, W147.data_ptr(), dx.data_ptr(), Fr, acc, st), (Fr, 3, 224, 224))

# ---- the general stem: (12, 97, 131) gives 588 weight-gradient rows and (3, 512, 509) 765 forward tiles against 512 blocks ----
for (Fr, H, W) in ((1, 32, 32), (3, 33, 47), (3, 97, 131), (12, 97, 131), (3, 512, 509), (3, 224, 224)):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = frames(Fr, H, W)
    for tdt, dti in ((F32, 0), (BF16, 1)):
        tag = f"gen {'fp32' if dti == 0 else 'bf16'} F={Fr} {H}x{W}"
        xn = nan((Fr, H, W, 3), tdt)
        assert xn.numel() * xn.element_size() == L.r3m_stem_gen_image_bytes(Fr, H, W, dti)
        ok(L.r3m_stem_gen_prep(x.data_ptr(), xn.data_ptr(), Fr, H, W, dti, st))
        print(f"{tag} prep {sha(xn)}")
        for want_stats in (1, 0):
            y, stats = nan((Fr, Ho, Wo, 64), tdt), nan(((Fr * Ho * Wo + 255) // 256, 2, 64))
            ok(L.r3m_stem_gen_fwd(xn.data_ptr(), W147.data_ptr(), y.data_ptr(), stats.data_ptr() if want_stats else None, Fr, H, W, dti, st))
            print(f"{tag} fwd stats={want_stats} {sha(y, stats)}")
        dy = rnd((Fr, Ho, Wo, 64), 7).to(DEV).to(tdt)
        ws = torch.empty(L.r3m_stem_gen_wgrad_ws_bytes(), dtype=torch.uint8, device=DEV)
        accumulate_both(f"{tag} wgrad", lambda dw, acc: L.r3m_stem_gen_wgrad(
            xn.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), Fr, H, W, acc, dti, st), (64, 7, 7, 3))
        accumulate_both(f"{tag} input_grad", lambda dx, acc: L.r3m_stem_gen_input_grad(
            dy.data_ptr(), W147.data_ptr(), dx.data_ptr(), Fr, H, W, acc, dti, st), (Fr, 3, H, W))

# ---- crop pre-passes: the clips and boxes of tests/test_gpu_augment.py's bit-identity test, and one clip narrower than 4 pixels
# (uint8 clips that narrow take the generic bf16 kernel) ----
NF = 7
for (H, W) in ((256, 256), (256, 320), (300, 512), (240, 700), (9, 4), (33, 7), (8, 3)):
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (NF, 3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    boxes = torch.tensor([[0, 0, H, W], [H - min(H, 5), W - min(W, 4), min(H, 5), min(W, 4)], [0, W - min(W, 9), min(H, 6), min(W, 9)],
                          [H // 3, 0, max(1, H // 2), max(1, W // 2)], [1, 1, 1, 1],
                          [H // 5, W // 7, max(2, H // 2), max(2, int(W * 0.6))], [0, max(0, W - 224), min(H, 224), min(W, 224)]],
                         dtype=torch.int32).to(DEV)
    for src, is_u8 in ((raw, 1), (raw.float(), 0)):
        for dti in (0, 1):
            out = nan((NF, 224, 224, 3)) if dti == 0 else nan((L.r3m_stem_xn16_bytes(NF) // 2,), BF16)
            ok(L.r3m_stem_prep_crop(src.data_ptr(), is_u8, boxes.data_ptr(), 1, H, W, out.data_ptr(), NF, dti, st))
            print(f"crop {H}x{W} src={'u8' if is_u8 else 'f32'} image={'fp32' if dti == 0 else 'bf16'} {sha(out)}")
