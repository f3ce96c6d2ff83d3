"""-m gpu: the reset of the few-row kernel's workspace (SmallLaunchSet::reset, csrc/conv_small.hip) covers every ticket block, for each
of the five callers: the call runs once on a workspace of zero bytes and once on the same workspace refilled with 0xFF over its
whole length; the outputs must be bit-equal and free of NaN. A ticket block that the one memset misses, or that a launch looks for
at another offset than the memset cleared, starts at 0xFFFFFFFF: no block of the tile draws ticket S - 1, nobody stores, and the
pre-filled NaN of the output stays (the kernel is wait-free: a garbage ticket means no store, never a spin or a fault).

So that this can fail at all, every call holds a launch with S > 1, and the multi-launch calls hold at least two launches the
routing rule takes; both are asserted from r3m_debug_conv_small_plan / r3m_debug_linear_small_plan, so that a change of the rule
cannot make the test vacuous. Ticket blocks of different sizes (a block is 4 bytes per tile padded to 256: more than 64 tiles)
make a wrong offset visible as well; where the shapes give them is asserted per case:
  * the encoder at one 64 x 64 frame has 256-byte blocks only, at two 224 x 224 frames layer1's launches have 98 tiles;
  * the text model at B * T <= 16 has 256-byte blocks only, at 3 x 128 tokens the QKV Linear has 72 tiles;
  * the reward head's four Linears have the same rows and the same width: their blocks are equal at every size."""
import ctypes as C

import numpy as np
import pytest
import torch

import linear_small_cases as lc
import small_conv_cases as sc
from util import DEV, _st, nhwc, rnd

pytestmark = pytest.mark.gpu


def _ticket_bytes(p):
    return -(-p["tiles_m"] * p["tiles_n"] * 4 // 256) * 256


def _taken(plans, differ):
    """the plans the routing rule takes; asserts what makes the case able to fail"""
    taken = [p for p in plans if p["take"]]
    assert len(taken) >= 2 and any(p["S"] > 1 for p in taken), taken
    assert (len({_ticket_bytes(p) for p in taken}) > 1) == differ, [_ticket_bytes(p) for p in taken]
    return taken


def _zero_then_ff(ws, run):
    """run() on the workspace zeroed, then refilled with 0xFF: equal bits, no NaN"""
    assert ws.dtype == torch.uint8
    ws.zero_()
    first = [t.clone() for t in run()]
    ws.fill_(0xFF)
    second = run()
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert not torch.isnan(a).any() and not torch.isnan(b).any()
        assert torch.equal(a, b)


def test_conv2d_fwd_affine_small(hip):
    case, flags = (1, 5, 5, 128, 64, 3, 1, 1), sc.AR
    assert sc.conv_small_plan(hip, case, flags)["S"] > 1
    N, Hi, Wi, Ci, Co, k, s, p = case
    xd = nhwc(rnd((N, Ci, Hi, Wi), 1)).to(DEV)
    wd = rnd((Co, Ci, k, k), 2, -0.2, 0.2).permute(0, 2, 3, 1).contiguous().to(DEV)
    scale, shift = rnd((Co,), 21, 0.5, 1.5).to(DEV), rnd((Co,), 22, -0.6, 0.6).to(DEV)
    need = hip.r3m_conv2d_small_workspace_bytes(*case, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def run():
        out = torch.full((N, Hi, Wi, Co), float("nan"), device=DEV)
        rc = hip.r3m_conv2d_fwd_affine_small(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), scale.data_ptr(), shift.data_ptr(), *case, flags, 0,
                                             ws.data_ptr(), need, _st())
        assert rc == 0, hip.r3m_last_error()
        return [out]

    _zero_then_ff(ws, run)


def test_linear_fwd_small(hip):
    case, flags = (17, 256, 128), lc.BR
    p = lc.linear_small_plan(hip, case, flags)
    assert p["S"] > 1 and p["tiles_n"] == 2, p
    M, K, N = case
    xd, wd, bd = rnd((M, K), 1).to(DEV), rnd((N, K), 2, -0.2, 0.2).to(DEV), rnd((N,), 22, -0.6, 0.6).to(DEV)
    need = hip.r3m_linear_small_workspace_bytes(M, K, N, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def run():
        out = torch.full((M, N), float("nan"), device=DEV)
        rc = hip.r3m_linear_fwd_small(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), M, K, N, flags, 0, ws.data_ptr(), need, _st())
        assert rc == 0, hip.r3m_last_error()
        return [out]

    _zero_then_ff(ws, run)


@pytest.mark.parametrize("F,hw,differ", [(1, (64, 64), False), (2, (224, 224), True)])
def test_prepared_encoder(hip, F, hw, differ):
    from oracle import detgen
    from test_gpu_inference_session import _encoder
    convs, need = sc.resnet_convs(hip, 18, F, hw)
    assert need > 0
    _taken([sc.conv_small_plan(hip, g) for g in convs[1:]], differ)
    sess = _encoder(18).inference_session()
    x = torch.from_numpy(detgen.smooth_frames(f"smallws{F}", (F, 3) + hw, 7)).to(DEV)

    def run():
        if sess._arena is not None:                         # the activations live in the arena: a launch that stores nothing must not
            sess._arena.fill_(0xFF)                         # find the previous call's values there
            sess.refresh()
        with torch.no_grad():
            h, maps = sess.forward_features(x)
        return [h] + [maps[k] for k in sorted(maps)]

    run()                                                   # allocates the session's arena and workspace
    assert sess._workspace.numel() == need
    _zero_then_ff(sess._workspace, run)


def test_reward_head(hip):
    from test_gpu_reward_infer import _setup
    size, R = (512, 1024, 768), 5
    D, H, LD = size
    taken = _taken([lc.linear_small_plan(hip, case, fl) for case, fl in lc.head_linears(R, D, H, LD)], False)
    assert len(taken) == 4
    flat, e0, eg, le, _ = _setup(size)
    flat_d, e0d, egd, led = flat.to(DEV), e0[:R].contiguous().to(DEV), eg[:R].contiguous().to(DEV), le[:R].contiguous().to(DEV)
    need = hip.r3m_langrew_infer_workspace_bytes(R, D, H, LD)
    assert need > 0, hip.r3m_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def run():
        score = torch.full((R,), float("nan"), device=DEV)
        rc = hip.r3m_langrew_infer(e0d.data_ptr(), egd.data_ptr(), led.data_ptr(), flat_d.data_ptr(), score.data_ptr(), ws.data_ptr(), need,
                                   R, R, D, H, LD, _st())
        assert rc == 0, hip.r3m_last_error()
        return [score]

    _zero_then_ff(ws, run)


@pytest.mark.parametrize("B,T,differ", [(2, 8, False), (3, 128, True)])
def test_text_model(hip, B, T, differ):
    import text_ref
    from oracle import detgen
    from r3m_amd.text import HipDistilBert
    from test_gpu_text import MODELS
    d = MODELS["b"]
    assert d["n_layers"] == 2
    _taken([lc.linear_small_plan(hip, case, fl) for case, fl in lc.text_linears(B * T, d["dim"], d["ffn"])], differ)
    model = HipDistilBert.from_state_dict(text_ref.detgen_state_dict("deeptext_b", **d), d["n_heads"], DEV)
    ids = torch.from_numpy((detgen.unit(f"smallws_ids_{B}_{T}", B * T) * d["vocab"]).astype(np.int64).reshape(B, T))
    mask = torch.from_numpy(text_ref.ragged_mask(B, T, 3))

    def run():
        return list(model.hidden_and_pools(ids, mask, few_rows=True))

    run()                                                   # allocates the model's workspace for (B, T)
    ws, nbytes = model._ws[(B, T, True)]
    assert nbytes == ws.numel() == hip.r3m_text_small_workspace_bytes((C.c_int * 6)(*model.dims), B, T)
    _zero_then_ff(ws, run)
