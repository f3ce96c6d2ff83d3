"""Thin autograd / tensor wrappers over the C ABI (include/r3m_hip.h). PyTorch here is plumbing: allocation, streams,
autograd bookkeeping. Every function requires CUDA (HIP) tensors and raises otherwise — no eager fallback.
"""
import operator

import torch

from . import _lib

MAX_NEGATIVES = 16       # R3M_MAX_NEGATIVES of include/r3m_hip.h: the cap of csrc/loss.hip and csrc/lang.hip (the reference has none)

METRIC_SLOTS = {"l2loss": 0, "l1loss": 1, "l0loss": 2, "tcnloss": 3, "aligned": 4, "rewloss": 5, "rewacc1": 6, "rewacc2": 7,
                "rewacc3": 8, "full_loss": 9}


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("r3m_amd.ops: HIP kernels need CUDA/HIP tensors (no CPU fallback)")


def check_num_negatives(n, tcnweight=0.0, who="r3m_amd"):
    """The number of cross-clip negatives (the reference's model.num_negatives) as an int in 0..MAX_NEGATIVES; ValueError otherwise,
    and for 0 with the time-contrastive loss on, where the reference fails (torch.stack of an empty list, r3m/trainer.py:140)."""
    shown = n
    try:                       # any integer-like (numpy integers, 0-d integer tensors), as range() takes them; no bool, no float
        n = None if isinstance(n, bool) else operator.index(n)
    except TypeError:
        n = None
    if n is None or not 0 <= n <= MAX_NEGATIVES:
        raise ValueError(f"{who}: num_negatives={shown!r} must be an int in 0..{MAX_NEGATIVES} (the HIP objective's cap)")
    if n == 0 and tcnweight > 0:
        raise ValueError(f"{who}: num_negatives=0 with tcnweight > 0: the reference fails there (torch.stack of an empty list, "
                         "r3m/trainer.py:140)")
    return n


def inverse_permutations(perm):
    """perm [P,B] int -> inverse [P,B] (iperm[p, perm[p, i]] = i)."""
    P, B = perm.shape
    inv = torch.empty_like(perm)
    ar = torch.arange(B, dtype=perm.dtype, device=perm.device).expand(P, B)
    inv.scatter_(1, perm.long(), ar)
    return inv


class _R3MLossFn(torch.autograd.Function):
    """full_loss(alle [, scores]) with the reference's metrics as a side output; gradient computed in the same launches."""

    @staticmethod
    def forward(ctx, alle, perm, scores, mask, l2w, l1w, tcnw, langw, l2dist, N):
        B, five, D = alle.shape
        assert five == 5
        N = check_num_negatives(N, tcnw, "r3m_loss")
        if perm is not None and (perm.dim() != 2 or tuple(perm.shape) != (2 * N, B)):
            raise ValueError(f"r3m_loss: perm {tuple(perm.shape)} must be [2 * num_negatives, B] = [{2 * N}, {B}]")
        if scores is not None and (scores.dim() != 2 or tuple(scores.shape) != (6 + 3 * N, B)):
            raise ValueError(f"r3m_loss: scores {tuple(scores.shape)} must be [6 + 3 * num_negatives, B] = [{6 + 3 * N}, {B}]")
        _need_cuda(alle, perm, scores, mask)
        L = _lib.lib()
        alle = alle.contiguous()
        dev = alle.device
        ws_bytes = L.r3m_loss_workspace_bytes_n(B, N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        metrics = torch.zeros(16, dtype=torch.float32, device=dev)
        dalle = torch.empty_like(alle)
        if perm is None:
            perm = torch.arange(B, dtype=torch.int32, device=dev).repeat(2 * N, 1)
        perm = perm.to(device=dev, dtype=torch.int32).contiguous()
        iperm = inverse_permutations(perm).contiguous()
        st = _lib.stream_ptr(dev)
        dscore = None
        have_lang = scores is not None and langw > 0
        with _lib.on(alle):
            _lib.check(L.r3m_loss_tcn_lp_n(alle.data_ptr(), perm.data_ptr(), iperm.data_ptr(), dalle.data_ptr(), ws.data_ptr(), ws_bytes,
                                           B, D, N, 1 if l2dist else 0, float(l2w), float(l1w), float(tcnw), st), "loss_tcn_lp")
            if have_lang:
                scores = scores.contiguous()
                mask = mask.to(device=dev, dtype=torch.float32).contiguous()
                dscore = torch.empty_like(scores)
                _lib.check(L.r3m_loss_lang_infonce_n(scores.data_ptr(), mask.data_ptr(), dscore.data_ptr(), ws.data_ptr(), ws_bytes, B,
                                                     N, float(langw), st), "loss_lang_infonce")
            _lib.check(L.r3m_loss_finalize(ws.data_ptr(), ws_bytes, B, 1 if have_lang else 0, metrics.data_ptr(), float(l2w),
                                           float(l1w), float(tcnw), float(langw) if have_lang else 0.0, st), "loss_finalize")
        ctx.save_for_backward(dalle, dscore)
        ctx.mark_non_differentiable(metrics)
        return metrics[9].clone(), metrics

    @staticmethod
    def backward(ctx, gfull, _gmetrics):
        dalle, dscore = ctx.saved_tensors
        ga = dalle * gfull
        gs = None if dscore is None else dscore * gfull
        return ga, None, gs, None, None, None, None, None, None, None


def r3m_loss(alle, perm, l2weight, l1weight, tcnweight, l2dist=True, scores=None, mask=None, langweight=0.0, num_negatives=3):
    """alle [B,5,D]; perm [2N,B] TCN permutations in the reference's draw order (es0, es2 per negative; None: identities);
    scores [6+3N,B] + mask [B] for the language head (optional); N = num_negatives, 0..MAX_NEGATIVES (0 only with tcnweight == 0).
    A row count that does not fit N raises ValueError before any launch.
    Returns (full_loss 0-d tensor with grad, metrics[16] tensor — slots in METRIC_SLOTS)."""
    return _R3MLossFn.apply(alle, perm, scores, mask, l2weight, l1weight, tcnweight, langweight, l2dist, num_negatives)
