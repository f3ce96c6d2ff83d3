#!/usr/bin/env python
"""Bit record of the objective and the batched reward head at num_negatives = 3 (GPU only): one SHA-256 per output for fixed inputs,
through ops.r3m_loss and LanguageReward.batched_scores -- dalle, metrics, scores, dscore, the head's parameter gradients and the head's
dalle; l2dist and cosine; fp32 and bf16 head; B = 8, 256 and 257 clips. Three listings must be equal, line for line:
  tools/build_ab.sh HEAD                                                              # the parent commit's library
  R3M_HIP_LIB=r3m_amd/lib/libr3m_hip_base.so python tools/negatives_bits.py old > a   # the parent's library, the entry points it has
  python tools/negatives_bits.py old > b                                              # this tree, the same (old) entry points
  python tools/negatives_bits.py n > c                                                # this tree, the `_n` entry points with N = 3
`old` routes the Python layers' `_n` calls to r3m_loss_tcn_lp / r3m_loss_lang_infonce / r3m_langrew_*_dt (use_old_entries below), which
is all a library from before the `_n` entry points has."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def use_old_entries(L):
    """make the `_n` names of the loaded library handle call the entry points without N (N must be 3)"""
    def three(N):
        assert N == 3, "the entry points without N compute num_negatives = 3"
    def ws_loss(B, N):
        three(N)
        return L.r3m_loss_workspace_bytes(B)
    def tcn(*a):                                         # (..., B, D, N, l2dist, ...)
        three(a[8])
        return L.r3m_loss_tcn_lp(*a[:8], *a[9:])
    def infonce(*a):                                     # (..., B, N, langweight, stream)
        three(a[6])
        return L.r3m_loss_lang_infonce(*a[:6], *a[7:])
    def ws_head(B, D, H, LD, N):
        three(N)
        return L.r3m_langrew_workspace_bytes(B, D, H, LD)
    def fwd(*a):                                         # (..., B, D, hidden, lang_dim, N, dtype, stream)
        three(a[11])
        return L.r3m_langrew_forward_dt(*a[:11], *a[12:])
    def bwd(*a):                                         # (..., B, D, hidden, lang_dim, N, accumulate, dtype, stream)
        three(a[11])
        return L.r3m_langrew_backward_dt(*a[:11], *a[12:])
    L.r3m_loss_workspace_bytes_n, L.r3m_loss_tcn_lp_n, L.r3m_loss_lang_infonce_n = ws_loss, tcn, infonce
    L.r3m_langrew_workspace_bytes_n, L.r3m_langrew_forward_n, L.r3m_langrew_backward_n = ws_head, fwd, bwd


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def main():
    from r3m_amd import _lib, ops
    from r3m_amd.models_language import LanguageReward
    from util import DEV, rnd
    mode = sys.argv[1] if len(sys.argv) > 1 else "n"
    assert mode in ("old", "n"), __doc__
    L = _lib.lib()
    if mode == "old":
        use_old_entries(L)
    for B, D, H in ((8, 512, 64), (256, 2048, 1024), (257, 512, 64)):
        g = torch.Generator().manual_seed(900 + B)
        perms = torch.stack([torch.randperm(B, generator=g) for _ in range(15)]).to(torch.int32).to(DEV)
        alle0 = torch.relu(rnd((B, 5, D), 901, -0.5, 1.0)).to(DEV)
        feats = rnd((B, 768), 902, -0.6, 0.6).to(DEV)
        mask = (rnd((B,), 903) > -0.4).float().to(DEV)
        for prec in ("fp32", "bf16"):
            rew = LanguageReward(None, D, H, 768, precision=prec)
            torch.manual_seed(904)
            rew.reset_parameters()
            rew = rew.to(DEV)
            for l2dist in (True, False):
                what = f"B={B} D={D} hidden={H} head={prec} {'l2dist' if l2dist else 'cosine'}"
                alle = alle0.clone().requires_grad_(True)
                scores = rew.batched_scores(alle, feats, perms[:9])
                print(f"{what} scores {sha(scores)}")
                leaf_a, leaf_s = alle0.clone().requires_grad_(True), scores.detach().clone().requires_grad_(True)
                full, met = ops.r3m_loss(leaf_a, perms[9:15], 1e-5, 1e-5, 1.0, l2dist=l2dist, scores=leaf_s, mask=mask, langweight=1.0)
                full.backward()
                print(f"{what} metrics {sha(met)}")
                print(f"{what} dalle {sha(leaf_a.grad)}")
                print(f"{what} dscore {sha(leaf_s.grad)}")
                rew.mark_grads_stale()
                scores.backward(leaf_s.grad)
                print(f"{what} head grads {sha(rew.flat_grads())}")
                print(f"{what} head dalle {sha(alle.grad)}")
                # the time-contrastive loss alone (langweight 0): another finalize path
                leaf_a = alle0.clone().requires_grad_(True)
                full, met = ops.r3m_loss(leaf_a, perms[9:15], 1e-5, 1e-5, 1.0, l2dist=l2dist)
                full.backward()
                print(f"{what} tcn-only metrics {sha(met)} dalle {sha(leaf_a.grad)}")


if __name__ == "__main__":
    main()
