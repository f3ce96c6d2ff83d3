"""not gpu: oracle/r3m_ref.r3m_loss_ref with num_negatives 1 and 5 against the goldens the REFERENCE's own Trainer.update made with that
attribute (tests/golden/make_golden_negatives.py -> loss_neg{1,5}_{l2,cos}.npz), at the gates tests/test_oracle.py applies to G3. This
pins the oracle for N != 3, which the GPU tests of tests/test_gpu_negatives.py rely on."""
import os
import sys

import numpy as np
import pytest
import torch

from util import rel_err


@pytest.mark.parametrize("l2dist", [True, False], ids=["l2dist", "cosine"])
@pytest.mark.parametrize("N", [1, 5])
def test_oracle_loss_matches_reference_golden_with_num_negatives(golden_dir, N, l2dist):
    from oracle import detgen, r3m_ref
    sys.path.insert(0, golden_dir)
    from make_golden import make_alle
    g = np.load(os.path.join(golden_dir, f"loss_neg{N}_{'l2' if l2dist else 'cos'}.npz"))
    assert int(g["num_negatives"]) == N and g["perms"].shape == (5 * N, 8) and g["scores"].shape == (6 + 3 * N, 8)
    B, D = 8, 512
    m = r3m_ref.R3MRef(size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=1.0, l2dist=l2dist)
    m.num_negatives = N
    sd = {}
    for k, v in m.lang_rew.state_dict().items():
        fan_in = v.shape[1] if v.dim() == 2 else m.lang_rew.state_dict()[k.replace("bias", "weight")].shape[1]
        a = 1.0 / np.sqrt(fan_in)
        sd[k] = torch.from_numpy(detgen.uniform("lr" + k, tuple(v.shape), -a, a))
    m.lang_rew.load_state_dict(sd)
    alle = torch.from_numpy(make_alle(B, D, "alle")).requires_grad_(True)
    feats = torch.from_numpy(detgen.uniform("langfeat", (B, 768), -0.6, 0.6))
    mask = torch.ones(B)
    mask[5] = 0.0
    perms = torch.from_numpy(g["perms"])
    full, met, scores = r3m_ref.r3m_loss_ref(m, alle, tcn_perm=perms[3 * N:5 * N], lang_feats=feats, lang_mask=mask,
                                             lang_perm=perms[0:3 * N])
    full.backward()
    ref = dict(zip([str(n) for n in g["metric_names"]], g["metric_values"]))
    assert set(met.keys()) == set(ref.keys())
    for k, v in ref.items():
        assert abs(met[k] - v) <= 1e-5 * max(1.0, abs(v)), (k, met[k], v)
    assert rel_err(scores.detach().numpy(), g["scores"])[0] < 1e-5
    assert rel_err(alle.grad.numpy(), g["dalle"])[0] < 1e-4
    assert rel_err(m.lang_rew.pred[8].weight.grad.numpy(), g["grad_pred.8.weight"])[0] < 1e-4
    for k, p in m.lang_rew.named_parameters():
        ref_n = float(g["gradnorm_" + k])
        assert abs(float(p.grad.double().norm()) - ref_n) <= 1e-4 * max(ref_n, 1e-12), k


def test_goldens_keep_compared_pairs_apart(golden_dir):
    """the stored scores: every positive is more than 1e-4 from the largest of its 1 + N negatives (the maker's seed rule)"""
    for N in (1, 5):
        for tag in ("l2", "cos"):
            s = np.load(os.path.join(golden_dir, f"loss_neg{N}_{tag}.npz"))["scores"].astype(np.float64)
            for j in range(3):
                mx = np.max(np.stack([s[3 + j]] + [s[6 + 3 * k + j] for k in range(N)]), 0)
                assert np.abs(s[j] - mx).min() > 1e-4, (N, tag, j)
