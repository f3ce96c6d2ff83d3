"""Generates tests/golden/loss_neg{1,5}_{l2,cos}.npz: G3 (make_golden.py::loss_golden) with model.module.num_negatives set to 1 and to 5
on the fake core, by running the REFERENCE's own Trainer.update (imported by path, oracle/by_path.py) on CPU fp32.
Run in the authoring container only (needs the reference tree):   python tests/golden/make_golden_negatives.py

Same set-up as G3: B = 8 clips, D = 512, embeddings make_alle(B, D, "alle"), sentence features and head weights from oracle/detgen.py,
clip 5 masked. Same content: perms [5N, B] (the 3N language draws, then the 2N TCN draws, in the order Trainer.update makes them),
metrics, d full_loss / d alle, the 6 + 3N scores in call order, the norm of every head gradient and two head gradients in full.

The seed of the permutations is the first one from SEED0 on at which every pair of numbers that a counting metric compares is more than
1e-4 apart in float64 (the rule of tests/test_gpu_objective.py): each positive score against the largest of its 1 + N negatives
(rewacc1-3), and s02 / s12, s01 / s02 of every clip (aligned). One pair is exempt because it is equal by construction, bit for bit in
any precision: make_alle gives clip 3 es2 == es1, so its s01 and s02 are the same arithmetic on the same numbers."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OUT, _FakeCore, _FakeModel, make_alle  # noqa: E402  (puts the repository root on sys.path)
from oracle import by_path, detgen  # noqa: E402

SEED0 = 4321
GAP = 1e-4
TIED_CLIP = 3


def call_scores(lang_rew, alle, feats, lang_perm, N):
    """the 6 + 3N evaluations in call order (trainer.py:72-92), in the dtype of the arguments"""
    e0, eg, es0, es1, es2 = [alle[:, i] for i in range(5)]
    G = lambda a, b: lang_rew(a, b, feats)[0]
    sc = [G(e0, eg), G(e0, es1), G(e0, es2), G(e0, e0), G(e0, es0), G(e0, es1)]
    for k in range(N):
        for j, other in enumerate((eg, es1, es2)):
            p = lang_perm[3 * k + j]
            sc.append(G(e0[p], other[p]))
    return torch.stack(sc)


def gaps_ok(core, alle, feats, perms, N):
    with torch.no_grad():
        a = alle.double()
        s = call_scores(copy.deepcopy(core.lang_rew).double(), a, feats.double(), perms[:3 * N], N)
        for j in range(3):
            mx = torch.stack([s[3 + j]] + [s[6 + 3 * k + j] for k in range(N)]).max(0)[0]
            if float((s[j] - mx).abs().min()) <= GAP:
                return False
        s02, s12, s01 = core.sim(a[:, 4], a[:, 2]), core.sim(a[:, 4], a[:, 3]), core.sim(a[:, 3], a[:, 2])
        free = torch.arange(a.shape[0]) != TIED_CLIP
        assert torch.equal(alle[TIED_CLIP, 4], alle[TIED_CLIP, 3])
        return float((s02 - s12).abs().min()) > GAP and float((s01 - s02)[free].abs().min()) > GAP


def loss_golden_negatives(N, l2dist, B=8, D=512):
    r3m, lang, trainer = by_path.load_reference()
    feats = torch.from_numpy(detgen.uniform("langfeat", (B, 768), -0.6, 0.6))
    core = _FakeCore(r3m, lang, D, l2dist, 1.0, feats)
    core.num_negatives = N
    shapes = [(k, tuple(v.shape)) for k, v in core.lang_rew.state_dict().items()]
    sd = {}
    for k, shp in shapes:
        fan_in = shp[1] if len(shp) == 2 else shapes[[s[0] for s in shapes].index(k.replace("bias", "weight"))][1][1]
        a = 1.0 / np.sqrt(fan_in)
        sd[k] = torch.from_numpy(detgen.uniform("lr" + k, shp, -a, a))
    core.lang_rew.load_state_dict(sd)
    alles = torch.from_numpy(make_alle(B, D, "alle").reshape(B * 5, D)).requires_grad_(True)
    alle = alles.detach().reshape(B, 5, D)
    model = _FakeModel(core, alles)
    b_lang = ["open the drawer"] * B
    b_lang[5] = ""                           # masked clip (trainer.py:107-109)
    for seed in range(SEED0, SEED0 + 1000):
        torch.manual_seed(seed)
        perms = torch.stack([torch.randperm(B) for _ in range(5 * N)])   # the draws Trainer.update is about to make
        if gaps_ok(core, alle, feats, perms, N):
            break
    else:
        raise AssertionError("no seed keeps the compared pairs apart")
    torch.manual_seed(seed)
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self                # trainer.py:108 hard-codes .cuda()
    try:
        metrics, _ = trainer.Trainer(1).update(model, (torch.zeros(B, 5, 3, 224, 224), b_lang), 0)
    finally:
        torch.Tensor.cuda = orig_cuda
    out = {"perms": perms.numpy(), "seed": np.array(seed), "num_negatives": np.array(N),
           "dalle": alles.grad.numpy().reshape(B, 5, D).copy(),
           "metric_names": np.array(list(metrics.keys())), "metric_values": np.array(list(metrics.values()), dtype=np.float64)}
    for k, p in core.lang_rew.named_parameters():
        out["gradnorm_" + k] = np.array(float(p.grad.double().norm()))
    out["grad_pred.8.weight"] = core.lang_rew.pred[8].weight.grad.numpy().copy()
    out["grad_pred.0.bias"] = core.lang_rew.pred[0].bias.grad.numpy().copy()
    with torch.no_grad():
        out["scores"] = call_scores(core.lang_rew, alle, feats, perms[:3 * N], N).numpy()
    path = os.path.join(OUT, f"loss_neg{N}_{'l2' if l2dist else 'cos'}.npz")
    np.savez_compressed(path, **out)
    print("loss", N, "l2" if l2dist else "cos", "seed", seed, os.path.getsize(path), "bytes",
          dict(zip(metrics.keys(), [round(v, 6) for v in metrics.values()])))


if __name__ == "__main__":
    for N in (1, 5):
        for l2dist in (True, False):
            loss_golden_negatives(N, l2dist)
    print("reference size: loss_l2.npz", os.path.getsize(os.path.join(OUT, "loss_l2.npz")), "bytes")
