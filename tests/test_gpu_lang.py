"""-m gpu: language-reward head (batched 15-call MLP, csrc/lang.hip) + language InfoNCE, against the reference's own
Trainer.update run (tests/golden/loss_*.npz, G3) and against the CPU oracle for a full step with langweight = 1."""
import os
import sys

import numpy as np
import pytest
import torch

from util import infonce_torch as _infonce_torch, langrew_bf16_model, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lang_state(module):
    from oracle import detgen
    sd = {}
    full = module.state_dict()
    for k, v in full.items():
        fan_in = v.shape[1] if v.dim() == 2 else full[k.replace("bias", "weight")].shape[1]
        a = 1.0 / np.sqrt(fan_in)
        sd[k] = torch.from_numpy(detgen.uniform("lr" + k, tuple(v.shape), -a, a))
    return sd


@pytest.mark.parametrize("l2dist", [True, False])
def test_full_loss_with_language_matches_reference_golden(hip, golden_dir, l2dist):
    from oracle import detgen
    from r3m_amd import ops
    from r3m_amd.models_language import LanguageReward
    sys.path.insert(0, golden_dir)
    from make_golden import make_alle
    g = np.load(os.path.join(golden_dir, f"loss_{'l2' if l2dist else 'cos'}.npz"))
    B, D = 8, 512
    rew = LanguageReward(None, D, 1024, 768)
    assert list(rew.state_dict().keys()) == [f"pred.{i}.{p}" for i in (0, 2, 4, 6, 8) for p in ("weight", "bias")]
    rew.load_state_dict(_lang_state(rew))
    rew = rew.to(DEV)
    alle = torch.from_numpy(make_alle(B, D, "alle")).to(DEV).requires_grad_(True)
    feats = torch.from_numpy(detgen.uniform("langfeat", (B, 768), -0.6, 0.6)).to(DEV)
    mask = torch.ones(B)
    mask[5] = 0.0
    perms = torch.from_numpy(g["perms"])
    scores = rew.batched_scores(alle, feats, perms[0:9].to(torch.int32).to(DEV))
    e_max, _ = rel_err(scores.detach().cpu().numpy(), g["scores"])
    print("scores max-rel", e_max)
    assert e_max < 1e-5
    full, m = ops.r3m_loss(alle, perms[9:15].to(torch.int32).to(DEV), 1e-5, 1e-5, 1.0, l2dist=l2dist, scores=scores, mask=mask.to(DEV),
                           langweight=1.0)
    ref = dict(zip([str(n) for n in g["metric_names"]], g["metric_values"]))
    got = m.cpu().numpy()
    for k, v in ref.items():
        assert abs(got[ops.METRIC_SLOTS[k]] - v) <= 1e-5 * max(1.0, abs(v)), (k, got[ops.METRIC_SLOTS[k]], v)
    rew.mark_grads_stale()
    full.backward()
    e_max, e_l2 = rel_err(alle.grad.cpu().numpy(), g["dalle"])
    print(f"dalle max-rel {e_max:.3e} l2-rel {e_l2:.3e}")
    assert e_max < 1e-4
    P = dict(rew.named_parameters())
    for k, p in P.items():
        ref_n = float(g["gradnorm_" + k])
        assert abs(float(p.grad.double().norm()) - ref_n) <= 1e-4 * max(ref_n, 1e-12), k
    assert rel_err(P["pred.8.weight"].grad.cpu().numpy(), g["grad_pred.8.weight"])[0] < 1e-4
    assert rel_err(P["pred.0.bias"].grad.cpu().numpy(), g["grad_pred.0.bias"])[0] < 1e-4
    # single-call API (reference signature) agrees with the batched rows
    e0, eg = alle.detach()[:, 0], alle.detach()[:, 1]
    s1, info = rew(e0, eg, feats)
    assert info == {} and rel_err(s1.detach().cpu().numpy(), g["scores"][0])[0] < 1e-5


def test_full_step_with_language_vs_oracle(hip):
    """BASELINE config 3 shape of the step (langweight=1, L1=1e-5, frozen text features) on ResNet-18, B=4, vs the CPU oracle."""
    from oracle import detgen, r3m_ref
    from r3m_amd import R3M
    from r3m_amd.parallel import SingleDevice
    from r3m_amd.trainer import Trainer
    B = 4
    m = R3M("cuda", 1e-4, 1024, size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=1.0)
    shapes = [(k, tuple(v.shape)) for k, v in m.convnet.state_dict().items()]
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes).items()}
    m.convnet.load_state_dict(sd)
    lsd = _lang_state(m.lang_rew)
    m.lang_rew.load_state_dict(lsd)
    ref = r3m_ref.R3MRef(size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=1.0)
    ref.convnet.load_state_dict(sd)
    ref.lang_rew.load_state_dict(lsd)
    model = SingleDevice(m).to(DEV)
    frames = torch.from_numpy(detgen.frames("langstep", (B, 5, 3, 224, 224)))
    feats = torch.from_numpy(detgen.uniform("langfeat", (B, 768), -0.6, 0.6))
    mask = torch.tensor([1.0, 1.0, 0.0, 1.0])
    torch.manual_seed(5)
    lang_perm = torch.stack([torch.randperm(B) for _ in range(9)])
    tcn_perm = torch.stack([torch.randperm(B) for _ in range(6)])
    torch.manual_seed(5)
    metrics, _ = Trainer(1).update(model, (frames.to(DEV), (feats.to(DEV), mask)), 0)
    mref = r3m_ref.train_step_ref(ref, frames, tcn_perm=tcn_perm, lang_feats=feats, lang_mask=mask, lang_perm=lang_perm)
    assert set(metrics.keys()) == set(mref.keys())
    for k, v in mref.items():
        assert abs(metrics[k] - v) <= 2e-4 * max(1.0, abs(v)), (k, metrics[k], v)
    # post-step language-head weights (Adam moved them by ~lr each)
    w_gpu = m.lang_rew.state_dict()["pred.8.weight"].cpu()
    w_ref = ref.lang_rew.state_dict()["pred.8.weight"]
    d = (w_gpu - w_ref).abs()
    assert float(d.max()) <= 2.1e-4 and float((d > 2e-5).float().mean()) < 0.05


@pytest.mark.parametrize("B,D,H,LD", [(4, 64, 64, 32), (5, 512, 128, 768), (3, 2048, 1024, 768)])
def test_langrew_c_abi_vs_torch(hip, B, D, H, LD):
    """r3m_langrew_forward/backward through the C ABI vs a torch-CPU MLP evaluated call by call (models_language.py:43-55)."""
    from util import langrew_layers, langrew_scores_call_by_call, rnd
    layers = langrew_layers(D, H, LD, seed=0)
    alle = torch.relu(rnd((B, 5, D), 1, -0.5, 1.0)).requires_grad_(True)
    feats = rnd((B, LD), 2, -0.6, 0.6)
    g = torch.Generator().manual_seed(3)
    perm = torch.stack([torch.randperm(B, generator=g) for _ in range(9)])
    dscore = rnd((15, B), 4, -1.0, 1.0)
    scores_ref = langrew_scores_call_by_call(layers, alle, feats, perm)
    (scores_ref * dscore).sum().backward()

    flat = torch.cat([t.detach().reshape(-1) for l in layers for t in (l.weight, l.bias)])
    n = hip.r3m_langrew_num_params(D, H, LD)
    assert n == flat.numel()
    flat = torch.cat([flat, torch.zeros((-n) % 4)]).to(DEV)
    grads = torch.zeros_like(flat)
    wsb = hip.r3m_langrew_workspace_bytes(B, D, H, LD)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    alled, featsd = alle.detach().to(DEV), feats.to(DEV)
    permd = perm.to(torch.int32).to(DEV)
    from r3m_amd.ops import inverse_permutations
    ipermd = inverse_permutations(permd).contiguous()
    assert ipermd.dtype == torch.int32 and int(ipermd.min()) == 0 and int(ipermd.max()) == B - 1
    scores = torch.empty((15, B), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    rc = hip.r3m_langrew_forward(alled.data_ptr(), featsd.data_ptr(), permd.data_ptr(), flat.data_ptr(), scores.data_ptr(),
                                 ws.data_ptr(), wsb, B, D, H, LD, st)
    assert rc == 0, hip.r3m_last_error()
    assert rel_err(scores.cpu().numpy(), scores_ref.detach().numpy())[0] < 2e-5
    dalle = torch.zeros((B, 5, D), device=DEV)
    dsd = dscore.to(DEV)
    rc = hip.r3m_langrew_backward(dsd.data_ptr(), ipermd.data_ptr(), flat.data_ptr(), grads.data_ptr(), dalle.data_ptr(), ws.data_ptr(),
                                  wsb, B, D, H, LD, 0, st)
    assert rc == 0, hip.r3m_last_error()
    torch.cuda.synchronize()
    assert rel_err(dalle.cpu().numpy(), alle.grad.numpy())[0] < 1e-4
    gref = torch.cat([t.grad.reshape(-1) for l in layers for t in (l.weight, l.bias)])
    off = 0
    for l in layers:
        for t in (l.weight, l.bias):
            k = t.numel()
            e = rel_err(grads[off:off + k].cpu().numpy(), t.grad.reshape(-1).numpy())[0]
            assert e < 1e-4, (tuple(t.shape), e)
            off += k
    assert gref.numel() == n


def test_reference_style_15_call_loop_equals_batched(hip, golden_dir):
    """VERDICT r1 #1 / SURVEY A5: the reference's trainer calls model.module.get_reward 15 times WITH autograd
    (/root/reference/r3m/trainer.py:72-92, restated below call for call). Through the differentiable HIP
    LanguageReward.forward that loop must give the same scores, the same d loss/d embeddings and the same head gradients as
    the one-pass batched_scores() — and the scores of the reference's own run (golden G3)."""
    from oracle import detgen
    from r3m_amd import R3M
    sys.path.insert(0, golden_dir)
    from make_golden import make_alle
    g = np.load(os.path.join(golden_dir, "loss_l2.npz"))
    B, D = 8, 512
    m = R3M("cuda", 1e-4, 1024, size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=1.0)
    m.lang_rew.load_state_dict(_lang_state(m.lang_rew))
    m = m.to(DEV)
    rew = m.lang_rew
    feats = torch.from_numpy(detgen.uniform("langfeat", (B, 768), -0.6, 0.6)).to(DEV)
    mask = torch.ones(B, device=DEV)
    mask[5] = 0.0
    perms = torch.from_numpy(g["perms"])[0:9]

    # ---- the reference's loop (trainer.py:70-92), 15 autograd calls through R3M.get_reward ----
    alle = torch.from_numpy(make_alle(B, D, "alle")).to(DEV).requires_grad_(True)
    e0, eg, es0, es1, es2 = (alle[:, i] for i in range(5))
    rows = [None] * 15
    rows[0] = m.get_reward(e0, eg, feats)[0]
    rows[1] = m.get_reward(e0, es1, feats)[0]
    rows[2] = m.get_reward(e0, es2, feats)[0]
    rows[3] = m.get_reward(e0, e0, feats)[0]
    rows[4] = m.get_reward(e0, es0, feats)[0]
    rows[5] = m.get_reward(e0, es1, feats)[0]
    for k in range(3):
        for j, other in enumerate((eg, es1, es2)):
            pi = perms[3 * k + j].to(DEV)
            rows[6 + 3 * k + j] = m.get_reward(e0[pi], other[pi], feats)[0]
    assert all(r.shape == (B,) and r.requires_grad for r in rows)
    loop_scores = torch.stack(rows)
    assert rel_err(loop_scores.detach().cpu().numpy(), g["scores"])[0] < 1e-5        # the reference's own scores
    m.encoder_opt.zero_grad()
    _infonce_torch(loop_scores, mask).backward()
    assert rew.has_grads()
    dalle_loop = alle.grad.clone()
    grads_loop = rew.flat_grads().clone()

    # ---- the batched pass under the same loss ----
    alle2 = torch.from_numpy(make_alle(B, D, "alle")).to(DEV).requires_grad_(True)
    scores = rew.batched_scores(alle2, feats, perms.to(torch.int32).to(DEV))
    assert rel_err(loop_scores.detach().cpu().numpy(), scores.detach().cpu().numpy())[0] < 1e-6
    m.encoder_opt.zero_grad()
    _infonce_torch(scores, mask).backward()
    e_max, e_l2 = rel_err(dalle_loop.cpu().numpy(), alle2.grad.cpu().numpy())
    print(f"15-call loop vs batched: dalle max-rel {e_max:.3e} l2 {e_l2:.3e}")
    assert e_max < 1e-4
    gb = rew.flat_grads()
    for name, off, shape in rew._layout:
        n = int(np.prod(shape))
        if n == 1:      # pred.8.bias: the sum of d loss/d score over all scores — cancels to ~0 (each clip's InfoNCE gradients sum to 0)
            assert abs(float(grads_loop[off]) - float(gb[off])) < 1e-6
            continue
        e = rel_err(grads_loop[off:off + n].cpu().numpy(), gb[off:off + n].cpu().numpy())[0]
        assert e < 1e-4, (name, e)

    # ---- and the head really trains from the loop: one Adam step moves every tensor of the head ----
    before = rew.flat_params().clone()
    m.encoder_opt.step()
    moved = (rew.flat_params() - before).abs()
    for name, off, shape in rew._layout:
        n = int(np.prod(shape))
        assert float(moved[off:off + n].max()) > 0, name


def test_single_call_reward_edge_cases(hip):
    """LanguageReward.forward: B = 1 collapses to a 0-d score like the reference's .squeeze() (models_language.py:55); no-grad
    calls work; wrong shapes raise; gradient w.r.t. the text features is available too."""
    from r3m_amd.models_language import LanguageReward
    rew = LanguageReward(None, 64, 64, 32)
    rew.load_state_dict(_lang_state(rew))
    rew = rew.to(DEV)
    g = torch.Generator().manual_seed(4)
    e0, eg, le = torch.rand((1, 64), generator=g).to(DEV), torch.rand((1, 64), generator=g).to(DEV), torch.rand((1, 32), generator=g).to(DEV)
    s, info = rew(e0, eg, le)
    assert s.dim() == 0 and info == {}
    with torch.no_grad():
        s2, _ = rew(e0, eg, le)
    assert float(s) == float(s2) and not s2.requires_grad
    with pytest.raises(ValueError):
        rew(e0[:, :32], eg, le)
    # torch-CPU MLP as the checker, all three input gradients
    import torch.nn as nn
    P = {k: v.detach().cpu() for k, v in rew.state_dict().items()}
    x = [t.detach().cpu().repeat(3, 1).clone().requires_grad_(True) for t in (e0, eg, le)]
    h = torch.cat(x, -1)
    for li in (0, 2, 4, 6):
        h = torch.relu(h @ P[f"pred.{li}.weight"].t() + P[f"pred.{li}.bias"])
    ref = (h @ P["pred.8.weight"].t() + P["pred.8.bias"]).squeeze()
    ref.sum().backward()
    xg = [t.detach().repeat(3, 1).clone().requires_grad_(True) for t in (e0, eg, le)]
    rew.mark_grads_stale()
    sg, _ = rew(*xg)
    sg.sum().backward()
    assert rel_err(sg.detach().cpu().numpy(), ref.detach().numpy())[0] < 1e-5
    for a, b in zip(xg, x):
        assert rel_err(a.grad.cpu().numpy(), b.grad.numpy())[0] < 1e-4


@pytest.mark.parametrize("D", [512, 2048])
def test_single_call_reward_matches_reference_golden(hip, golden_dir, D):
    """G4: LanguageReward.forward (the differentiable single call, csrc/lang.hip r3m_langrew_call_*) against the REFERENCE's
    LanguageReward forward + backward at both head widths (tests/golden/langrew_d{512,2048}.npz)."""
    from oracle import detgen
    from r3m_amd.models_language import LanguageReward
    g = np.load(os.path.join(golden_dir, f"langrew_d{D}.npz"))
    rew = LanguageReward(None, D, 1024, 768)
    rew.load_state_dict(_lang_state(rew))
    rew = rew.to(DEV)
    B = 4
    e0 = torch.from_numpy(np.maximum(detgen.uniform(f"g4e0_{D}", (B, D), -0.3, 1.0), 0)).to(DEV).requires_grad_(True)
    eg = torch.from_numpy(np.maximum(detgen.uniform(f"g4eg_{D}", (B, D), -0.3, 1.0), 0)).to(DEV).requires_grad_(True)
    le = torch.from_numpy(detgen.uniform(f"g4le_{D}", (B, 768), -0.6, 0.6)).to(DEV)
    score, _ = rew(e0, eg, le)
    assert rel_err(score.detach().cpu().numpy(), g["score"])[0] < 1e-5
    rew.mark_grads_stale()
    (score * torch.from_numpy(detgen.uniform("g4cw", (B,), 0.5, 1.5)).to(DEV)).sum().backward()
    assert rel_err(e0.grad.cpu().numpy(), g["de0"])[0] < 1e-4 and rel_err(eg.grad.cpu().numpy(), g["deg"])[0] < 1e-4
    P = dict(rew.named_parameters())
    for k, p in P.items():
        ref_n = float(g["gradnorm_" + k])
        assert abs(float(p.grad.double().norm()) - ref_n) <= 1e-4 * max(ref_n, 1e-12), k
    assert rel_err(P["pred.8.weight"].grad.cpu().numpy(), g["grad_pred.8.weight"])[0] < 1e-4
    assert rel_err(P["pred.0.bias"].grad.cpu().numpy(), g["grad_pred.0.bias"])[0] < 1e-4


def test_step_with_sentence_strings_runs_the_text_model_once(hip):
    """SURVEY §8(f)2 end to end on the GPU: Trainer.update fed SENTENCES (list[str], '' = no language -> masked, trainer.py:107-109)
    runs the frozen text model ONCE for the step's 15 reward evaluations, and gives the same metrics as feeding the features."""
    from oracle import detgen, tiny_text
    from r3m_amd import R3M
    from r3m_amd.parallel import SingleDevice
    from r3m_amd.trainer import Trainer
    B = 4
    sents = [tiny_text.SENTENCES[i] for i in (0, 1, 2, 3)]            # index 2 is '' (masked clip)
    res = {}
    for mode in ("strings", "features"):
        m = R3M("cuda", 1e-4, 1024, size=18, l2weight=1e-5, l1weight=1e-5, langweight=1.0, tcnweight=1.0)
        shapes = [(k, tuple(v.shape)) for k, v in m.convnet.state_dict().items()]
        m.convnet.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes).items()})
        m.lang_rew.load_state_dict(_lang_state(m.lang_rew))
        model = SingleDevice(m).to(DEV)
        m.lang_enc.device = DEV
        m.lang_enc.use_backend(tiny_text.WhitespaceTokenizer(), tiny_text.tiny_distilbert())
        frames = torch.from_numpy(detgen.frames("langstep", (B, 5, 3, 224, 224))).to(DEV)
        torch.manual_seed(5)
        if mode == "strings":
            met, _ = Trainer(1).update(model, (frames, sents), 0)
            assert m.lang_enc.encoder_calls == 1
        else:
            feats = m.lang_enc(sents)
            mask = torch.tensor([1.0 * (s != "") for s in sents])
            met, _ = Trainer(1).update(model, (frames, (feats, mask)), 0)
        res[mode] = met
    assert res["strings"].keys() == res["features"].keys()
    for k in res["strings"]:
        assert res["strings"][k] == res["features"][k], k


@pytest.mark.parametrize("B,D", [(3, 512), (16, 2048)])
def test_bf16_head_follows_fp32_head_and_its_own_rounding_model(hip, B, D):
    """LanguageReward(precision="bf16") (r3m_langrew_*_dt with R3M_DT_BF16): the batched pass with bf16 storage of the MLP's tensors and
    bf16 GEMM operands. Checker 1 = the fp32 head on the same inputs (scores and gradients follow it to bf16 accuracy). Checker 2 = a
    float64 torch MLP with a bf16 rounding exactly where the kernel stores bf16 (input rows, weights, every hidden activation):
    the forward must match THAT to accumulation accuracy — a wrong layout / missing bias / wrong mask cannot hide in bf16 noise."""
    from oracle import detgen
    from r3m_amd.models_language import LanguageReward
    H, LD = 1024, 768
    torch.manual_seed(11)
    perm = torch.stack([torch.randperm(B) for _ in range(9)]).to(torch.int32).to(DEV)
    alle0 = torch.from_numpy(detgen.uniform("alle16", (B, 5, D), -1.0, 1.0))
    feats = torch.from_numpy(detgen.uniform("langfeat16", (B, LD), -0.6, 0.6)).to(DEV)
    wts = torch.from_numpy(detgen.uniform("dscore16", (15, B), -1.0, 1.0)).to(DEV)
    res = {}
    for prec in ("fp32", "bf16"):
        rew = LanguageReward(None, D, H, LD, precision=prec)
        rew.load_state_dict(_lang_state(rew))
        rew = rew.to(DEV)
        alle = alle0.clone().to(DEV).requires_grad_(True)
        scores = rew.batched_scores(alle, feats, perm)
        rew.mark_grads_stale()
        (scores * wts).sum().backward()
        res[prec] = (scores.detach().double().cpu(), alle.grad.double().cpu(), rew.flat_grads().double().cpu().clone(), rew)

    def cos(a, b):
        return float((a * b).sum() / (a.norm() * b.norm()))
    s32, da32, g32, rew32 = res["fp32"]
    s16, da16, g16, _ = res["bf16"]
    print(f"bf16 head B={B} D={D}: scores max|d| {float((s16 - s32).abs().max()):.3e} (max|s| {float(s32.abs().max()):.3f}); "
          f"cos dalle {cos(da16, da32):.6f}, cos param grads {cos(g16, g32):.6f}")
    assert float((s16 - s32).abs().max()) <= 2e-2 * max(1.0, float(s32.abs().max()))
    assert cos(da16, da32) >= 0.99 and cos(g16, g32) >= 0.99

    # checker 2: float64 MLP with the kernel's rounding points (straight-through in the backward pass)
    wb = [tuple(rew32.state_dict()[f"pred.{li}.{pn}"].double().cpu().clone().requires_grad_(True) for pn in ("weight", "bias")) for li in (0, 2, 4, 6, 8)]
    s_model, da_model, g_model = langrew_bf16_model(wb, alle0, feats, perm, wts)
    err = float((s16 - s_model).abs().max())
    n = g_model.numel()
    print(f"bf16 head vs its float64 rounding model: scores max|d| {err:.3e}; cos dalle {cos(da16, da_model):.6f}, cos param grads "
          f"{cos(g16[:n], g_model):.6f} (fp32 head vs the same model: {cos(da32, da_model):.6f} / {cos(g32[:n], g_model):.6f})")
    assert err <= 2e-3 * max(1.0, float(s_model.abs().max()))
    assert cos(da16, da_model) >= 0.999 and cos(g16[:n], g_model) >= 0.999
