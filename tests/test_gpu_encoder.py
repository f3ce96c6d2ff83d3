"""-m gpu: the HIP encoder engine / loss / full step against the committed golden vectors (made by the reference's own code,
tests/golden/make_golden.py) and against the CPU oracle at other sizes. Gate: encoder outputs max|d|/max|ref| <= 1e-4
(BASELINE.json north_star: 'within 1e-4 rel-err of CPU reference'), fp32."""
import os

import numpy as np
import pytest
import torch

from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def report(line):
    """Parity numbers also go to gpurun_out/parity.txt (kept with the profiles; print() is lost under xdist)."""
    print(line)
    try:
        os.makedirs(os.path.join(_ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(_ROOT, "gpurun_out", "parity.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _load_state(convnet, tag="w"):
    from oracle import detgen
    shapes = [(k, tuple(v.shape)) for k, v in convnet.state_dict().items()]
    sd = detgen.resnet_state_dict(shapes, tag)
    convnet.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})


def _last_bn(size):
    return "layer4.2.bn3" if size == 50 else ("layer4.1.bn2" if size == 18 else "layer4.2.bn2")


def _float64_grads_with_decisions(size, flip_idx, keys):
    """Float64 oracle gradients of the G1 case with the last block's ReLU decided as the HIP forward decided it at the listed
    elements (flat NCHW index into the block's pre-ReLU sum, float64_was_on): on -> forced off (output 0, no gradient), off ->
    forced on (pass-through). Runs on the GPU box's CPU (seconds)."""
    from oracle import detgen, r3m_ref
    ref = r3m_ref.R3MRef(size=size, langweight=0.0, tcnweight=1.0)
    shapes = [(k, tuple(v.shape)) for k, v in ref.convnet.state_dict().items()]
    ref.convnet.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in detgen.resnet_state_dict(shapes, "w").items()})
    ref = ref.double()
    ref.train()
    net = ref.convnet
    blk = net.layer4[-1]
    off = torch.tensor([i for i, was_on in flip_idx if was_on], dtype=torch.long)
    on = torch.tensor([i for i, was_on in flip_idx if not was_on], dtype=torch.long)

    class Forced(torch.nn.Module):
        def __init__(self, nth):
            super().__init__()
            self.nth, self.k = nth, 0

        def forward(self, z):
            self.k += 1
            y = torch.relu(z)
            if self.k == self.nth:                         # the block's LAST ReLU (after the residual add)
                flat_z, flat_y = z.flatten(), y.flatten().clone()
                if len(on):
                    flat_y[on] = flat_z[on]
                if len(off):
                    flat_y[off] = 0.0
                y = flat_y.view_as(z)
            return y

    blk.relu = Forced(3 if size == 50 else 2)
    x = torch.from_numpy(detgen.frames("frames8", (8, 3, 224, 224))).double()
    h = net(ref.normlayer(x / 255.0))
    cw = torch.from_numpy(detgen.uniform("cw", tuple(h.shape), 0.5, 1.5)).double()
    (h * cw).sum().backward()
    P = dict(net.named_parameters())
    return {k: P[k].grad.numpy() for k in keys}


@pytest.mark.parametrize("size", [18, 34, 50])
def test_encoder_matches_reference_golden(hip, golden_dir, size):
    from oracle import detgen
    from r3m_amd import R3M
    g = np.load(os.path.join(golden_dir, f"encoder_r{size}.npz"))
    m = R3M("cuda", 1e-4, 1024, size=size, langweight=0.0, tcnweight=1.0)
    _load_state(m.convnet)
    m = m.to(DEV)
    x = torch.from_numpy(detgen.frames("frames8", (8, 3, 224, 224))).to(DEV)
    m.eval()
    with torch.no_grad():
        h_eval = m(x).cpu().numpy()
    e_max, e_l2 = rel_err(h_eval, g["h_eval"])
    report(f"r{size} eval: max-rel {e_max:.3e} l2-rel {e_l2:.3e}")
    assert e_max <= 1e-4
    m.train()
    h = m(x)
    e_max, e_l2 = rel_err(h.detach().cpu().numpy(), g["h_train"])
    report(f"r{size} train: max-rel {e_max:.3e} l2-rel {e_l2:.3e}")
    assert e_max <= 1e-4
    sd = m.convnet.state_dict()
    lb = _last_bn(size)
    for k in ("bn1.running_mean", "bn1.running_var", lb + ".running_mean", lb + ".running_var"):
        assert rel_err(sd[k].cpu().numpy(), g["post_" + k])[0] < 1e-4, k
    assert int(sd["bn1.num_batches_tracked"]) == 1
    cw = torch.from_numpy(detgen.uniform("cw", tuple(h.shape), 0.5, 1.5)).to(DEV)
    (h * cw).sum().backward()
    P = dict(m.convnet.named_parameters())
    # Gradient gate. fp32 round-off is amplified through 18-50 train-mode BatchNorm backward passes: the reference's OWN
    # PyTorch-CPU fp32 gradients sit 5e-3 (ResNet-18/34) to 2e-2 (ResNet-50) l2-rel away from a float64 evaluation of the
    # same graph at conv1 (tests/golden/encoder_r*_fp64.npz, printed by make_golden.py). So the HIP gradients are gated
    # against float64 truth at <= 3x the reference-fp32 error of the same tensor (floor 1e-4), not fp32 against fp32. Measured
    # ratios (profiles/r03_parity_report.txt): ResNet-18 1.0-1.6, ResNet-50 1.0-1.4, ResNet-34 2.1-2.6 on every early-layer tensor. The
    # ResNet-34 figure is not scatter and not a reduction defect: the HIP forward decides ONE ReLU of the last block differently from
    # float64 (z = +3.4e-5, the kink table below), which the reference's CPU evaluation happens not to; that one flipped element
    # (1 of 200 704, ~2e-3 of |dz|) is carried down through 33 BatchNorm backward passes like any other fp32 perturbation and adds
    # ~8e-3 to every early tensor (sqrt(9.4e-3^2 - 4.4e-3^2)); ResNet-18 / 50 have no flip that the reference does not share.
    g64 = np.load(os.path.join(golden_dir, f"encoder_r{size}_fp64.npz"))
    worst_hip = worst_cpu = 0.0
    for name, n32, n64 in zip(g["grad_names"], g["grad_norms"], g64["grad_norms"]):
        got = float(P[str(name)].grad.double().norm())
        worst_hip = max(worst_hip, abs(got - n64) / max(n64, 1e-12))
        worst_cpu = max(worst_cpu, abs(n32 - n64) / max(n64, 1e-12))
    report(f"r{size} grad-norm worst rel vs fp64: hip {worst_hip:.3e}  reference-cpu-fp32 {worst_cpu:.3e}")
    assert worst_hip <= max(3.0 * worst_cpu, 1e-4)   # no blanket floor: the reference-fp32 error of the same tensors sets the scale
    # Last BatchNorm: its gradients are gated UP TO ReLU decisions of the last block on elements whose float64 pre-activation lies
    # within 2e-4 of zero (tests/golden/encoder_r*_kink.npz). VERDICT r1 weak #3: ResNet-34's d(gamma) sat 1.3e-3 from float64
    # while the reference's CPU fp32 sat at 1e-6 — that is ONE element (z = +3.4e-5 in float64, decided <= 0 by the fp32 forward
    # here; tools/experiments/debug_r34_lastbn.py reproduces 1.344e-3 / 1.807e-4 to all digits), not a reduction defect. A flip is
    # identified on d(beta) (it moves that channel by exactly dz of the element) and then applied to d(gamma): both gradients must
    # be explained by the SAME decisions; what remains is gated at max(4 x reference-fp32 error, 1e-4) — no blanket floor.
    kink = np.load(os.path.join(golden_dir, f"encoder_r{size}_kink.npz"))
    r_b = P[lb + ".bias"].grad.cpu().double().numpy() - g64["grad_" + lb + ".bias"].astype(np.float64)
    r_g = P[lb + ".weight"].grad.cpu().double().numpy() - g64["grad_" + lb + ".weight"].astype(np.float64)
    flips, flip_idx = [], []
    for c, z, dgam, dbet, fi in zip(kink["channel"], kink["z"], kink["dgamma"], kink["dbeta"], kink["idx"]):
        sgn = -1.0 if z > 0 else 1.0                       # float64 had it on (off): deciding otherwise removes (adds) its term
        if abs(r_b[c] - sgn * dbet) < 0.25 * abs(dbet):    # the channel's d(beta) residual IS this element's dz
            r_b[c] -= sgn * dbet
            r_g[c] -= sgn * dgam
            flips.append((int(c), float(z)))
            flip_idx.append((int(fi), bool(z > 0)))
    n_b = float(np.linalg.norm(g64["grad_" + lb + ".bias"].astype(np.float64)))
    n_g = float(np.linalg.norm(g64["grad_" + lb + ".weight"].astype(np.float64)))
    report(f"r{size} last BatchNorm: {len(flips)} ReLU decision(s) differ from float64 at |z| < {float(kink['tau']):.0e}: {flips}; "
           f"after accounting for them d(gamma) l2-rel {np.linalg.norm(r_g) / n_g:.3e}, d(beta) {np.linalg.norm(r_b) / n_b:.3e}")
    # ResNet-50's train-mode forward sits 2.6e-5 (max-rel of the activation scale) from float64 against 3-8e-6 for ResNet-18/34, so
    # more of its 82 table entries are decided differently (measured 15; ResNet-18: 2, ResNet-34: 1)
    assert len(flips) <= max(3, len(kink["z"]) // 4)
    keys = ("conv1.weight", "bn1.weight", "bn1.bias", lb + ".weight", lb + ".bias", "layer1.0.conv1.weight",
            "layer2.0.downsample.0.weight")
    # A flipped decision of the LAST block is not confined to the last BatchNorm: the element's dz (1 of 200 704, ~2e-3 of |dz|)
    # travels down through every BatchNorm backward like any other perturbation and reaches conv1 amplified — measured on
    # ResNet-34: one flip -> conv1.weight 2.1x the reference-fp32 error, two flips (round 3, after an fp32 reassociation in the
    # 3x3 kernels moved z[37] = -1.1e-4 across zero as well) -> 3.3x. So when a tensor misses the 3x gate and flips were
    # identified, the float64 oracle is evaluated HERE, on this box's CPU, with exactly those decisions imposed
    # (_float64_grads_with_decisions), and the gate is applied against THAT: the HIP gradients must equal the float64 gradients
    # of the network that makes the same ReLU decisions, to 3x the reference's own fp32 error.
    forced = None
    for k in keys:
        hip_err = rel_err(P[k].grad.cpu().numpy(), g64["grad_" + k])[1]
        cpu_err = rel_err(g["grad_" + k], g64["grad_" + k])[1]
        report(f"r{size} grad {k}: l2-rel vs fp64: hip {hip_err:.3e}  reference-cpu-fp32 {cpu_err:.3e}")
        if k == lb + ".weight":
            hip_err = float(np.linalg.norm(r_g) / n_g)
        elif k == lb + ".bias":
            hip_err = float(np.linalg.norm(r_b) / n_b)
        if hip_err > max(3.0 * cpu_err, 1e-4) and flip_idx and k not in (lb + ".weight", lb + ".bias"):
            if forced is None:
                forced = _float64_grads_with_decisions(size, flip_idx, keys)
            hip_err = rel_err(P[k].grad.cpu().numpy(), forced[k])[1]
            report(f"r{size} grad {k}: l2-rel vs fp64 WITH the {len(flip_idx)} identified ReLU decision(s) imposed: hip {hip_err:.3e}")
        assert hip_err <= max(3.0 * cpu_err, 1e-4), k


@pytest.mark.parametrize("l2dist", [True, False])
def test_tcn_lp_loss_matches_reference_golden(hip, golden_dir, l2dist):
    """G3 (TCN + LP part): same embeddings and permutations as the reference's Trainer.update run."""
    from r3m_amd import ops
    g = np.load(os.path.join(golden_dir, f"loss_{'l2' if l2dist else 'cos'}.npz"))
    import sys
    sys.path.insert(0, golden_dir)
    from make_golden import make_alle
    B, D = 8, 512
    alle = torch.from_numpy(make_alle(B, D, "alle")).to(DEV).requires_grad_(True)
    perms = torch.from_numpy(g["perms"])
    tcn_perm = perms[9:15].to(torch.int32).to(DEV)
    full, m = ops.r3m_loss(alle, tcn_perm, 1e-5, 1e-5, 1.0, l2dist=l2dist)
    names = [str(n) for n in g["metric_names"]]
    ref = dict(zip(names, g["metric_values"]))
    got = m.cpu().numpy()
    for k in ("l2loss", "l1loss", "l0loss", "tcnloss", "aligned"):
        assert abs(got[ops.METRIC_SLOTS[k]] - ref[k]) <= 1e-5 * max(1.0, abs(ref[k])), (k, got[ops.METRIC_SLOTS[k]], ref[k])
    # the golden full_loss / dalle include the language term; its part is checked in test_gpu_lang.py. Here: oracle on CPU.
    from oracle import r3m_ref
    mref = r3m_ref.R3MRef(size=18, l2weight=1e-5, l1weight=1e-5, langweight=0.0, tcnweight=1.0, l2dist=l2dist)
    a2 = alle.detach().cpu().requires_grad_(True)
    fl, met, _ = r3m_ref.r3m_loss_ref(mref, a2, tcn_perm=perms[9:15])
    fl.backward()
    assert abs(float(full) - met["full_loss"]) <= 1e-5 * abs(met["full_loss"])
    full.backward()
    e_max, e_l2 = rel_err(alle.grad.cpu().numpy(), a2.grad.numpy())
    report(f"loss grad l2dist={l2dist}: max-rel {e_max:.3e} l2-rel {e_l2:.3e}")
    assert e_max < 1e-4


@pytest.mark.parametrize("size", [18, 34, 50])
def test_full_step_matches_reference_golden(hip, golden_dir, size):
    """G5: two Trainer.update steps (encoder + loss + backward + Adam), B = 2 clips, ResNet-18 / 34 / 50 (the reference's own
    Trainer.update + torch.optim.Adam on CPU made the vectors: tests/golden/make_golden.py::step_golden)."""
    from oracle import detgen
    from r3m_amd import R3M
    from r3m_amd.parallel import SingleDevice
    from r3m_amd.trainer import Trainer
    g = np.load(os.path.join(golden_dir, f"step_r{size}.npz"))
    m = R3M("cuda", 1e-4, 1024, size=size, l2weight=1e-5, l1weight=1e-5, langweight=0.0, tcnweight=1.0)
    _load_state(m.convnet)
    model = SingleDevice(m).to(DEV)
    frames = torch.from_numpy(detgen.frames("stepframes", (2, 5, 3, 224, 224))).to(DEV)
    torch.manual_seed(77)
    T = Trainer(1)
    names = [str(n) for n in g["metric_names"]]
    after1 = {}
    for s in range(2):
        metrics, _ = T.update(model, (frames, [""] * 2), s)
        if s == 0:
            torch.cuda.synchronize()
            sd1 = m.convnet.state_dict()
            after1 = {k: sd1[k].detach().cpu().numpy().copy() for k in ("conv1.weight", "bn1.weight", "bn1.bias", _last_bn(size) + ".weight")}
        assert list(metrics.keys()) == names
        ref = dict(zip(names, g[f"metric_values_{s}"]))
        # step 0 sees identical weights: tight. Step 1 follows an Adam update whose first step moves every weight by
        # +-lr according to the SIGN of its gradient; fp32-noise-level gradients flip sign between any two fp32
        # implementations, so the second step's loss agrees to ~1e-3 only (chaotic, not a kernel property).
        # ResNet-50 (measured 1.0e-2 on tcnloss of step 1, ResNet-18 / 34 3e-4): 23.5 M weights each moved by +-lr with the sign of a
        # gradient that is round-off for many of them, then 53 train-mode BatchNorms over 10 frames
        tol = 2e-4 if s == 0 else (2e-2 if size == 50 else 5e-3)
        report(f"r{size} full step {s}: " + ", ".join(f"{k} {metrics[k]:.6g} (ref {ref[k]:.6g})" for k in names))
        for k in names:
            assert abs(metrics[k] - ref[k]) <= tol * max(1.0, abs(ref[k])), (s, k, metrics[k], ref[k])
    sd = m.convnet.state_dict()
    lr = 1e-4
    # After the FIRST Adam step every weight has moved by ~lr with the SIGN of its gradient: against the reference's weights only
    # the elements whose gradient is round-off in sign differ (by 2 lr). Gate: <= 2.1 lr and fewer than 15 % of the elements
    # beyond 0.2 lr (captured in `after1` below, inside the loop). After the SECOND step the updates come from gradients at weights
    # that already differ, and ResNet-50's conv1 / bn1 gradients sit 2e-2 from float64 in ANY fp32 evaluation (kink-free case
    # below) — measured 40 % of its bn1 elements beyond 0.2 lr against 5-11 % for ResNet-18 / 34 — so there only the bound of two
    # steps (<= 4.2 lr) is gated and the fraction is reported.
    fails = []
    for k, got1 in after1.items():
        ref1 = g["post1_" + k].reshape(-1)
        d = np.abs(got1.reshape(-1) - ref1)
        flipped = float((d > 0.2 * lr).mean())
        report(f"r{size} after step 1 {k}: max abs diff {d.max() / lr:.2f} lr, fraction beyond 0.2 lr {flipped:.3f}")
        if not (d.max() <= 2.1 * lr and flipped < 0.15):
            fails.append(("step1", k, float(d.max()), flipped))
    for k in ("bn1.weight", "bn1.bias", _last_bn(size) + ".weight", "conv1.weight"):
        got = sd[k].cpu().numpy().reshape(-1)[:50000]
        ref = g["post_" + k].reshape(-1)
        d = np.abs(got - ref)
        flipped = float((d > 0.2 * lr).mean())
        report(f"r{size} after step 2 {k}: max abs diff {d.max() / lr:.2f} lr, fraction beyond 0.2 lr {flipped:.3f}")
        if not d.max() <= 4 * lr * 1.05 or (size != 50 and not flipped < 0.15):
            fails.append(("step2", k, float(d.max()), flipped))
    assert not fails, fails
    # running statistics after TWO steps: 0.9 x (step-1 statistics, gated at 1e-4 by the encoder golden) + 0.1 x the statistics of
    # conv1 outputs under weights that already took one Adam step — and that step moves a weight by +-lr according to the SIGN of
    # its gradient (see above), so a few conv1 weights differ by 2 lr = 2e-4 from the reference's: 1e-4-level differences in the
    # second batch mean are the optimizer's chaos, not arithmetic (measured: ResNet-18 < 1e-4, ResNet-34 1.1e-4). ResNet-18 keeps
    # the 1e-4 gate it has always met; the chaos-free statement for all three sizes is the lr = 1e-7 golden below.
    for k in ("bn1.running_mean", "bn1.running_var"):
        assert rel_err(sd[k].cpu().numpy(), g["post_" + k])[0] < (1e-4 if size == 18 else 5e-4), k
    assert int(sd["bn1.num_batches_tracked"]) == 2


@pytest.mark.parametrize("size", [18, 34, 50])
def test_two_steps_small_lr_match_reference_golden(hip, golden_dir, size):
    """G9: the G5 case at lr = 1e-7 (tests/golden/make_golden.py::step_small_lr_golden, the reference's own Trainer.update +
    torch.optim.Adam): no Adam sign chaos, so the TWO-step pipeline of every size — second forward on updated running statistics,
    Adam's moments, num_batches_tracked — is gated at fp32 tolerances: metrics of both steps 2e-4, running statistics 1e-4, and
    exp_avg / exp_avg_sq of conv1.weight and of the last BatchNorm's weight after each step (exp_avg after step 1 = 0.1 x the
    gradient: gated against the reference at the tolerance the kink-free gradient test establishes for the same tensors)."""
    from oracle import detgen
    from r3m_amd import R3M
    from r3m_amd.parallel import SingleDevice
    from r3m_amd.trainer import Trainer
    g = np.load(os.path.join(golden_dir, f"step_r{size}_lr1e-7.npz"))
    lr = float(g["lr"])
    m = R3M("cuda", lr, 1024, size=size, l2weight=1e-5, l1weight=1e-5, langweight=0.0, tcnweight=1.0)
    _load_state(m.convnet)
    model = SingleDevice(m).to(DEV)
    frames = torch.from_numpy(detgen.frames("stepframes", (2, 5, 3, 224, 224))).to(DEV)
    torch.manual_seed(77)
    T = Trainer(1)
    names = [str(n) for n in g["metric_names"]]
    lb = _last_bn(size)
    P = dict(m.convnet.named_parameters())
    for s in range(2):
        metrics, _ = T.update(model, (frames, [""] * 2), s)
        torch.cuda.synchronize()
        ref = dict(zip(names, g[f"metric_values_{s}"]))
        report(f"r{size} lr=1e-7 step {s}: " + ", ".join(f"{k} {metrics[k]:.6g} (ref {ref[k]:.6g})" for k in names))
        for k in names:
            assert abs(metrics[k] - ref[k]) <= 2e-4 * max(1.0, abs(ref[k])), (s, k, metrics[k], ref[k])
        for pname, key in (("conv1.weight", "conv1"), (lb + ".weight", "lastbn")):
            mom = m.encoder_opt.moments(P[pname])
            assert mom is not None
            ea, eas = mom[0].cpu().numpy(), mom[1].cpu().numpy()
            e1 = rel_err(ea, g[f"exp_avg_{key}_{s}"])
            e2 = rel_err(eas, g[f"exp_avg_sq_{key}_{s}"])
            report(f"r{size} lr=1e-7 step {s} Adam moments of {pname}: exp_avg max-rel {e1[0]:.3e} l2 {e1[1]:.3e}, exp_avg_sq max-rel {e2[0]:.3e} l2 {e2[1]:.3e}")
            # the reference's own fp32 gradient of conv1 sits 3e-3 (ResNet-18) .. 2e-2 (ResNet-50) l2-rel from float64 (G8): two fp32
            # evaluations agree to that, not to 1e-4; the last BatchNorm's gradient is exact to 1e-4
            # (measured l2-rel: conv1 5e-3 / 1.1e-2 / 2.4e-2, last BatchNorm 1e-5 / 1.4e-4 / 2.3e-3 for ResNet-18 / 34 / 50: ResNet-50's last
            # BatchNorm sits behind a 2048-channel bottleneck whose fp32 gradient is itself 1e-3 from float64, G8)
            tol = (6e-2 if size == 50 else 3e-2) if key == "conv1" else (6e-3 if size == 50 else 2e-3)
            assert e1[1] < tol and e2[1] < 2 * tol, (s, pname, e1, e2)
    sd = m.convnet.state_dict()
    for k in ("bn1.running_mean", "bn1.running_var", lb + ".running_mean", lb + ".running_var"):
        e = rel_err(sd[k].cpu().numpy(), g["post_" + k])[0]
        report(f"r{size} lr=1e-7 after two steps {k}: max-rel {e:.3e}")
        assert e < 1e-4, (k, e)
    for k in ("bn1.weight", lb + ".weight", "conv1.weight"):
        d = np.abs(sd[k].cpu().numpy() - g["post_" + k]).max()
        assert d <= 2.1 * 2 * lr, (k, d)          # two steps of at most ~lr each, whatever the signs
    assert int(sd["bn1.num_batches_tracked"]) == 2 == int(g["nbt"])


def test_encoder_large_batch_properties(hip):
    """Full-size-ish properties that need no oracle: batch independence in eval mode, determinism, non-negativity."""
    from r3m_amd import R3M
    torch.manual_seed(0)
    m = R3M("cuda", 1e-4, 1024, size=50, langweight=0.0, tcnweight=1.0).to(DEV)
    m.eval()
    x = torch.randint(0, 256, (40, 3, 224, 224), device=DEV).float()
    with torch.no_grad():
        h1 = m(x)
        h2 = m(x)
        h3 = m(x[8:24])
    assert torch.equal(h1, h2)                      # bit-reproducible
    assert (h1 >= 0).all()                          # avg-pool of ReLU
    torch.testing.assert_close(h1[8:24], h3, rtol=1e-5, atol=1e-6)   # eval-mode frames are independent


@pytest.mark.parametrize("B", [1, 3])
def test_small_ragged_batches_vs_oracle(hip, B):
    """Edge sizes: a single clip (every permutation is the identity: negatives at distance 0, sub-gradient 0) and an odd
    batch (5B frames not a multiple of any tile size) — one full step against the CPU oracle."""
    from oracle import detgen, r3m_ref
    from r3m_amd import R3M
    from r3m_amd.parallel import SingleDevice
    from r3m_amd.trainer import Trainer
    m = R3M("cuda", 1e-4, 1024, size=18, l2weight=1e-5, l1weight=1e-5, langweight=0.0, tcnweight=1.0)
    _load_state(m.convnet)
    ref = r3m_ref.R3MRef(size=18, l2weight=1e-5, l1weight=1e-5, langweight=0.0, tcnweight=1.0)
    ref.convnet.load_state_dict({k: v.cpu() for k, v in m.convnet.state_dict().items()})
    model = SingleDevice(m).to(DEV)
    frames = torch.from_numpy(detgen.frames(f"ragged{B}", (B, 5, 3, 224, 224)))
    torch.manual_seed(11)
    perms = torch.stack([torch.randperm(B) for _ in range(6)])
    torch.manual_seed(11)
    metrics, _ = Trainer(1).update(model, (frames.to(DEV), [""] * B), 0)
    mref = r3m_ref.train_step_ref(ref, frames, tcn_perm=perms)
    for k, v in mref.items():
        assert abs(metrics[k] - v) <= 2e-4 * max(1.0, abs(v)), (B, k, metrics[k], v)
    assert all(np.isfinite(v) for v in metrics.values())
    sd = m.convnet.state_dict()
    assert torch.isfinite(sd["conv1.weight"]).all() and int(sd["bn1.num_batches_tracked"]) == 1


@pytest.mark.parametrize("size,F,precision", [(18, 8, "fp32"), (18, 1, "fp32"), (34, 5, "fp32"), (50, 3, "fp32"), (50, 4, "bf16"), (34, 8, "bf16")])
def test_fused_and_standalone_bn_backward_reduce_agree(hip, size, F, precision):
    """Round 2: for fp32 plans the first pass of BatchNorm backward runs inside the dgrad epilogues (EPI_BNRED). The two backward
    schedules (r3m_resnet_set_fused_bn_reduce 1 / 0) must give the same parameter gradients — same sums, different summation
    order — on the same forward, incl. odd frame counts (partial 64-row groups), both dtypes (bf16 plans: the fused form is off by
    default, switched on here), train and eval BatchNorm; gates in the body."""
    from r3m_amd import R3M, _lib
    L = _lib.lib()
    m = R3M("cuda", 1e-4, 1024, size=size, langweight=0.0, tcnweight=1.0, precision=precision)
    _load_state(m.convnet)
    m = m.to(DEV)
    from oracle import detgen
    x = torch.from_numpy(detgen.frames("frames8", (8, 3, 224, 224)))[:F].to(DEV)
    for training in (True, False):
        m.train(training)
        res = {}
        for fused in (1, 0):
            m.encoder_opt.zero_grad()
            h = m(x)
            plan = m.convnet._plans[F]
            L.r3m_resnet_set_fused_bn_reduce(plan, fused)
            cw = torch.from_numpy(detgen.uniform("cw", tuple(h.shape), 0.5, 1.5)).to(DEV)
            (h * cw).sum().backward()
            res[fused] = {k: p.grad.detach().clone() for k, p in m.convnet.named_parameters()}
        L.r3m_resnet_set_fused_bn_reduce(m.convnet._plans[F], 1 if precision == "fp32" else 0)
        worst, worst_k, worst_l4 = 0.0, "", 0.0
        for k in res[0]:
            a, b = res[1][k].double(), res[0][k].double()
            e = float((a - b).norm() / b.norm().clamp_min(1e-30))
            if e > worst:
                worst, worst_k = e, k
            if k.startswith("layer4.") and e > worst_l4:
                worst_l4 = e
        report(f"r{size} {precision} F={F} {'train' if training else 'eval'}: fused vs stand-alone BN-backward reduce, worst tensor l2-rel "
               f"{worst:.3e} ({worst_k}), worst layer4 tensor {worst_l4:.3e}")
        if not training:
            # fixed statistics: c1 = c2 = 0, so the schedules differ ONLY in the BatchNorm parameter gradients' summation order —
            # every activation gradient, hence every conv weight gradient, is bit-identical
            assert all(torch.equal(res[1][k], res[0][k]) for k in res[0] if res[0][k].dim() == 4), "conv weight gradients must be identical"
            assert worst <= 1e-5, (worst, worst_k)
        else:
            # batch statistics: c1 / c2 differ in the last bits and that round-off is amplified through every BatchNorm backward
            # below (the reference's own fp32 gradients sit 5e-3 .. 2e-2 from float64 at conv1, tests above): tight where few
            # passes lie below (layer4), fp32-noise level everywhere else
            # measured: fp32 3e-6 .. 1.2e-5 on the worst tensor (bn1.bias), 7e-7 .. 1.3e-6 in layer4; bf16 (flipped roundings of
            # the stored gradients, chaotic on noise frames — tests/test_gpu_bf16.py) 2e-2 .. 7e-2 / 3e-3 .. 6e-3
            tol4 = 2e-5 if precision == "fp32" else 3e-2
            tol = 1e-4 if precision == "fp32" else 0.3
            assert worst_l4 <= tol4 and worst <= tol, (worst, worst_k, worst_l4)


@pytest.mark.parametrize("size,F,precision", [(18, 5, "fp32"), (34, 3, "bf16"), (50, 4, "fp32"), (50, 3, "bf16")])
def test_paired_bn_backward_is_bit_identical(hip, size, F, precision):
    """Round 5: the two BatchNorms that feed a downsample block's add + ReLU see the same masked gradient; their backward passes run
    as one launch each (second pass always; first pass too on bf16 plans). Same arithmetic per element and the same summation order
    as the separate passes: every parameter gradient must be BIT-identical with the switch on and off, train and eval."""
    from oracle import detgen
    from r3m_amd import R3M, _lib
    L = _lib.lib()
    m = R3M("cuda", 1e-4, 1024, size=size, langweight=0.0, tcnweight=1.0, precision=precision)
    _load_state(m.convnet)
    m = m.to(DEV)
    x = torch.from_numpy(detgen.frames("frames8", (8, 3, 224, 224)))[:F].to(DEV)
    for training in (True, False):
        m.train(training)
        res = {}
        for on in (1, 0):
            m.encoder_opt.zero_grad()
            h = m(x)
            assert L.r3m_resnet_set_bn_pair(m.convnet._plans[F], on) in (0, 1)
            cw = torch.from_numpy(detgen.uniform("cw", tuple(h.shape), 0.5, 1.5)).to(DEV)
            (h * cw).sum().backward()
            res[on] = {k: p.grad.detach().clone() for k, p in m.convnet.named_parameters()}
        L.r3m_resnet_set_bn_pair(m.convnet._plans[F], 1)
        bad = [k for k in res[0] if not torch.equal(res[0][k], res[1][k])]
        assert not bad, (training, bad[:5])


def test_second_forward_before_backward(hip):
    """The reference encoder is a plain autograd graph (models_r3m.py:84-100): h1 = enc(x1); h2 = enc(x2); backward through both
    works. Here a forward's activations live in a preallocated arena: with the default of one arena the FIRST forward's backward
    must refuse (never compute on overwritten activations); with R3M(..., max_live_forwards=2) both are alive and the joint
    backward equals the sum of the two separate ones (VERDICT r3 'one arena per module')."""
    from oracle import detgen
    from r3m_amd import R3M
    x = torch.from_numpy(detgen.frames("twofwd", (8, 3, 224, 224))).to(DEV)
    x1, x2 = x[:4].contiguous(), x[4:].contiguous()

    def build(k):
        m = R3M("cuda", 1e-4, 64, size=18, langweight=0.0, tcnweight=1.0, max_live_forwards=k).to(DEV)
        _load_state(m.convnet)
        m.convnet.eval()                                   # running statistics: the two forwards do not see each other
        return m

    m1 = build(1)
    h1 = m1.convnet(x1)
    h2 = m1.convnet(x2)
    with pytest.raises(RuntimeError, match="max_live_forwards"):
        h1.sum().backward()
    m1.encoder_opt.zero_grad()
    h2.sum().backward()                                    # the most recent forward is still intact
    g_b = m1.convnet.flat_grads().clone()
    m1.encoder_opt.zero_grad()
    h1 = m1.convnet(x1)
    (h1 * 0.5).sum().backward()
    g_a = m1.convnet.flat_grads().clone()

    m2 = build(2)
    m2.encoder_opt.zero_grad()
    h1 = m2.convnet(x1)
    h2 = m2.convnet(x2)
    ((h1 * 0.5).sum() + h2.sum()).backward()               # autograd runs the two encoder backwards in either order: both accumulate
    g = m2.convnet.flat_grads()
    ref = g_a + g_b
    err = float((g - ref).abs().max() / ref.abs().max())
    report(f"two live forwards: joint backward vs sum of separate backwards max-rel {err:.2e}")
    assert err < 2e-6
    # a third forward evicts the oldest of the ring of two
    h1 = m2.convnet(x1); h2 = m2.convnet(x2); h3 = m2.convnet(x1)
    with pytest.raises(RuntimeError, match="max_live_forwards"):
        h1.sum().backward()
    (h2.sum() + h3.sum()).backward()
    # a forward NOBODY differentiates (no_grad / inference call) between a training forward and its backward must not evict it
    # (ADVICE r4): it takes a free slot, or the scratch slot when every ring slot is live
    m1.encoder_opt.zero_grad()
    h1 = m1.convnet(x1)
    with torch.no_grad():
        e2 = m1.convnet(x2)
        e2b = m1.convnet(x2)
    assert m1.convnet._scratch is not None and m1.convnet._scratch.arena is not None
    (h1 * 0.5).sum().backward()
    assert torch.equal(m1.convnet.flat_grads(), g_a)
    assert torch.equal(e2, e2b)
    m1.convnet.release_scratch()
    assert m1.convnet._scratch.arena is None
    with torch.no_grad():                                  # nothing is live any more: the ring slot itself serves, no scratch arena
        e2c = m1.convnet(x2)
    assert m1.convnet._scratch.arena is None and torch.equal(e2, e2c)


def _kink_free_draw(golden_dir, size, draw, fused_bn_reduce=None):
    """One kink-free case (detgen.NOKINK_STATES[size][draw]): HIP gradients and the reference's own fp32 gradients against float64.
    Returns {tensor name: (hip l2-rel error, reference error)} for the seven named tensors + "rms" / "worst" over ALL tensors."""
    from oracle import detgen
    from r3m_amd import R3M
    tag, shift, frames = detgen.NOKINK_STATES[size][draw]
    g = np.load(os.path.join(golden_dir, f"encoder_r{size}_nokink{detgen.NOKINK_SUFFIX[draw]}.npz"))
    assert float(g["min_abs_z"]) > 1e-3
    m = R3M("cuda", 1e-4, 1024, size=size, langweight=0.0, tcnweight=1.0).to(DEV)
    shapes = [(k, tuple(v.shape)) for k, v in m.convnet.state_dict().items()]
    sd = detgen.resnet_state_dict_no_kink(shapes, size, tag=tag, shift=shift)
    m.convnet.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m.train()
    x = torch.from_numpy(detgen.frames(frames, (8, 3, 224, 224))).to(DEV)
    h = m(x)
    e = rel_err(h.detach().cpu().numpy(), g["h_train"])[0]
    e64 = rel_err(h.detach().cpu().numpy(), g["h_train_fp64"])[0]
    report(f"r{size} kink-free draw {draw} ({tag}, {frames}): train-mode embedding max-rel vs reference fp32 {e:.2e}, vs float64 {e64:.2e}")
    assert e < 1e-4
    cw = torch.from_numpy(detgen.uniform("cw", tuple(h.shape), 0.5, 1.5)).to(DEV)
    (h * cw).sum().backward()
    P = dict(m.convnet.named_parameters())
    worst_hip = worst_cpu = 0.0
    sq_hip = sq_cpu = 0.0
    worst_name = ""
    for name, n32, n64 in zip(g["grad_names"], g["grad_norms"], g["grad_norms_fp64"]):
        got = float(P[str(name)].grad.double().norm())
        e_hip, e_cpu = abs(got - n64) / max(n64, 1e-12), abs(n32 - n64) / max(n64, 1e-12)
        if e_hip > worst_hip:
            worst_hip, worst_name = e_hip, str(name)
        worst_cpu = max(worst_cpu, e_cpu)
        sq_hip += e_hip * e_hip
        sq_cpu += e_cpu * e_cpu
    n_t = len(g["grad_names"])
    out = {"rms": ((sq_hip / n_t) ** 0.5, (sq_cpu / n_t) ** 0.5), "worst": (worst_hip, worst_cpu)}
    report(f"r{size} kink-free draw {draw}: grad-norm rel vs fp64 over {n_t} tensors: worst hip {worst_hip:.3e} ({worst_name}) reference-cpu-fp32 "
           f"{worst_cpu:.3e}; rms hip {out['rms'][0]:.3e} reference-cpu-fp32 {out['rms'][1]:.3e} ratio {out['rms'][0] / max(out['rms'][1], 1e-12):.2f}")
    lb = _last_bn(size)
    for k in ("conv1.weight", "bn1.weight", "bn1.bias", lb + ".weight", lb + ".bias", "layer1.0.conv1.weight", "layer2.0.downsample.0.weight"):
        hip_err = rel_err(P[k].grad.cpu().numpy(), g["grad64_" + k])[1]
        cpu_err = rel_err(g["grad_" + k], g["grad64_" + k])[1]
        out[k] = (hip_err, cpu_err)
        report(f"r{size} kink-free draw {draw} grad {k}: l2-rel vs fp64: hip {hip_err:.3e}  reference-cpu-fp32 {cpu_err:.3e}  ratio {hip_err / max(cpu_err, 1e-12):.2f}")
    return out


@pytest.mark.parametrize("size", [18, 34, 50])
def test_encoder_gradients_kink_free_case(hip, golden_dir, size):
    """G8 (made statistical in round 5 — VERDICT r4 item 3): the gradient gate with NO escape hatch. On a kink-free
    state (detgen.resnet_state_dict_no_kink: no float64 pre-activation of the last block within 1e-3 of zero) every fp32 forward
    makes the float64 ReLU decisions of the last block, so the HIP gradients are gated against float64 relative to the error of the
    reference's own PyTorch-CPU fp32 gradients of the same tensor — unconditionally: no flip table, no re-evaluation of the oracle.
    ONE golden state is one draw of fp32 round-off on each side (round 4's ResNet-18 draw read 2.2-2.9 against a 3.0 gate), so the
    gate runs over THREE independent (weights, frames) draws per size (detgen.NOKINK_STATES): the MEDIAN ratio hip / reference must be
    <= 2 and every single draw <= 4 (an error below 1e-4 always passes), for the seven named tensors and for the rms over all
    parameter tensors; the single worst tensor of a draw stays within 4x the reference's own worst."""
    draws = [_kink_free_draw(golden_dir, size, d) for d in range(3)]
    fails = []
    for k in draws[0]:
        if k == "worst":
            continue
        ratios = []
        for d in draws:
            hip_err, cpu_err = d[k]
            ratios.append(0.0 if hip_err <= 1e-4 else hip_err / max(cpu_err, 1e-12))
        med = sorted(ratios)[1]
        report(f"r{size} kink-free {k}: hip / reference error ratios over the three draws {', '.join(f'{r:.2f}' for r in ratios)}  median {med:.2f}")
        if med > 2.0 or max(ratios) > 4.0:
            fails.append((k, ratios))
    for i, d in enumerate(draws):
        # the single worst tensor = the maximum of 60-159 strongly correlated draws (one perturbation reaches every tensor below it)
        if d["worst"][0] > max(4.0 * d["worst"][1], 1e-4):
            fails.append(("worst", i, d["worst"]))
    assert not fails, fails


# ---- round 6: the inference path (r3m_resnet_forward with training = 2) ------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [18, 34, 50])
def test_inference_forward_fused_vs_unfused(hip, size, precision):
    """`load_r3m(...).eval()` under torch.no_grad() (/root/reference/r3m/__init__.py:72-75, r3m/example.py:19-33) runs the inference
    sequence: eval-mode BatchNorm, the residual join and the ReLU are applied where each convolution stores its result
    (EPI_AFFINE | EPI_ACCUM | EPI_RELU), no stand-alone BatchNorm pass runs. Against the unfused eval sequence (conv, then bn_act_fwd;
    r3m_debug_set_fused_inference(0)) on the same weights and frames:
      fp32: BIT-IDENTICAL embeddings (the fused store computes the same fmaf(y, scale, shift) [+ residual] and max(., 0) on the same
            fp32 values), for a frame count that fills whole tiles and for a ragged one;
      bf16: the fused store rounds ONCE (the conv result is never stored) where the unfused pair rounds twice — embeddings agree to
            1e-2 l2-rel and the fused one is at least as close to the float64 emulation-free truth of the same bf16-rounded weights.
    A grad-enabled eval forward keeps the saved-state sequence (training = 0): its backward still works and matches."""
    from r3m_amd import R3M
    torch.manual_seed(5)
    m = R3M("cuda", 1e-4, 1024, size=size, langweight=0.0, tcnweight=1.0, precision=precision)
    _load_state(m.convnet)
    m = m.to(DEV).eval()
    for F in (8, 5):
        x = torch.randint(0, 256, (F, 3, 224, 224), device=DEV).float()
        with torch.no_grad():
            old = hip.r3m_debug_set_fused_inference(1)
            try:
                h_f = m(x)
                hip.r3m_debug_set_fused_inference(0)
                h_u = m(x)
            finally:
                hip.r3m_debug_set_fused_inference(old)
        assert torch.isfinite(h_f).all()
        if precision == "fp32":
            assert torch.equal(h_f, h_u), float((h_f - h_u).abs().max())
        else:
            d = float((h_f - h_u).norm() / h_u.norm())
            report(f"r{size} bf16 inference, {F} frames: fused vs unfused eval embedding l2-rel {d:.3e}")
            assert d < 1e-2
    # the saved-state eval forward (grad enabled) is unchanged and differentiable; an inference forward is not
    x = torch.randint(0, 256, (4, 3, 224, 224), device=DEV).float()
    h = m(x)
    with torch.no_grad():
        h_inf = m(x)
    if precision == "fp32":
        assert torch.equal(h.detach(), h_inf)
    h.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in m.convnet.parameters())


def test_inference_forward_keeps_nothing_for_a_backward(hip):
    """C ABI contract: r3m_resnet_backward after a training = 2 forward is an error (the activations were overwritten in place)."""
    from r3m_amd import R3M
    m = R3M("cuda", 1e-4, 1024, size=18, langweight=0.0, tcnweight=1.0).to(DEV).eval()
    x = torch.randint(0, 256, (2, 3, 224, 224), device=DEV).float()
    with torch.no_grad():
        m(x)
    conv = m.convnet
    slot = conv._ring[0]             # no forward is live: the ring's first slot took this one (_pick_slot)
    plan = slot.plans[2]
    dh = torch.ones((2, conv.outdim), device=DEV)
    g = conv.flat_grads()
    rc = hip.r3m_resnet_backward(plan, dh.data_ptr(), conv.flat_params().data_ptr(), g.data_ptr(), slot.arena.data_ptr(), 0, 4, 0,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"inference mode" in hip.r3m_last_error()
