"""not gpu: what the objective and the batched reward head answer about num_negatives = N on the host -- workspace sizes and every
refusal, each of which returns before any HIP call (include/r3m_hip.h), so the pointers below are dummies and no GPU is needed. The
Python layers (ops.r3m_loss, LanguageReward.batched_scores, R3M, Trainer.update) refuse a wrong row count / a bad N before they touch
a device, too."""
import ctypes
import types

import pytest
import torch

SHAPES = [(1, 32), (5, 2048), (256, 512), (257, 8)]          # (B, D)
HID, LD = 64, 768


@pytest.fixture(scope="module")
def L():
    from r3m_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_int * 64)()
    p.keep = buf
    return ctypes.addressof(buf)


def err(L):
    return L.r3m_last_error().decode()


def test_workspace_sizes_at_three_are_the_old_ones_and_grow_with_n(L):
    for B, D in SHAPES:
        assert L.r3m_loss_workspace_bytes_n(B, 3) == L.r3m_loss_workspace_bytes(B) > 0
        assert L.r3m_langrew_workspace_bytes_n(B, 512, HID, LD, 3) == L.r3m_langrew_workspace_bytes(B, 512, HID, LD) > 0
        loss = [L.r3m_loss_workspace_bytes_n(B, N) for N in range(17)]
        head = [L.r3m_langrew_workspace_bytes_n(B, 512, HID, LD, N) for N in range(17)]
        assert all(b > a > 0 for a, b in zip(loss, loss[1:])), loss
        assert all(b > a > 0 for a, b in zip(head, head[1:])), head
        # 3 + 2N pairs of 4 statistics and 1 coefficient per clip
        assert loss[4] - loss[3] == B * 2 * 5 * 4


@pytest.mark.parametrize("N", [-1, 17])
def test_n_outside_the_range_is_refused_with_the_number(L, p, N):
    B, D = 5, 64
    assert L.r3m_loss_workspace_bytes_n(B, N) == 0 and f"num_negatives={N}" in err(L) and "0..16" in err(L)
    assert L.r3m_langrew_workspace_bytes_n(B, D, HID, LD, N) == 0 and f"num_negatives={N}" in err(L) and "0..16" in err(L)
    big = 1 << 30
    rc = L.r3m_loss_tcn_lp_n(p, p, p, p, p, big, B, D, N, 1, 1e-5, 1e-5, 1.0, None)
    assert rc != 0 and "loss_tcn_lp" in err(L) and f"num_negatives={N}" in err(L)
    rc = L.r3m_loss_lang_infonce_n(p, p, p, p, big, B, N, 1.0, None)
    assert rc != 0 and "loss_lang_infonce" in err(L) and f"num_negatives={N}" in err(L)
    for dt in (0, 1):
        rc = L.r3m_langrew_forward_n(p, p, p, p, p, p, big, B, D, HID, LD, N, dt, None)
        assert rc != 0 and "langrew_forward" in err(L) and f"num_negatives={N}" in err(L)
        rc = L.r3m_langrew_backward_n(p, p, p, p, p, p, big, B, D, HID, LD, N, 0, dt, None)
        assert rc != 0 and "langrew_backward" in err(L) and f"num_negatives={N}" in err(L)


def test_zero_negatives_with_the_time_contrastive_loss_names_the_reference_line(L, p):
    big = 1 << 30
    rc = L.r3m_loss_tcn_lp_n(p, p, p, p, p, big, 5, 64, 0, 1, 1e-5, 1e-5, 0.5, None)
    assert rc != 0 and "num_negatives=0" in err(L) and "trainer.py:140" in err(L) and "torch.stack" in err(L)
    # the sizes themselves exist: N = 0 is the language loss with its in-clip negative, or the LP terms alone
    assert L.r3m_loss_workspace_bytes_n(5, 0) > 0 and L.r3m_langrew_workspace_bytes_n(5, 64, HID, LD, 0) > 0


@pytest.mark.parametrize("N", [0, 1, 3, 16])
def test_a_workspace_one_byte_short_is_refused(L, p, N):
    B, D = 5, 64
    need = L.r3m_loss_workspace_bytes_n(B, N)
    tcnw = 1.0 if N else 0.0
    rc = L.r3m_loss_tcn_lp_n(p, p, p, p, p, need - 1, B, D, N, 1, 1e-5, 1e-5, tcnw, None)
    assert rc != 0 and "workspace too small" in err(L) and str(need) in err(L) and f"{N} negatives" in err(L)
    rc = L.r3m_loss_lang_infonce_n(p, p, p, p, need - 1, B, N, 1.0, None)
    assert rc != 0 and "workspace too small" in err(L) and str(need) in err(L)
    need = L.r3m_langrew_workspace_bytes_n(B, D, HID, LD, N)
    rc = L.r3m_langrew_forward_n(p, p, p, p, p, p, need - 1, B, D, HID, LD, N, 0, None)
    assert rc != 0 and "langrew_forward: workspace too small" in err(L) and str(need) in err(L)
    rc = L.r3m_langrew_backward_n(p, p, p, p, p, p, need - 1, B, D, HID, LD, N, 0, 1, None)
    assert rc != 0 and "langrew_backward: workspace too small" in err(L) and str(need) in err(L)
    # the old entry points are the N = 3 calls: a workspace sized for fewer negatives is too small for them
    if N < 3:
        small = L.r3m_loss_workspace_bytes_n(B, N)
        assert L.r3m_loss_tcn_lp(p, p, p, p, p, small, B, D, 1, 1e-5, 1e-5, 1.0, None) != 0 and "workspace too small" in err(L)
    # r3m_loss_finalize reads the per-clip partials that lead the workspace (12 floats per clip): one byte less is refused, and
    # every N's workspace holds them
    assert L.r3m_loss_finalize(p, 48 * B - 1, B, 0, p, 1e-5, 1e-5, 1.0, 0.0, None) != 0
    assert "loss_finalize: workspace too small" in err(L) and str(48 * B) in err(L)
    assert L.r3m_loss_workspace_bytes_n(B, 0) >= 48 * B


def test_a_row_count_past_32_bits_is_refused(L, p):
    B = (1 << 31) // 54 + 1
    assert L.r3m_langrew_workspace_bytes_n(B, 64, HID, LD, 16) == 0 and "2^31" in err(L)
    assert L.r3m_langrew_forward_n(p, p, p, p, p, p, 1 << 40, B, 64, HID, LD, 16, 0, None) != 0 and "2^31" in err(L)


def test_ops_r3m_loss_checks_the_row_counts_before_any_launch():
    from r3m_amd import ops
    B, D = 4, 32
    alle = torch.zeros(B, 5, D)                                  # CPU tensors: a check that came after the device check would not be reached
    perm = torch.arange(B, dtype=torch.int32).repeat(6, 1)
    with pytest.raises(ValueError, match=r"perm \(6, 4\) must be \[2 \* num_negatives, B\] = \[4, 4\]"):
        ops.r3m_loss(alle, perm, 1e-5, 1e-5, 1.0, num_negatives=2)
    with pytest.raises(ValueError, match=r"scores \(15, 4\) must be \[6 \+ 3 \* num_negatives, B\] = \[21, 4\]"):
        ops.r3m_loss(alle, None, 1e-5, 1e-5, 1.0, scores=torch.zeros(15, B), mask=torch.ones(B), langweight=1.0, num_negatives=5)
    with pytest.raises(ValueError, match="num_negatives=17"):
        ops.r3m_loss(alle, None, 1e-5, 1e-5, 1.0, num_negatives=17)
    with pytest.raises(ValueError, match=r"num_negatives=0 with tcnweight > 0.*trainer\.py:140"):
        ops.r3m_loss(alle, None, 1e-5, 1e-5, 1.0, num_negatives=0)
    # right row counts pass the checks and reach the device check (no CPU fallback)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.r3m_loss(alle, perm[:4], 1e-5, 1e-5, 1.0, num_negatives=2)


def test_batched_scores_checks_the_permutation_rows_before_any_launch():
    from r3m_amd.models_language import LanguageReward
    rew = LanguageReward(None, 32, 64, 32)
    alle, feats = torch.zeros(4, 5, 32), torch.zeros(4, 32)
    with pytest.raises(ValueError, match="has 10 rows"):
        rew.batched_scores(alle, feats, torch.zeros(10, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="has 51 rows"):
        rew.batched_scores(alle, feats, torch.zeros(51, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"must be \[3 \* num_negatives, B\]"):
        rew.batched_scores(alle, feats, torch.zeros(9, 5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rew.batched_scores(alle, feats, torch.zeros(6, 4, dtype=torch.int32))


def test_model_and_trainer_validate_num_negatives():
    from r3m_amd import R3M
    from r3m_amd.trainer import Trainer
    import numpy as np
    from r3m_amd.ops import check_num_negatives
    assert check_num_negatives(np.int64(5)) == 5 and check_num_negatives(torch.tensor(2)) == 2 and type(check_num_negatives(np.int32(1))) is int
    for bad in (-1, 17, 2.0, True, np.float32(3), "3", None):
        with pytest.raises(ValueError, match="num_negatives"):
            R3M("cuda", 1e-4, 64, size=18, langweight=0.0, tcnweight=1.0, num_negatives=bad)
    with pytest.raises(ValueError, match=r"trainer\.py:140"):
        R3M("cuda", 1e-4, 64, size=18, langweight=0.0, tcnweight=1.0, num_negatives=0)
    # the attribute is writable after construction, as on the reference: Trainer.update checks it before the encoder runs
    class Wrapped(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the encoder ran")
    for n, tcnw, what in ((17, 1.0, "num_negatives=17"), (0, 1.0, r"trainer\.py:140"), (-2, 0.0, "num_negatives=-2")):
        model = Wrapped()
        model.module = types.SimpleNamespace(num_negatives=n, tcnweight=tcnw, langweight=0.0, l2weight=1e-5, l1weight=1e-5, l2dist=True)
        with pytest.raises(ValueError, match=what):
            Trainer(1).update(model, (torch.zeros(2, 5, 3, 224, 224), [""] * 2), 0)
