"""The clDice definition (tests/cldice_oracle.py) on the CPU: its explicit statement (b) against the autograd statement (a), its
behaviour on tied inputs, the hard score on hand-made cases, and what the package refuses.  No GPU."""
import numpy as np
import pytest
import torch

import cldice_oracle as O

SHAPES = O.PARITY_SHAPES + O.DEGENERATE_SHAPES


@pytest.mark.parametrize("iters", O.ITERS)
@pytest.mark.parametrize("shape", SHAPES)
def test_explicit_statement_matches_autograd(shape, iters):
    p, t = O.case(shape)
    ref = O.reference(shape, iters)                      # (asserts that the case is worth testing)
    lb, gb, sb = O.loss_and_grad_b(p, t, iters, 1.0, torch.float64)
    assert abs(float(lb) - float(ref["l64"])) <= 1e-12
    assert float((gb - ref["g64"]).abs().max()) <= 1e-12
    assert float((sb - ref["s64"]).abs().max()) <= 1e-12 * max(1.0, float(ref["s64"].abs().max()))
    fa, fb = O.soft_skeleton_a(p, iters), O.soft_skeleton_b(p, iters)
    assert fa.dtype == fb.dtype == torch.float32
    assert torch.equal(fa.view(torch.int32), fb.view(torch.int32))


def test_every_leading_index_is_a_volume_of_its_own():
    p, _ = O.case((2, 7, 9, 11))
    whole = O.soft_skeleton_b(p, 3)
    for v in range(2):
        assert torch.equal(whole[v:v + 1], O.soft_skeleton_b(p[v:v + 1], 3))
        assert torch.equal(whole[v:v + 1], O.soft_skeleton_a(p[v:v + 1], 3))


@pytest.mark.parametrize("shape", O.PARITY_SHAPES[:2])
def test_tied_inputs_are_deterministic_and_finite(shape):
    binary, rounded, t = O.tied_inputs(shape)
    for p in (binary, rounded):
        assert torch.unique(p).numel() <= 11
        one = O.loss_and_grad_b(p, t, 3)
        two = O.loss_and_grad_b(p.clone(), t.clone(), 3)
        for a, b in zip(one, two):
            assert torch.isfinite(a).all() and torch.equal(a, b)
        assert float(one[1].abs().max()) > 0


def test_hard_score_on_hand_made_cases():
    label, skel, leak, leak_skel = O.tube_case()
    assert O.cldice_score(label, label, skel, skel) == (1.0, 1.0, 1.0)
    other, other_skel = np.zeros_like(label), np.zeros_like(skel)
    other[6:9, 6:9, 2:18] = 1
    other_skel[7, 7, 3:17] = 1
    assert not (other & label).any()
    assert O.cldice_score(other, label, other_skel, skel) == (0.0, 0.0, 0.0)
    score, tprec, tsens = O.cldice_score(leak, label, leak_skel, skel)
    assert tsens == 1.0 and tprec == 15 / 18 and score == 2 * tprec / (tprec + 1)
    assert O.cldice_counts(leak, label, leak_skel, skel) == (15, 18, 14, 14)


def test_hard_score_of_empty_skeletons_is_zero():
    label, skel = O.tube_case()[:2]
    empty = np.zeros_like(label)
    assert O.cldice_score(empty, label, empty, skel) == (0.0, 0.0, 0.0)
    assert O.cldice_score(label, empty, skel, empty) == (0.0, 0.0, 0.0)
    assert O.cldice_score(empty, empty, empty, empty) == (0.0, 0.0, 0.0)


def test_refusals():
    import seunet_amd as A
    p, t = O.case((2, 7, 9, 11))
    for bad in (-1, 17, 2.0, True):
        with pytest.raises(ValueError, match="must be an integer from 0 to 16"):
            A.soft_skeleton(p, iters=bad)
        with pytest.raises(ValueError, match="must be an integer from 0 to 16"):
            A.soft_cldice_loss(p, t, iters=bad)
    with pytest.raises(ValueError, match="the last three axes are the volume"):
        A.soft_skeleton(p[0, 0])
    with pytest.raises(ValueError, match="none may be empty"):
        A.soft_skeleton(p[:, :0])
    with pytest.raises(ValueError, match=r"target of shape \(1, 7, 9, 11\) for a prediction of shape \(2, 7, 9, 11\)"):
        A.soft_cldice_loss(p, t[:1])
    with pytest.raises(ValueError, match="target_skeleton of shape"):
        A.soft_cldice_loss(p, t, target_skeleton=t[:1])
    with pytest.raises(RuntimeError, match="soft_skeleton needs GPU tensors"):
        A.soft_skeleton(p)
    with pytest.raises(RuntimeError, match="soft_cldice_loss needs GPU tensors"):
        A.soft_cldice_loss(p, t)
    with pytest.raises(RuntimeError, match="cldice_score: needs a CUDA tensor"):
        A.cldice_score(torch.zeros(3, 3, 3), torch.zeros(3, 3, 3))
    lib = A._lib.load()
    assert lib.seunet_cldice_workspace_bytes(1, 4, 4, 4, 17, 0) == 0 and "iters=17" in A._lib.last_error()
    assert lib.seunet_cldice_workspace_bytes(1, 0, 4, 4, 3, 0) == 0 and "empty shape" in A._lib.last_error()
    assert lib.seunet_cldice_workspace_bytes(0, 4, 4, 4, 3, 0) == 0 and "empty shape" in A._lib.last_error()
    assert 0 < lib.seunet_cldice_workspace_bytes(2, 7, 9, 11, 3, 0) < lib.seunet_cldice_workspace_bytes(2, 7, 9, 11, 3, 1)


@pytest.mark.parametrize("iters", (0, 3, 16))
def test_workspace_layout(iters):
    """two E buffers; with save the d chain (iters + 1 volumes), the S chain (iters), the a chain (iters + 1) and one choice byte
    per voxel and iteration -- each sub-buffer rounded up to 256 bytes"""
    import seunet_amd as A
    lib = A._lib.load()

    def up(v):
        return (v + 255) // 256 * 256
    n = 2 * 7 * 9 * 11
    assert lib.seunet_cldice_workspace_bytes(2, 7, 9, 11, iters, 0) == 2 * up(4 * n)
    assert lib.seunet_cldice_workspace_bytes(2, 7, 9, 11, iters, 1) == \
        2 * up(4 * n) + 2 * up(4 * n * (iters + 1)) + up(4 * n * iters) + up(n * (iters + 1))
