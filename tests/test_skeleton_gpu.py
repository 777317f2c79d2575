"""GPU skeletonisation (csrc/skeleton.hip through prep.skeletonize_3d) against tests/skeleton_oracle.py, the plain-Python
statement of DESIGN.md section 3d: bitwise on the eight pinned volumes (and their digests), pass counts, input forms, and
the chain into the consumers of a skeleton."""
import numpy as np
import pytest
import torch

import skeleton_oracle as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", so.CASES)
def test_equals_the_oracle_bitwise(A, name):
    v, want, passes = so.solved(name)
    t = dev(v)
    before = t.clone()
    got, got_passes = A.skeletonize_3d(t, return_passes=True)
    assert got.dtype == torch.uint8 and got.device == t.device and tuple(got.shape) == v.shape
    assert torch.equal(t, before)                                            # the input is not modified
    g = got.cpu().numpy()
    assert np.array_equal(g, want), f"{int((g != want).sum())} voxels differ"
    assert so.digest(g) == so.EXPECTED[name][2]
    assert got_passes == passes
    assert torch.equal(A.skeletonize_3d(t), got)                             # a second call gives identical bits


def test_word_aligned_rows_and_carries(A):
    """A last axis of exactly two words with a full last word, on a dense random volume: it exercises two-word rows.  It does
    NOT pin the carry at k = 63/64 of the re-check: the oracle with that carry dropped gives the same bits on this volume
    (test_skeleton_host.py::test_the_dense_two_word_volume_does_not_see_the_carry).  The `plate` and `plate_noise` cases of
    test_skeleton_rounds_gpu.py pin it."""
    v = (np.random.default_rng(7).random((5, 6, 128)) < 0.7).astype(np.uint8)
    want, passes = so.skeletonize(v)
    got, got_passes = A.skeletonize_3d(dev(v), return_passes=True)
    assert np.array_equal(got.cpu().numpy(), want) and got_passes == passes


def test_long_chains_across_rows(A):
    """A thin slab: the candidates of its 72-row face each wait for the row before, which takes more re-check rounds than
    run as launches of their own, so the single-workgroup loop finishes the sub-iteration."""
    v = np.ones((2, 72, 40), dtype=np.uint8)
    want, passes = so.skeletonize(v)
    got, got_passes = A.skeletonize_3d(dev(v), return_passes=True)
    assert np.array_equal(got.cpu().numpy(), want) and got_passes == passes


def test_input_forms_agree(A):
    v, want, _ = so.solved("tree")
    ref = A.skeletonize_3d(dev(v))
    as_numpy = A.skeletonize_3d(v.astype(np.int32) * 7)                      # any dtype, non-zero = foreground
    assert isinstance(as_numpy, np.ndarray) and as_numpy.dtype == np.uint8 and np.array_equal(as_numpy, want)
    assert torch.equal(A.skeletonize_3d(dev(v).bool()), ref)
    view = dev(np.ascontiguousarray(v.transpose(2, 0, 1))).permute(1, 2, 0)  # same values, not contiguous
    assert not view.is_contiguous()
    assert torch.equal(A.skeletonize_3d(view), ref)


def test_feeds_the_consumers_of_a_skeleton(A):
    v, want, _ = so.solved("tree")
    label = dev(v)
    pred = label.clone()
    pred[:, :, 100:] = 0
    skeleton = A.skeletonize_3d(label)
    loc_skeleton, loc_small = A.hard_mining_candidates(label, skeleton, pred)
    missed = want.astype(bool) & (pred.cpu().numpy() != 1)
    assert len(loc_skeleton) == int(missed.sum()) > 0 and len(loc_small) > 0
    w_br, br_skel = A.break_weight(label, pred, skeleton)
    assert w_br.shape == label.shape and br_skel.shape == label.shape
    assert A.postprocess.tree_length_calculation(label, skeleton) == 100.0


def test_argument_errors(A):
    with pytest.raises(ValueError):
        A.skeletonize_3d(torch.zeros((4, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        A.skeletonize_3d(np.zeros((4, 4)))
    with pytest.raises(RuntimeError):
        A.skeletonize_3d(torch.zeros((4, 4, 4), dtype=torch.uint8))
