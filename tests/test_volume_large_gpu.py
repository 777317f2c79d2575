"""``marching_cubes``, ``mesh_adjacency``, ``smooth_mesh``, ``label_meshes``, ``surface_distances`` and ``surface_metrics`` at the
sizes where the exclusive scan they number their outputs with (``run_scan`` / ``scan_add``, csrc/bitvol.hip)
leaves the first chunk of its top level: more than 2^20 packed words, vertices or histogram bins.  Every production-size volume
goes through that loop; the small tests stop at a few thousand elements.

The cases, their oracle results (one run per process) and what each reaches are in tests/volume_large_cases.py;
tests/test_volume_large_host.py proves on the CPU that each reaches it.  Every comparison is bit for bit against the numpy
oracles (tests/mesh_oracle.py, tests/mesh_label_oracle.py, tests/surface_oracle.py, and scipy's transform for the distances),
except the three surface means, which keep ``surface_oracle.mean_bound``.  Every test calls its operation twice and compares
the bytes.  The default stream only."""
import numpy as np
import pytest
import torch

import volume_large_cases as vc
from test_mesh_gpu import same
from test_mesh_label_gpu import same as same_labels
from test_surface_gpu import TOLERANCES, check_metrics
from test_surface_host import bits

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


def same_bytes(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. extraction ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.MESH_CASES)
def test_extraction_equals_the_oracle(A, name):
    v, verts, faces = vc.mesh(name)
    t = dev(v)
    got_v, got_f = A.marching_cubes(t, vc.LEVEL)
    print(name, "V", len(verts), "F", len(faces), "got", tuple(got_v.shape), tuple(got_f.shape))
    same(got_v, verts)
    same(got_f, faces)
    again_v, again_f = A.marching_cubes(t, vc.LEVEL)
    same_bytes(again_v, got_v)
    same_bytes(again_f, got_f)


# ---- 2. adjacency and one smoothing sweep -------------------------------------------------------------------------------------------
def test_adjacency_equals_the_oracle(A):
    _, verts, faces = vc.mesh("one_more")
    indptr, indices, boundary = vc.adjacency()
    f = dev(faces)
    got = A.mesh_adjacency(f, len(verts))
    same(got[0], indptr)
    same(got[1], indices)
    same(got[2], boundary)
    again = A.mesh_adjacency(f, len(verts))
    for g, a in zip(got, again):
        same_bytes(a, g)


def test_one_smoothing_sweep_equals_the_oracle(A):
    _, verts, faces = vc.mesh("one_more")
    v, f = dev(verts), dev(faces)
    got = A.smooth_mesh(v, f, n_iter=1, relaxation_factor=0.2)
    same(got, vc.smoothed())
    same_bytes(A.smooth_mesh(v, f, n_iter=1, relaxation_factor=0.2), got)
    same(v, verts)                                                           # the input is left alone


# ---- 3. labelled meshes -------------------------------------------------------------------------------------------------------------
def twice_same_labels(A, L, res, num):
    t = dev(L)
    got = A.label_meshes(t, num=num)
    same_labels(got, res)
    again = A.label_meshes(t, num=num)
    same_bytes(again.verts, got.verts)
    same_bytes(again.faces, got.faces)
    assert np.array_equal(again.vert_ptr, got.vert_ptr) and np.array_equal(again.face_ptr, got.face_ptr)
    return got


def test_label_meshes_equal_the_oracle(A):
    """The labels 1 and 300: the word scan has two chunks, both sorts run two passes over more than 2^22 items."""
    L, res = vc.labels()
    got = twice_same_labels(A, L, res, vc.LABEL_NUM)
    assert got.num == vc.LABEL_NUM and (len(res[0]), len(res[1])) == (5187422, 6436289)
    same_labels(A.label_meshes(dev(L)), res)                                  # the largest label found on the device


@pytest.mark.parametrize("which", list(vc.LABEL_TOPS))
def test_label_sorts_with_items_on_both_sides_of_the_chunk_border(A, which):
    """The same voxels with the larger label renamed so that its radix digit is 255: the histogram scan of every pass has items
    in its second chunk (tests/volume_large_cases.py says why 300 has none)."""
    L, res = vc.labels_renamed(which)
    twice_same_labels(A, L, res, vc.LABEL_TOPS[which])


def test_label_meshes_of_the_first_label_alone(A):
    """``num=1``: the one-pass sort over the same words.  A label above ``num`` is refused, not dropped, so the larger label is
    cleared for the call that is compared; the refusal is pinned beside it."""
    L, _ = vc.labels()
    with pytest.raises(ValueError, match="above num = 1"):
        A.label_meshes(dev(L), num=1)
    L1, res = vc.labels_first_only()
    twice_same_labels(A, L1, res, 1)


# ---- 4. surface distances and metrics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.SURFACE_CASES)
def test_distances_counts_and_voxels_equal_the_oracle(A, name):
    a, b, spacing, D, n_a, n_b, voxels = vc.surface(name)
    ta, tb = dev(a), dev(b)
    got, ga, gb, gv = A.surface_distances(ta, tb, spacing, return_voxels=True)
    print(name, "n_a", n_a, "n_b", n_b, "got", ga, gb)
    assert (ga, gb) == (n_a, n_b)
    assert got.dtype == torch.float64 and gv.dtype == torch.int32
    assert np.array_equal(gv.cpu().numpy(), voxels)
    again = A.surface_distances(ta, tb, spacing)
    assert len(again) == 3 and again[1:] == (n_a, n_b)
    same_bytes(again[0], got)
    if D is None:
        pytest.skip("scipy is not installed: counts and voxel indices compared, the distances are not")
    assert np.array_equal(bits(got.cpu().numpy()), bits(D))
    if name == "one_more":
        assert (n_a, n_b, np.unique(D[:n_a]).size) == (1049416, 1048858, 8)    # a massive tie for the radix select


@pytest.mark.parametrize("name", vc.SURFACE_CASES)
def test_metrics_equal_the_oracle(A, name):
    a, b, spacing, D, n_a, n_b, _ = vc.surface(name)
    ta, tb = dev(a), dev(b)
    got = A.surface_metrics(ta, tb, spacing, tolerances=TOLERANCES)
    again = A.surface_metrics(ta, tb, spacing, tolerances=TOLERANCES)
    assert (got.n_a, got.n_b) == (n_a, n_b)
    assert again == got and bits(again.assd) == bits(got.assd) and bits(again.asd_ab) == bits(got.asd_ab)     # the same bits
    if D is None:
        pytest.skip("scipy is not installed: the counts compared, the metrics are not")
    check_metrics(got, vc.metrics(name, TOLERANCES), D, n_a, n_b)
