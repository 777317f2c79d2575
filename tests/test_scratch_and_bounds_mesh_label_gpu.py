"""The labelled surface meshing (label_meshes, branch_meshes) over dirty scratch memory, with red zones around every buffer
(tests/guarded_alloc.py), as tests/test_scratch_and_bounds_mesh_gpu.py runs the plain meshing: three runs -- workspaces and
outputs pre-filled with 0x00, 0xFF and seeded random bytes, the input copied into a red-zoned buffer -- must leave every red zone
as it was, give the same bits, and equal the numpy oracle (tests/mesh_label_oracle.py), never another run of the code under
test.  The shapes cross a 64-voxel word, fill many sort blocks and need both radix digits."""
import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import mesh_label_oracle as lo

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
SHAPES = {(5, 6, 67): (3, 0.5), (24, 20, 70): (300, 0.7)}
CENTRE, SPACING = (2.5, 3.0, 31.25), (0.7, 0.8, 1.25)
_WANT = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def want(shape):
    """The volume, the oracle's meshes of it and its branch models after two sweeps, computed once."""
    if shape not in _WANT:
        L = lo.random_labels(shape, SHAPES[shape][0], SHAPES[shape][1], sum(shape))
        L[1, 2, 63], L[1, 2, 64] = 1, 2
        _WANT[shape] = (L, lo.label_meshes(L), lo.branch_meshes(L, SPACING, CENTRE, n_iter=2))
    return _WANT[shape]


def dev(a):
    return guard(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(got, res):
    assert np.array_equal(got.vert_ptr, res[2]) and np.array_equal(got.face_ptr, res[3])
    assert np.array_equal(got.faces.cpu().numpy(), res[1])
    assert np.array_equal(bits(got.verts.cpu().numpy()), bits(res[0]))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_label_meshes(A, shape):
    L, res, _ = want(shape)
    got = three_fills(lambda: A.label_meshes(dev(L)), "mesh label extraction")
    same(got, res)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_branch_meshes(A, shape):
    L, _, res = want(shape)
    got = three_fills(lambda: A.branch_meshes(dev(L), SPACING, CENTRE, n_iter=2), "mesh label branches")
    same(got, res)


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
