"""The surface-meshing wrappers (extraction, adjacency, smoothing, STL records) over dirty scratch memory, with red zones around
every buffer (tests/guarded_alloc.py), as the sibling files run the other volume operations: three runs -- workspaces and outputs
pre-filled with 0x00, 0xFF and seeded random bytes, inputs copied into red-zoned buffers -- must leave every red zone as it was,
give the same bits, and equal the numpy oracle (tests/mesh_oracle.py), never another run of the code under test.  The shapes
cross a 64-voxel word and fill more than one block of the scan; one extraction (tests/volume_large_cases.py) fills more than
one chunk of the scan's top level."""
import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import mesh_oracle as mo
import volume_large_cases as vc

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
SHAPES = {(5, 6, 67): 0.5, (40, 40, 70): 0.3}
_WANT = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def want(shape):
    """The volume and the oracle's mesh of it, computed once."""
    if shape not in _WANT:
        v = (np.random.default_rng(sum(shape)).random(shape) < SHAPES[shape]).astype(np.uint8)
        v[1, 2, 63] = v[1, 2, 64] = 1
        _WANT[shape] = (v,) + mo.marching_cubes(v)
    return _WANT[shape]


def dev(a):
    return guard(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_extraction(A, shape):
    v, verts, faces = want(shape)
    got_v, got_f = three_fills(lambda: A.marching_cubes(dev(v)), "mesh extraction")
    assert np.array_equal(bits(host(got_v)), bits(verts)) and np.array_equal(host(got_f), faces)


def test_extraction_past_the_first_chunk_of_the_top_scan(A):
    """``ragged`` of tests/volume_large_cases.py: 1026 block totals, so the top scan runs a second chunk whose last block is not
    full.  The block-total arrays past their end and the 64-bit totals are what a wrong guard there would read uninitialised."""
    v, verts, faces = vc.mesh("ragged")
    got_v, got_f = three_fills(lambda: A.marching_cubes(dev(v), vc.LEVEL), "mesh extraction")
    assert np.array_equal(bits(host(got_v)), bits(verts)) and np.array_equal(host(got_f), faces)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_adjacency(A, shape):
    _, verts, faces = want(shape)
    indptr, indices, boundary = three_fills(lambda: A.mesh_adjacency(dev(faces), len(verts)), "mesh adjacency")
    w = mo.adjacency(faces, len(verts))
    assert np.array_equal(host(indptr), w[0]) and np.array_equal(host(indices), w[1]) and np.array_equal(host(boundary), w[2])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_smoothing(A, shape):
    _, verts, faces = want(shape)
    got = three_fills(lambda: [A.smooth_mesh(dev(verts), dev(faces), n_iter=n) for n in (1, 3)], "mesh smoothing")
    for n, g in zip((1, 3), got):
        assert np.array_equal(bits(host(g)), bits(mo.smooth(verts, faces, n, 0.2)))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_stl_records(A, shape):
    _, verts, faces = want(shape)
    centre, scale = (2.5, 3.0, 31.25), (0.07, 0.08, 0.125)

    def op():
        v, f = dev(verts), dev(faces)
        return A.stl_records(v, f), A.stl_records(v, f, centre, scale), A.transform_mesh(v, centre, scale)
    plain, moved, affine = three_fills(op, "mesh stl")
    assert np.array_equal(host(plain), mo.stl_records(verts, faces))
    assert np.array_equal(host(moved), mo.stl_records(verts, faces, centre, scale))
    assert np.array_equal(bits(host(affine)), bits(mo.affine(verts, centre, scale)))


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
