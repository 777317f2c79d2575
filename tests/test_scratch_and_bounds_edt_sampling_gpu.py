"""The EDT with voxel spacing and the per-branch wall distance over dirty scratch memory, with red zones around every buffer
(tests/guarded_alloc.py), as tests/test_scratch_and_bounds_morphometry_gpu.py runs the morphometry: three runs -- the outputs and
the workspace pre-filled with 0x00, 0xFF and seeded random bytes, the inputs copied into red-zoned buffers -- must leave every
red zone as it was, give the same bits, and equal the oracles (tests/edt_sampling_oracle.py, tests/wall_distance_oracle.py), never
another run of the code under test.  The shapes have rows that cross a wave end and rows shorter than a wave, lines without a
site, and more lines than one workgroup."""
import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import edt_sampling_oracle as eo
import wall_distance_oracle as wo

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
SHAPES = ((2, 3, 67), (3, 5, 7), (20, 17, 3))                    # (20, 17, 3): 340 lines in the pass along axis 2
SPACING = (0.7, 0.8, 1.25)
NUM = 5
_WANT = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def want(shape):
    """Random inputs of a shape and the oracles' results for them, computed once."""
    if shape not in _WANT:
        rng = np.random.default_rng(sum(shape))
        parsing = rng.integers(1, NUM, shape).astype(np.int32)               # labels 1 .. NUM - 1: label NUM has no voxel
        parsing[rng.random(shape) < 0.04] = 0
        parsing[0, -1, -1] = 0                                               # (few zeros: many planes of axis 2 have none)
        skeleton = (rng.random(shape) < 0.6).astype(np.uint8)
        mask = (parsing != 0).astype(np.uint8)
        if shape[2] > 3:
            assert not (mask == 0).any(axis=(0, 1)).all()                    # lines without a site in the pass along axis 1
        dist, indices = eo.edt(mask, SPACING)
        tables, status = wo.wall_distance(parsing, skeleton, indices, SPACING, NUM)
        assert status == 0
        _WANT[shape] = (parsing, skeleton, mask, dist, indices, tables)
    return _WANT[shape]


def dev(a):
    return guard(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("shape", SHAPES)
def test_distance_transform(A, shape):
    _, _, mask, dist, indices, _ = want(shape)
    got_dist, got_ind = three_fills(lambda: A.distance_transform_edt(dev(mask), return_indices=True, sampling=SPACING), "edt sampling")
    assert np.array_equal(got_ind.cpu().numpy(), indices) and np.array_equal(bits(got_dist.cpu().numpy()), bits(dist))


@pytest.mark.parametrize("shape", SHAPES)
def test_branch_wall_distance(A, shape):
    parsing, skeleton, _, _, indices, tables = want(shape)
    given = three_fills(lambda: A.branch_wall_distance(dev(parsing), dev(skeleton), SPACING, NUM, indices=dev(indices)), "wall distance")
    wo.same_tables(given, tables)
    inside = three_fills(lambda: A.branch_wall_distance(dev(parsing), dev(skeleton), SPACING, NUM), "wall distance, EDT inside")
    wo.same_tables(inside, tables)


def test_branch_morphometry_physical(A):
    parsing, skeleton, _, _, _, tables = want(SHAPES[0])
    got = three_fills(lambda: A.branch_morphometry(dev(parsing), dev(skeleton), SPACING, NUM, inscribed="physical"), "morphometry physical")
    wo.same_tables({k: getattr(got, k) for k in wo.TABLES}, tables)
    for k, v in wo.radii(tables, SPACING).items():
        assert np.array_equal(bits(getattr(got, k)), bits(v)), k


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
