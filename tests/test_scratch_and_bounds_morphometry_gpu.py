"""The branch morphometry (branch_stats, branch_morphometry) over dirty scratch memory, with red zones around every buffer
(tests/guarded_alloc.py), as the other test_scratch_and_bounds_* files run their operations: three runs -- the result buffer and
every workspace of the steps behind the defaults pre-filled with 0x00, 0xFF and seeded random bytes, the inputs copied into
red-zoned buffers -- must leave every red zone as it was, give the same bits, and equal the numpy oracle
(tests/morphometry_oracle.py), never another run of the code under test.  The shapes have rows that cross a wave end and rows
shorter than a wave; the fixture is a real parse with more than one workgroup."""
import os

import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import morphometry_oracle as mo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
SHAPES = ((2, 3, 67), (3, 5, 7))
SPACING = (0.7, 0.8, 1.25)
NUM = 600                                                    # labels that share a slot of the volume pass's LDS table (k and k + 256)
_WANT = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def want(shape):
    """Random inputs of a shape and the oracle's tables of them, computed once."""
    if shape not in _WANT:
        rng = np.random.default_rng(sum(shape))
        parsing = rng.integers(0, NUM + 1, shape).astype(np.int32)
        parsing[..., :5] = 2
        skeleton = (rng.random(shape) < 0.6).astype(np.uint8)
        sqdist = rng.integers(0, 1000, shape).astype(np.int32)
        tables, status = mo.branch_stats(parsing, skeleton, NUM, sqdist)
        assert status == 0
        _WANT[shape] = (parsing, skeleton, sqdist, mo.rows_from_one(tables))
    return _WANT[shape]


def dev(a):
    return guard(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def same(got, rows):
    for k in mo.INT_TABLES:
        have = got[k] if isinstance(got, dict) else getattr(got, k)
        assert have.dtype == rows[k].dtype and np.array_equal(have, rows[k]), k


@pytest.mark.parametrize("shape", SHAPES)
def test_branch_stats(A, shape):
    parsing, skeleton, sqdist, rows = want(shape)
    got = three_fills(lambda: A.branch_stats(dev(parsing), dev(skeleton), NUM, dev(sqdist)), "morphometry stats")
    same(got, rows)


@pytest.mark.parametrize("shape", SHAPES)
def test_branch_morphometry(A, shape):
    parsing, skeleton, sqdist, rows = want(shape)
    got = three_fills(lambda: A.branch_morphometry(dev(parsing), dev(skeleton), SPACING, NUM, dev(sqdist)), "morphometry table")
    same(got, rows)
    derived = mo.derived(rows, SPACING)
    for k in mo.FLOAT_COLUMNS:
        np.testing.assert_allclose(getattr(got, k), derived[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    parent, generation, _ = mo.branch_tree(rows["voxels"].tolist(), mo.adjacency(parsing, NUM))
    assert np.array_equal(got.parent, parent) and np.array_equal(got.generation, generation)


def test_fixture_with_the_defaults(A):
    """Case 1 of the parse fixtures; the skeleton and the squared EDT come from the defaults, so their workspaces are dirty too."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "parse_known.npz"))
    parsing = z["case1_parsing"].astype(np.int32)
    num = int(parsing.max())
    got = three_fills(lambda: A.branch_morphometry(dev(parsing), spacing=SPACING), "morphometry defaults")
    skeleton = A.skeletonize_3d(torch.from_numpy((parsing != 0).astype(np.uint8)).cuda())    # tested against its own oracle elsewhere
    sqdist = A.distance_transform_edt(torch.from_numpy((parsing != 0).astype(np.uint8)).cuda(), return_distances=False, return_sqdist=True)
    tables, status = mo.branch_stats(parsing, skeleton.cpu().numpy(), num, sqdist.cpu().numpy())
    assert status == 0 and got.num == num
    same(got, mo.rows_from_one(tables))
    given = three_fills(lambda: A.branch_stats(dev(parsing), dev(z["case1_skeleton"]), num), "morphometry fixture")
    tables, _ = mo.branch_stats(parsing, z["case1_skeleton"], num)
    same(given, mo.rows_from_one(tables))


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
