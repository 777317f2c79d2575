"""The airway cross-sections (cross_sections, branch_morphometry(cross_sections=True)) over dirty scratch memory, with red zones
around every buffer (tests/guarded_alloc.py), as tests/test_scratch_and_bounds_betti_gpu.py runs the Betti numbers: three runs --
the workspace of the point numbering and the result buffer pre-filled with 0x00, 0xFF and seeded random bytes, the inputs copied
into red-zoned buffers -- must leave every red zone as it was, give the same bits, and equal the oracle
(tests/cross_section_oracle.py), never another run of the code under test.  The cases have points at every face, edge and corner of
the volume, whose tangent windows and sample planes reach outside it, rows shorter and longer than a wave, a number of voxels that
is no multiple of a word of the point mask, and a section that covers the whole sample grid.

The skeleton passes through the wrappers' ``(a != 0).to(torch.uint8).contiguous()`` (the limit tests/guarded_alloc.py documents);
``parsing``, an int32 tensor, is used where it is, so a gather beside it would reach its red zones."""
import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import cross_section_cases as cc
import cross_section_oracle as co
from test_cross_section_gpu import same

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
SHAPES = ((2, 3, 67), (3, 5, 7), (1, 1, 130))
_WANT = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return guard(torch.from_numpy(np.array(a)).cuda())          # (a writable copy: the shared volumes are read-only)


def dense(shape):
    """Every voxel a point of one of two labels, and the oracle's result: computed once."""
    if shape not in _WANT:
        rng = np.random.default_rng(sum(shape))
        parsing = rng.integers(1, 3, shape).astype(np.int32)
        skeleton = np.ones(shape, np.uint8)
        _WANT[shape] = (parsing, skeleton, {w: co.cross_sections(parsing, skeleton, spacing=cc.ANISO, window=w) for w in (2, 7)})
    return _WANT[shape]


@pytest.mark.parametrize("window", [2, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_points_on_every_face(A, shape, window):
    parsing, skeleton, want = dense(shape)
    got = three_fills(lambda: A.cross_sections(dev(parsing), dev(skeleton), cc.ANISO, window=window), "cross sections")
    same(got, want[window])


@pytest.mark.parametrize("name", ["plane:full", "corner:", "noise:"])
def test_synthetic_cases(A, name):
    parsing, skeleton, kw = cc.case(name)
    got = three_fills(lambda: A.cross_sections(dev(parsing), dev(skeleton), **kw), "cross sections")
    same(got, co.cross_sections(parsing, skeleton, **kw))


def test_branch_table(A):
    parsing, skeleton, kw = cc.case("noise:")
    table = three_fills(lambda: A.branch_morphometry(dev(parsing), dev(skeleton), cc.ANISO, cross_sections=True), "cross section table")
    want = co.cross_sections(parsing, skeleton, spacing=cc.ANISO)
    rows = co.per_branch(want["label"], co.derived(want["count"], want["moments"], want["rim"], want["step"]), table.num)
    assert np.array_equal(table.section_count, rows["section_count"])
    for k in co.BRANCH_COLUMNS:
        np.testing.assert_allclose(getattr(table, k), rows[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
