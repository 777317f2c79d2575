"""The airway walls (airway_walls, branch_morphometry(walls=)) over dirty scratch memory, with red zones around every buffer
(tests/guarded_alloc.py), as tests/test_scratch_and_bounds_cross_section_gpu.py runs the cross-sections: three runs -- the
sections' workspace and rows, the uploaded rows and the result buffer pre-filled with 0x00, 0xFF and seeded random bytes, the
inputs copied into red-zoned buffers -- must leave every red zone as it was, give the same bits, and equal the oracle
(tests/airway_wall_oracle.py), never another run of the code under test.  The dense cases have points at every face, edge and
corner of the volume, whose rays leave it at once or after a few samples, rows shorter and longer than a wave and extents of 1 and 2,
where no or only one layer of corner cells exists.

The CT, an int16 or float32 tensor, and ``parsing``, an int32 tensor, are used where they are, so a corner gather or a label gather
beside them would reach their red zones; the skeleton passes through the wrappers' ``(a != 0).to(torch.uint8).contiguous()``."""
import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import airway_wall_cases as wc
import airway_wall_oracle as wo
import cross_section_oracle as co
from test_airway_wall_gpu import given, same

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
SHAPES = ((2, 3, 67), (3, 5, 7), (1, 1, 130), (4, 6, 9))
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
    """Every voxel a skeleton voxel, a third of them background, and the oracle's result: computed once."""
    if shape not in _WANT:
        rng = np.random.default_rng(sum(shape))
        parsing = rng.integers(0, 3, shape).astype(np.int32)
        skeleton = np.ones(shape, np.uint8)
        ct = wc.noise_ct(shape, seed=sum(shape))
        sections = co.cross_sections(parsing, skeleton, spacing=wc.ANISO)
        _WANT[shape] = (ct, parsing, skeleton, sections,
                        {f: wo.airway_walls(ct.astype(np.float32) if f else ct, parsing, sections, wc.directions(), wc.ANISO, min_contrast=50.0)
                         for f in (False, True)})
    return _WANT[shape]


@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_points_on_every_face(A, shape, as_float):
    ct, parsing, skeleton, _, want = dense(shape)
    ct = ct.astype(np.float32) if as_float else ct
    got = three_fills(lambda: A.airway_walls(dev(ct), dev(parsing), dev(skeleton), wc.ANISO, min_contrast=50.0, return_rays=True),
                      "airway walls")
    same(got, want[as_float])


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_sections_given(A, shape):
    ct, parsing, _, sections, want = dense(shape)
    got = three_fills(lambda: A.airway_walls(dev(ct), dev(parsing), None, wc.ANISO, sections=given(A, sections, wc.ANISO), min_contrast=50.0),
                      "airway walls")
    same(got, want[False])


@pytest.mark.parametrize("name", ["border:", "noise:", "tube:oblique"])
def test_named_cases(A, name):
    c = wc.case(name)
    got = three_fills(lambda: A.airway_walls(dev(c["ct"]), dev(c["parsing"]), dev(c["skeleton"]), c["spacing"], return_rays=True),
                      "airway walls")
    same(got, wc.want(name))


def test_branch_table(A):
    c, want = wc.case("noise:"), wc.want("noise:")

    def op():
        ct, p, s = dev(c["ct"]), dev(c["parsing"]), dev(c["skeleton"])
        return A.branch_morphometry(p, s, c["spacing"], walls=A.airway_walls(ct, p, s, c["spacing"], min_rays=8))

    table = three_fills(op, "airway wall table")
    rows = wo.per_branch(want["label"], wo.derived(want["mask"], want["sums"], 8), table.num)
    assert np.array_equal(table.wall_sections, rows["wall_sections"])
    for k in wo.BRANCH_COLUMNS:
        np.testing.assert_allclose(getattr(table, k), rows[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
