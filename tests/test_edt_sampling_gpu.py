"""The EDT with voxel spacing and the per-branch wall distance on the GPU.

``distance_transform_edt(..., sampling=s)`` against the fixture recorded from scipy (tests/golden/edt_sampling_known.npz), against
the existing integer passes at unit sampling, and against the plain-Python oracle (tests/edt_sampling_oracle.py) on volumes the
fixture does not hold, lines longer than a wave included; the device square root on non-integer arguments; ``branch_wall_distance``
against tests/wall_distance_oracle.py; the two modes of ``branch_morphometry``; the error paths.  Everything is compared bit for
bit, float64 through its bit patterns."""
import os

import numpy as np
import pytest
import torch

import edt_sampling_oracle as eo
import morphometry_oracle as mo
import wall_distance_oracle as wo
from test_edt_sampling_host import SAMPLINGS, fixture_cases

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sampled(A, vol, s):
    dist, ind = A.distance_transform_edt(dev(vol), return_indices=True, sampling=s)
    assert dist.dtype == torch.float64 and ind.dtype == torch.int32 and tuple(ind.shape) == (3,) + vol.shape
    return dist.cpu().numpy(), ind.cpu().numpy()


def check(A, vol, s, want_dist, want_ind, what):
    dist, ind = sampled(A, vol, s)
    assert np.array_equal(ind, want_ind), what
    assert np.array_equal(bits(dist), bits(want_dist)), what


# ---- the distance transform --------------------------------------------------------------------------------------------------------
def test_fixture_equality(A):
    for k, vol, s, ind, _ in fixture_cases():
        check(A, vol, s, eo.distances(ind, s), ind.astype(np.int32), f"case {k} {vol.shape} {s}")


def test_unit_sampling_equals_the_integer_passes(A):
    for k, vol, _, _, _ in fixture_cases():
        want_dist, want_ind = A.distance_transform_edt(dev(vol), return_indices=True)
        check(A, vol, (1.0, 1.0, 1.0), want_dist.cpu().numpy(), want_ind.cpu().numpy(), f"case {k} {vol.shape}")
        one = A.distance_transform_edt(dev(vol), sampling=1)                      # a scalar is repeated; a single output is a tensor
        assert isinstance(one, torch.Tensor) and np.array_equal(bits(one.cpu().numpy()), bits(want_dist.cpu().numpy()))


def random_cases():
    """20 seeded volumes the fixture does not hold, extents up to (12, 13, 14), the first three with extent 1 on one axis each."""
    rng = np.random.default_rng(20242)
    for k in range(20):
        shape = [int(rng.integers(2, m + 1)) for m in (12, 13, 14)]
        if k < 3:
            shape[k] = 1
        if k == 3:
            shape = [12, 13, 14]
        vol = (rng.random(shape) >= (0.5, 0.05, 0.005)[k % 3]).astype(np.uint8)
        if vol.all():
            vol[tuple(int(rng.integers(0, n)) for n in shape)] = 0
        yield k, vol, SAMPLINGS[(k + 3) % len(SAMPLINGS)]


def test_against_the_oracle(A):
    shapes = []
    for k, vol, s in random_cases():
        shapes.append(vol.shape)
        want_dist, want_ind = eo.edt(vol, s)
        check(A, vol, s, want_dist, want_ind, f"random case {k} {vol.shape} {s}")
    assert all(any(sh[a] == 1 for sh in shapes) for a in range(3)) and (12, 13, 14) in shapes


def long_volume():
    if "long" not in _CACHE:
        rng = np.random.default_rng(130)
        _CACHE["long"] = (rng.random((3, 130, 70)) >= 0.02).astype(np.uint8)
    return _CACHE["long"]


@pytest.mark.parametrize("transposed", (False, True))
def test_long_lines(A, transposed):
    """Lines longer than a wave and stacks of many entries: (3, 130, 70) at density 0.02, and the same volume as (70, 3, 130)."""
    vol = long_volume()
    if transposed:
        vol = np.ascontiguousarray(vol.transpose(2, 0, 1))
        assert vol.shape == (70, 3, 130)
    s = (2.5, 0.68, 0.68)
    want_dist, want_ind = eo.edt(vol, s)
    check(A, vol, s, want_dist, want_ind, f"long lines {vol.shape}")
    # the index is a nearest site: within the last bits of the minimum over all sites (tied sites may differ in the last bit)
    best = np.sqrt(eo.squared_distance_to_all_sites(vol, s))
    assert np.all(want_dist <= best * (1 + 4 * 2.0 ** -52))


@pytest.mark.parametrize("s", ((0.7, 1.0, 1.25), (1.0 / 3.0, 1.0, 7.0)))
def test_device_sqrt_is_correctly_rounded_off_the_integers(A, s):
    """8192 non-integer arguments over the two samplings: dist[i, 0, 1] of a (4096, 1, 2) volume whose only zero is (0, 0, 0)."""
    vol = np.ones((4096, 1, 2), np.uint8)
    vol[0, 0, 0] = 0
    dist, ind = sampled(A, vol, s)
    assert not ind.any()
    t0 = np.arange(4096, dtype=np.float64) * s[0]
    want = np.sqrt((t0 * t0 + 0.0) + s[2] * s[2])
    assert np.array_equal(bits(dist[:, 0, 1]), bits(want))
    assert np.array_equal(bits(dist[:, 0, 0]), bits(np.sqrt(t0 * t0)))


def test_linear_index_output(A):
    from seunet_amd import prep
    _, vol, s = next(c for c in random_cases() if c[0] == 3)
    _, ind, lin = prep._edt_sampling(dev(vol), s, False, True, True)
    ind, lin = ind.cpu().numpy(), lin.cpu().numpy()
    assert lin.dtype == np.int32 and np.array_equal(lin, np.ravel_multi_index(tuple(ind), vol.shape))


def test_no_sampling_and_voxel_mode_launch_nothing_new(A, monkeypatch):
    lib = A._lib.load()

    def forbidden(*a, **k):
        raise AssertionError("a new entry point was called on an existing path")
    for name in ("seunet_edt_sampling", "seunet_edt_sampling_workspace_bytes", "seunet_branch_wall_stats"):
        monkeypatch.setattr(lib, name, forbidden)
    parsing, skeleton = tube()
    A.distance_transform_edt(dev(parsing != 0), return_indices=True, return_sqdist=True, sampling=None)
    A.branch_morphometry(dev(parsing), dev(skeleton), (2.0, 1.0, 1.0))
    A.branch_stats(dev(parsing), dev(skeleton))
    with pytest.raises(AssertionError):
        A.distance_transform_edt(dev(parsing != 0), sampling=2.0)


# ---- the wall distance per branch -----------------------------------------------------------------------------------------------
def labelled_case():
    """(9, 10, 12), 3 labels in blobs with background between and around them, a random subset of them as the skeleton."""
    if "labelled" not in _CACHE:
        rng = np.random.default_rng(912)
        shape = (9, 10, 12)
        parsing = np.zeros(shape, np.int32)
        parsing[1:8, 1:5, 1:6] = 1
        parsing[2:7, 5:9, 2:11] = 2
        parsing[1:4, 1:4, 7:11] = 3
        parsing[rng.random(shape) < 0.1] = 0
        skeleton = (rng.random(shape) < 0.3).astype(np.uint8)                    # also on background voxels: ignored
        spacing = (0.7, 0.7, 1.25)
        indices = eo.feature_transform((parsing != 0).astype(np.uint8), spacing)
        _CACHE["labelled"] = (parsing, skeleton, spacing, indices)
    return _CACHE["labelled"]


@pytest.mark.parametrize("num", (3, 7))
def test_wall_distance_on_a_labelled_volume(A, num):
    parsing, skeleton, spacing, indices = labelled_case()
    want, status = wo.wall_distance(parsing, skeleton, indices, spacing, num)
    assert status == 0 and np.all(want["wall_count"][:3] > 0) and (skeleton[parsing == 0] != 0).any()
    wo.same_tables(A.branch_wall_distance(dev(parsing), dev(skeleton), spacing, num), want)             # the EDT computed inside
    wo.same_tables(A.branch_wall_distance(parsing, skeleton, spacing, num, indices=indices), want)     # numpy in, indices given
    if num == 3:
        wo.same_tables(A.branch_wall_distance(dev(parsing), dev(skeleton), spacing), want)              # num from the volume
    else:
        assert np.all(want["wall_count"][3:] == 0) and np.all(np.isinf(want["wall_sq_min"][3:])) and np.all(want["wall_sq_max"][3:] == 0)


def test_wall_distance_on_the_hand_case(A):
    """Indices given; a label with no skeleton voxel and a label with no voxel give (0, zeros, +inf, 0.0); a skeleton voxel whose
    parsing is 0 is ignored; a voxel without a feature is not measured."""
    parsing, skeleton, indices, spacing, num, want = wo.hand_case()
    got = A.branch_wall_distance(dev(parsing), dev(skeleton), spacing, num, indices=dev(indices))
    wo.same_tables(got, want)
    wo.same_tables(got, wo.wall_distance(parsing, skeleton, indices, spacing, num)[0])
    assert list(got) == list(wo.TABLES)
    scalar = A.branch_wall_distance(parsing, skeleton, 0.5, num, indices=indices)                      # a scalar spacing is repeated
    wo.same_tables(scalar, wo.wall_distance(parsing, skeleton, indices, (0.5, 0.5, 0.5), num)[0])


# ---- branch_morphometry ------------------------------------------------------------------------------------------------------------
def tube():
    """A straight tube of radius 3 voxels along axis 0 of a (24, 16, 16) volume, and its centre line."""
    i1, i2 = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    disc = (i1 - 8) ** 2 + (i2 - 8) ** 2 <= 9
    parsing = np.repeat(disc[None], 24, axis=0).astype(np.int32)
    skeleton = np.zeros(parsing.shape, np.uint8)
    skeleton[:, 8, 8] = 1
    return parsing, skeleton


def test_physical_mode_on_a_tube(A):
    parsing, skeleton = tube()
    spacing = (2.0, 1.0, 1.0)
    table = A.branch_morphometry(dev(parsing), dev(skeleton), spacing, inscribed="physical")
    assert abs(float(table.radius_inscribed_max[0]) - 3.0) <= 1.0 and abs(float(table.radius_inscribed_min[0]) - 3.0) <= 1.0
    indices = eo.feature_transform((parsing != 0).astype(np.uint8), spacing)
    want, _ = wo.wall_distance(parsing, skeleton, indices, spacing, 1)
    wo.same_tables({k: getattr(table, k) for k in wo.TABLES}, want)
    for k, v in wo.radii(want, spacing).items():
        assert np.array_equal(bits(getattr(table, k)), bits(v)), k
    assert table.r2_sum[0] == 0 and table.r2_min[0] == mo.INT32_MAX and table.r2_max[0] == -1
    # the same tube along axis 1, (16, 24, 16): across axis 0 its voxels are 2.0 wide.  From the centre line the nearest wall voxel
    # by index is (+-1, 0, +-3) or (+-3, 0, +-1), sqrt(10) voxels; in space it is (+-1, 0, +-3) at sqrt(2^2 + 3^2) = sqrt(13)
    turned = np.ascontiguousarray(parsing.transpose(1, 0, 2))
    turned_skel = np.ascontiguousarray(skeleton.transpose(1, 0, 2))
    phys = A.branch_morphometry(dev(turned), dev(turned_skel), spacing, inscribed="physical")
    vox = A.branch_morphometry(dev(turned), dev(turned_skel), spacing)
    unit = A.branch_morphometry(dev(turned), dev(turned_skel), (1.0, 1.0, 1.0))
    assert np.array_equal(bits(vox.radius_inscribed_max), bits(unit.radius_inscribed_max))         # blind to the spacing
    assert float(vox.radius_inscribed_max[0]) == np.sqrt(10.0) and float(phys.radius_inscribed_max[0]) == np.sqrt(13.0)


def test_default_mode_is_unchanged(A):
    from guarded_alloc import same_bits
    parsing, skeleton, spacing, _ = labelled_case()
    today = A.branch_morphometry(dev(parsing), dev(skeleton), spacing)
    voxel = A.branch_morphometry(dev(parsing), dev(skeleton), spacing, inscribed="voxel")
    same_bits(voxel, today, "inscribed='voxel' against no keyword")
    assert all(getattr(today, k) is None for k in wo.TABLES)
    sq = A.distance_transform_edt(dev(parsing != 0), return_distances=False, return_sqdist=True).cpu().numpy()
    rows = mo.rows_from_one(mo.branch_stats(parsing, skeleton, 3, sq)[0])
    for k in mo.INT_TABLES:
        assert np.array_equal(getattr(today, k), rows[k]), k
    derived = mo.derived(rows, spacing)
    for k in mo.FLOAT_COLUMNS:
        np.testing.assert_allclose(getattr(today, k), derived[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


# ---- error paths -------------------------------------------------------------------------------------------------------------------
def test_error_paths(A):
    vol = dev(np.array([[[0, 1, 1], [1, 1, 1]]], np.uint8))
    for bad in (0, -1.0, float("nan"), (1.0, 2.0), (1.0, 0.0, 1.0), (1.0, 1.0, float("nan")), (1.0, -1.0, 1.0)):
        with pytest.raises(ValueError):
            A.distance_transform_edt(vol, sampling=bad)
    with pytest.raises(ValueError):
        A.distance_transform_edt(vol, return_sqdist=True, sampling=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        A.distance_transform_edt(torch.ones((2, 3, 4), dtype=torch.uint8, device="cuda"), sampling=(0.7, 0.7, 1.25))
    parsing, skeleton, indices, spacing, num, want = wo.hand_case()
    bad = parsing.copy()
    bad[0, 2, 2] = num + 1                                      # on the skeleton
    with pytest.raises(ValueError, match="outside 0"):
        A.branch_wall_distance(bad, skeleton, spacing, num, indices=indices)
    with pytest.raises(ValueError, match="outside 0"):
        A.branch_stats(bad, skeleton, num)                      # the same error as branch_stats
    bad[0, 2, 2] = -2
    with pytest.raises(ValueError, match="outside 0"):
        A.branch_wall_distance(bad, skeleton, spacing, num, indices=indices)
    with pytest.raises(ValueError):
        A.branch_wall_distance(parsing, skeleton, spacing, 4096, indices=indices)
    with pytest.raises(ValueError):
        A.branch_wall_distance(parsing, skeleton, (1.0, 0.0, 1.0), num, indices=indices)
    with pytest.raises(ValueError):
        A.branch_wall_distance(parsing, skeleton, spacing, num, indices=indices[:, :2])
    sq = np.zeros(parsing.shape, np.int32)
    with pytest.raises(ValueError):
        A.branch_morphometry(parsing, skeleton, spacing, num, sqdist=sq, inscribed="physical")
    with pytest.raises(ValueError):
        A.branch_morphometry(parsing, skeleton, spacing, num, inscribed="mm")
    wo.same_tables(A.branch_wall_distance(parsing, skeleton, spacing, num, indices=indices), want)   # the library is usable afterwards
