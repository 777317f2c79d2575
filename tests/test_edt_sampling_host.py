"""Host checks of the EDT with voxel spacing and the per-branch wall distance: no GPU.

* tests/edt_sampling_oracle.py, the plain-Python statement of scipy's order of operations, equals the fixture recorded from
  scipy (tests/golden/edt_sampling_known.npz, scripts/make_golden_edt_sampling.py) bit for bit, and the distances recomputed from
  the fixture's indices have the recorded SHA-256;
* where scipy is installed, the oracle equals live scipy bit for bit on 210 seeded random volumes;
* tests/wall_distance_oracle.py equals tables written out by hand on a 3 x 3 x 4 case;
* ``BranchTable.from_stats`` with wall tables gives the physical radii of the stated formulae;
* ``normalize_sampling`` and the workspace layout the library reports."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import edt_sampling_oracle as eo
import morphometry_oracle as mo
import wall_distance_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "edt_sampling_known.npz")
SAMPLINGS = ((1.0, 1.0, 1.0), (0.5, 1.0, 2.0), (1.0, 2.0, 2.0), (0.7, 0.7, 1.25), (2.5, 0.68, 0.68), (1.0 / 3.0, 0.1, 7.0), (1.0, 1.0, 3.0))


def fixture_cases():
    z = np.load(GOLDEN)
    for k in range(int(z["cases"])):
        yield k, z[f"case{k}_vol"], tuple(float(v) for v in z[f"case{k}_sampling"]), z[f"case{k}_indices"], str(z[f"case{k}_sha256"])


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_fixture_holds_what_the_issue_lists():
    cases = list(fixture_cases())
    assert len(cases) >= 24 and os.path.getsize(GOLDEN) < 200 * 1024
    shapes = {v.shape for _, v, _, _, _ in cases}
    assert {(1, 1, 5), (16, 1, 3), (1, 9, 1), (7, 9, 11), (13, 10, 11)} <= shapes
    assert any(int((v == 0).sum()) == 1 for _, v, _, _, _ in cases)
    assert {tuple(s) for _, _, s, _, _ in cases} == set(SAMPLINGS)
    # whole planes of axis 2 (so whole lines of the passes along axes 1 and 2) without a site after the pass along axis 0
    assert any(v.shape[2] > 2 and ((v == 0).any(axis=(0, 1)).sum() <= 2) and (v == 0).sum() > 2 for _, v, _, _, _ in cases)
    assert all(v.size <= 1500 and (v == 0).any() for _, v, _, _, _ in cases)


def test_oracle_equals_the_fixture_bitwise():
    for k, vol, s, ind, sha in fixture_cases():
        dist, got = eo.edt(vol, s)
        assert got.dtype == np.int32 and np.array_equal(got, ind.astype(np.int32)), k
        from_indices = eo.distances(ind, s)
        assert hashlib.sha256(from_indices.tobytes()).hexdigest() == sha, k          # the numpy formula is scipy's
        assert np.array_equal(bits(dist), bits(from_indices)), k


def test_unit_sampling_cases_equal_the_integer_transform():
    """At sampling (1, 1, 1) the distance is the root of an integer and the indices are those of the unit transform: the claim
    behind reusing the integer pass along axis 0, here on the recorded scipy results themselves."""
    seen = 0
    for k, vol, s, ind, _ in fixture_cases():
        if s != (1.0, 1.0, 1.0):
            continue
        seen += 1
        sq = ((ind.astype(np.int64) - np.indices(vol.shape)) ** 2).sum(axis=0)
        assert np.array_equal(bits(eo.distances(ind, s)), bits(np.sqrt(sq.astype(np.float64)))), k
    assert seen >= 3


def test_oracle_equals_live_scipy_bitwise():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    differ_from_unit = 0
    for k in range(210):
        shape = tuple(int(v) for v in rng.integers(1, 10, 3))
        vol = (rng.random(shape) < (0.5, 0.8, 0.95)[k % 3]).astype(np.uint8)
        if vol.all():
            vol[tuple(int(rng.integers(0, n)) for n in shape)] = 0
        s = SAMPLINGS[k % len(SAMPLINGS)]
        want_dist, want_ind = ndimage.distance_transform_edt(vol, sampling=s, return_indices=True)
        dist, ind = eo.edt(vol, s)
        assert np.array_equal(ind, want_ind), (k, shape, s)
        assert np.array_equal(bits(dist), bits(want_dist)), (k, shape, s)
        differ_from_unit += not np.array_equal(ind, ndimage.distance_transform_edt(vol, return_distances=False, return_indices=True))
    assert differ_from_unit > 50          # the spacing changes which voxel is nearest, not only how far it is


def test_brute_force_bound_of_the_long_line_tests():
    """The contract's distance at the oracle's index is within 4 ulp-fractions of the minimum over all sites (tied sites may differ
    in the last bit): the bound tests/test_edt_sampling_gpu.py would use where the oracle is too slow."""
    rng = np.random.default_rng(3)
    vol = (rng.random((3, 20, 17)) >= 0.05).astype(np.uint8)
    s = (2.5, 0.68, 0.68)
    dist, _ = eo.edt(vol, s)
    best = eo.squared_distance_to_all_sites(vol, s)
    assert np.all(dist <= np.sqrt(best) * (1 + 4 * 2.0 ** -52))


def test_wall_oracle_on_the_hand_case():
    parsing, skeleton, indices, spacing, num, want = wo.hand_case()
    got, status = wo.wall_distance(parsing, skeleton, indices, spacing, num)
    assert status == 0
    wo.same_tables(got, want)
    bad = parsing.copy()
    bad[0, 2, 2] = num + 1                                     # on the skeleton: reported and ignored
    got, status = wo.wall_distance(bad, skeleton, indices, spacing, num)
    assert status == 1
    wo.same_tables(got, want)
    bad = parsing.copy()
    bad[2, 0, 0] = -3                                          # not on the skeleton: never read
    assert wo.wall_distance(bad, skeleton, indices, spacing, num)[1] == 0


def test_branch_table_formulae_in_physical_mode():
    from seunet_amd.morphometry import BranchTable
    parsing, skeleton, indices, spacing, num, wall = wo.hand_case()
    stats = mo.rows_from_one(mo.branch_stats(parsing, skeleton, num)[0])
    adjacency = mo.adjacency(parsing, num)
    table = BranchTable.from_stats(stats, adjacency, spacing, wall)
    s0, s1, s2 = spacing
    want_rms = [np.sqrt((s0 * s0 * 1 + s1 * s1 * 1 + s2 * s2 * 1) / 2), np.sqrt((s0 * s0 * 4 + s1 * s1 * 0 + s2 * s2 * 4) / 1), np.nan, np.nan]
    assert np.array_equal(bits(table.radius_inscribed_rms), bits(np.array(want_rms)))
    assert np.array_equal(bits(table.radius_inscribed_min), bits(np.array([np.sqrt(1.25), np.sqrt(17.0), np.nan, np.nan])))
    assert np.array_equal(bits(table.radius_inscribed_max), bits(np.array([2.0, np.sqrt(17.0), np.nan, np.nan])))
    radii = wo.radii(wall, spacing)
    for k, v in radii.items():
        assert np.array_equal(bits(getattr(table, k)), bits(v)), k
    for k in wo.TABLES:
        assert np.array_equal(getattr(table, k), wall[k]), k
    # the integer tables keep their "no sqdist" values, and the other columns do not depend on the mode
    assert np.all(table.r2_sum == 0) and np.all(table.r2_min == mo.INT32_MAX) and np.all(table.r2_max == -1)
    voxel = BranchTable.from_stats(stats, adjacency, spacing)
    assert all(getattr(voxel, k) is None for k in wo.TABLES) and np.all(np.isnan(voxel.radius_inscribed_max))
    for k in ("volume", "centroid", "length", "radius_equivalent", "parent", "generation"):
        assert np.array_equal(getattr(voxel, k), getattr(table, k), equal_nan=True), k
    assert set(voxel.to_dict()) == set(table.to_dict())


def test_normalize_sampling():
    from seunet_amd.prep import normalize_sampling
    assert normalize_sampling(0.7) == (0.7, 0.7, 0.7)
    assert normalize_sampling([1, 2, 3]) == (1.0, 2.0, 3.0)
    assert normalize_sampling(np.float32(0.1)) == (float(np.float32(0.1)),) * 3
    for bad in (0, -1.0, float("nan"), float("inf"), (1.0, 2.0), (1.0, 2.0, 3.0, 4.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), [[1.0, 1.0, 1.0]]):
        with pytest.raises(ValueError):
            normalize_sampling(bad)


def test_the_new_keywords_default_to_the_existing_behaviour():
    import inspect
    import seunet_amd as A
    p = inspect.signature(A.distance_transform_edt).parameters
    assert list(p)[:4] == ["volume", "return_distances", "return_indices", "return_sqdist"]
    assert p["sampling"].default is None and p["sampling"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(A.branch_morphometry).parameters["inscribed"].default == "voxel"
    assert callable(A.branch_wall_distance) and "branch_wall_distance" in A.__all__


def test_workspace_layout():
    """Four int16 volumes, each padded to 256 bytes: 8 bytes per voxel against the 12 of the integer passes."""
    import seunet_amd
    lib = seunet_amd._lib.load()
    f = lib.seunet_debug_volume_layout
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_size_t), C.c_int]
    for shape in ((1, 1, 1), (3, 5, 7), (13, 10, 11)):
        n = shape[0] * shape[1] * shape[2]
        each = (2 * n + 255) // 256 * 256
        buf = (C.c_size_t * 32)()
        assert f(12, *shape, buf, 16) == 4
        assert [buf[2 * i] for i in range(4)] == [i * each for i in range(4)] and all(buf[2 * i + 1] == each for i in range(4))
        assert lib.seunet_edt_sampling_workspace_bytes(*shape) == 4 * each < lib.seunet_edt_workspace_bytes(*shape) + 4 * 256
    assert lib.seunet_edt_sampling_workspace_bytes(0, 4, 4) == 0
