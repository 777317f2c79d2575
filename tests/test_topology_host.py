"""The graph stage of ``airway_parse`` (se-unet-airseg_amd/topology.py) on the host, stage by stage against
tests/golden/topology_known.npz: what the reference's own functions give on synthetic trees with stable sorts
(scripts/make_golden_topology.py).  No GPU: the dense stages are replaced by the fixture's LABEL_TRANS and skeleton."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "topology_known.npz")


def _load():
    """topology.py alone, without the package around it (it needs numpy only)."""
    spec = importlib.util.spec_from_file_location("seunet_topology", os.path.join(ROOT, "se-unet-airseg_amd", "topology.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


T = _load()
Z = np.load(GOLDEN)
NCASE = int(Z["ncase"])
FLAT_KEYS = ("index", "fatherindex", "start", "has_end", "end", "member_count", "members")


def case(ci):
    p = f"case{ci}_"
    return {k[len(p):]: Z[k] for k in Z.files if k.startswith(p)}


def table_of(rec, name):
    return T.unflatten({k: rec[f"{name}_{k}"] for k in FLAT_KEYS})


def assert_table(got, rec, name):
    flat = T.flatten(got)
    for k in FLAT_KEYS:
        assert np.array_equal(flat[k], rec[f"{name}_{k}"]), (name, k)


def moments_of(volume):
    def moments(k):
        i0, i1 = np.nonzero(volume[:, :, k])
        return len(i0), int(i0.sum()), int(i1.sum())
    return moments


def z_extent(volume):
    z = np.nonzero(volume)[2]
    return int(z.min()), int(z.max())


def test_the_fixture_covers_what_the_tests_rely_on():
    recs = [case(ci) for ci in range(NCASE)]
    assert {int(r["order"]) for r in recs} == {0, 1}
    assert any(int(r["mainpart"]) > 1 and not np.array_equal(r["B"], r["B0"]) for r in recs)
    assert any(len(r["merged_index"]) < len(r["table1_index"]) for r in recs)
    assert all(len(r["merged_index"]) >= 3 for r in recs)
    assert any(any(n % 64 for n in r["label"].shape) for r in recs) and any(r["label"].shape[2] > 128 for r in recs)
    assert np.isnan(Z["nan_basev0"]).any() and np.isnan(Z["nan_basev1"]).any()
    starts = [tuple(s) for s in Z["star_table_start"]]
    assert max(starts.count(s) for s in set(starts)) == 3
    for r in recs:                                   # equal axis-2 coordinates exist, so the sort order is a choice
        assert len(np.unique(np.nonzero(r["skeleton"])[2])) < int(r["skeleton"].sum())


def test_neighbour_order_follows_its_rule():
    want = []
    for d2 in (0, -1, 1):
        group = [(d0, d1, d2) for d0 in (-1, 0, 1) for d1 in (-1, 0, 1) if (d0, d1, d2) != (0, 0, 0)]
        assert group == sorted(group, key=lambda d: (d[0], d[1]))
        want += group
    assert list(T.NEIGHBOURS) == want and len(set(want)) == 26
    assert [len([d for d in T.NEIGHBOURS if d[2] == k]) for k in (0, -1, 1)] == [8, 9, 9]
    assert T.NEIGHBOURS[0] == (-1, -1, 0) and T.NEIGHBOURS[8] == (-1, -1, -1) and T.NEIGHBOURS[25] == (1, 1, 1)


@pytest.mark.parametrize("ci", range(NCASE))
def test_orientation(ci):
    from scipy import ndimage
    r = case(ci)
    label = r["label"] != 0
    k2, k8 = T.orientation_slices(*z_extent(label))
    sizes = []
    for k in (k2, k8):
        lab, n = ndimage.label(label[:, :, k], structure=np.ones((3, 3)))
        sizes.append(int(np.bincount(lab.ravel())[1:].max()) if n else 0)
    assert T.orientation(*sizes) == int(r["order"])


@pytest.mark.parametrize("ci", range(NCASE))
def test_sorted_skeleton_and_first_subsection(ci):
    r = case(ci)
    coords = np.argwhere(r["skeleton"] != 0)                     # raster order
    B0 = T.sorted_skeleton(coords, int(r["order"]), r["label"].shape[2])
    assert np.array_equal(B0, r["B0"])
    assert_table(T.subsection(B0), r, "table0")


@pytest.mark.parametrize("ci", range(NCASE))
def test_base_vector_and_mainpart_index(ci):
    r = case(ci)
    lt = r["label_trans"]
    basev = T.base_vector(*z_extent(lt), int(r["order"]), moments_of(lt))
    assert np.array_equal(basev.view(np.int64), r["basev"].view(np.int64))
    assert T.find_mainpart_index(int(r["B0"][0, 2]), table_of(r, "table0"), basev) == int(r["mainpart"])


@pytest.mark.parametrize("order", (0, 1))
def test_an_empty_slice_gives_nan_and_index_zero(order):
    vol = Z["nan_volume"]
    basev = T.base_vector(*z_extent(vol), order, moments_of(vol))
    want = Z[f"nan_basev{order}"]
    assert np.array_equal(np.isnan(basev), np.isnan(want)) and np.isnan(basev).any()
    assert np.array_equal(basev[~np.isnan(basev)], want[~np.isnan(want)])
    r = case(0)
    assert T.find_mainpart_index(int(r["B0"][0, 2]), table_of(r, "table0"), basev) == 0


@pytest.mark.parametrize("ci", range(NCASE))
def test_smoothing_and_second_subsection(ci):
    r = case(ci)
    mainpart = int(r["mainpart"])
    if mainpart > 1:
        B = T.process_mainairway_points(r["B0"], table_of(r, "table0"), mainpart)
        assert np.array_equal(B, r["B"]) and len(B) < len(r["B0"])
        assert_table(T.subsection(B), r, "table1")
    else:
        assert np.array_equal(r["B"], r["B0"])
        assert_table(table_of(r, "table0"), r, "table1")


@pytest.mark.parametrize("ci", range(NCASE))
def test_merging_flip_and_grade(ci):
    r = case(ci)
    before = table_of(r, "table1")
    merged = T.merging(before, 5)
    assert T.flatten(before)["members"].shape == r["table1_members"].shape          # the argument is left alone
    assert_table(before, r, "table1")
    if int(r["order"]) == 1:
        merged = T.flip_back(merged, r["label"].shape[2])
    assert_table(merged, r, "merged")
    codes = T.grade(merged)
    assert [c for c, _ in codes] == list(r["codes"]) and [f for _, f in codes] == list(r["father_codes"])


def test_multi_way_start_with_three_branches():
    """The hand-drawn star: siblings share the running member list, branch numbers follow the reference's rule."""
    table = T.subsection(Z["star_B"])
    flat = T.flatten(table)
    for k in FLAT_KEYS:
        assert np.array_equal(flat[k], Z[f"star_table_{k}"]), k
    merged = T.merging(table, 5)
    flat = T.flatten(merged)
    for k in FLAT_KEYS:
        assert np.array_equal(flat[k], Z[f"star_merged_{k}"]), k
    codes = T.grade(merged)
    assert [c for c, _ in codes] == list(Z["star_codes"]) and [f for _, f in codes] == list(Z["star_father_codes"])
    first3 = table[:3]
    assert len({b["start"] for b in first3}) == 1
    assert first3[1]["member"][:len(first3[0]["member"])] == first3[0]["member"]       # the shared list


@pytest.mark.parametrize("ci", range(NCASE))
def test_graph_stage_and_cd(ci):
    r = case(ci)
    lt = r["label_trans"]
    trace = {}
    merged, codes = T.graph_stage(np.argwhere(r["skeleton"] != 0), r["label"].shape, int(r["order"]), z_extent(lt), moments_of(lt), 5, trace)
    assert_table(merged, r, "merged")
    assert np.array_equal(trace["B"], r["B"]) and trace["mainpart"] == int(r["mainpart"])
    lin, val = T.branch_labels(merged, r["label"].shape)
    assert len(np.unique(lin)) == len(lin)
    cd = np.zeros(r["label"].size, np.int32)
    cd[lin] = val
    assert np.array_equal(cd.reshape(r["label"].shape), r["cd"].astype(np.int32))


def test_first_writer_wins_in_cd():
    table = [{"index": 1, "fatherindex": 0, "start": (0, 0, 0), "member": [(0, 0, 1), (0, 0, 2)], "end": (0, 0, 3)},
             {"index": 2, "fatherindex": 1, "start": (0, 0, 3), "member": [(0, 1, 3), (0, 0, 2)]},
             {"index": 3, "fatherindex": 1, "start": (0, 1, 3), "member": [(1, 1, 3)]}]
    lin, val = T.branch_labels(table, (2, 2, 4))
    got = dict(zip(lin.tolist(), val.tolist()))
    at = lambda p: (p[0] * 2 + p[1]) * 4 + p[2]
    assert got == {at((0, 0, 0)): 1, at((0, 0, 1)): 1, at((0, 0, 2)): 1, at((0, 0, 3)): 1, at((0, 1, 3)): 2, at((1, 1, 3)): 3}
    assert any(int(c["cd"].max()) and _claimed_twice(c) for c in (case(ci) for ci in range(NCASE)))


def _claimed_twice(r):
    seen = {}
    for k, b in enumerate(table_of(r, "merged"), start=1):
        for p in T.branch_voxels(b):
            if seen.setdefault(p, k) != k:
                return True
    return False


def test_smoothing_interpolation_is_scipys():
    """2000 seeded random integer polylines of 6-80 points: the knots of ``smooth_points``, scipy's extrapolating linear
    ``interp1d`` at 0 .. n - 1, bitwise after ``np.round``."""
    from scipy.interpolate import interp1d
    rng = np.random.default_rng(20261018)
    for _ in range(2000):
        n = int(rng.integers(6, 81))
        P = rng.integers(0, 600, size=(n, 3))
        knots = np.append(np.arange(0, n, n // 3), n - 1)
        if abs(int(knots[-2]) - int(knots[-1])) < 5:
            knots = np.delete(knots, -2)
        for a in range(3):
            want = interp1d(knots, P[knots, a], kind="linear", fill_value="extrapolate")(np.linspace(0, n - 1, n))
            got = T.interp_linear(knots, P[knots, a], n)
            assert np.array_equal(np.round(got).astype(int), np.round(want).astype(int))
            assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_smooth_points_holds_steps_and_sorts_stably():
    P = np.array([(0, 0, 9), (0, 5, 8), (0, 5, 8), (1, 9, 7), (1, 9, 5), (2, 9, 5), (2, 9, 3), (3, 9, 2), (9, 9, 1), (9, 0, 0)])
    got = T.smooth_points(P)
    assert got.shape[1] == 3 and len(got) <= len(P)
    assert (np.diff(got[:, 2]) > 0).all()                        # one row per axis-2 value, ascending
    assert (np.abs(np.diff(got, axis=0)) <= 1).all()             # each coordinate within 1 of the row before


def test_value_errors_name_their_stage():
    with pytest.raises(ValueError, match="skeleton"):
        T.sorted_skeleton(np.zeros((0, 3), np.int64), 0, 10)
    with pytest.raises(ValueError, match="subsection"):
        T.subsection(np.zeros((0, 3), np.int64))
    two = [{"index": 1, "fatherindex": 0, "start": (0, 0, 0), "member": [(0, 0, k) for k in range(1, 9)]},
           {"index": 2, "fatherindex": 1, "start": (0, 0, 9), "member": [(0, 0, k) for k in range(10, 19)]}]
    with pytest.raises(ValueError, match="grade.*2 branches"):
        T.grade(two)
    overflow = [dict(two[0], fatherindex=0), dict(two[1], index=1, fatherindex=7)]       # a father number past the last index
    with pytest.raises(ValueError, match="merging.*child_num"):
        T.merging(overflow, 5)
    with pytest.raises(ValueError, match="merging"):
        T.merging([{"index": 1, "fatherindex": 0, "start": (0, 0, 0), "member": []}], 5)   # every branch short: nothing left
    n2 = 12
    flipped = [{"index": 1, "fatherindex": 0, "start": (0, 0, 0), "member": [(0, 0, 1)]}]       # flipped back: z = n2
    with pytest.raises(ValueError, match="cd.*outside the volume"):
        T.branch_labels(T.flip_back(flipped, n2), (2, 2, n2))
    with pytest.raises(ValueError, match="smoothing"):
        T.smooth_points(np.array([(0, 0, 0), (0, 0, 1)]))
