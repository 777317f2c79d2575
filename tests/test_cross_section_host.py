"""The cross-section oracle (tests/cross_section_oracle.py) against known answers, and the host side of
``seunet_amd.morphometry`` (the derived columns, the per-branch aggregation); no GPU.  tests/test_cross_section_gpu.py then holds
the device to the oracle bit for bit on these same inputs (tests/cross_section_cases.py).

Measured figures of the oracle that the assertions below rest on (DESIGN.md section 3p records them):
  cylinders of radius 5 under spacing (1.25, 0.7, 0.7): |area - pi r^2| is 0.35 .. 3.32 against derived bounds of 36.3 .. 45.8;
  |diameter - 2 r| is at most 0.617 over the nine cases (axis 1 or 2, step 0.5, the major diameter);
  digital lines of 24 voxels, largest angle between the tangent and the true direction over all points, the same at window 3 and 4
  (the ends decide): (1,1,0) 1.2e-6 deg, (3,2,1) 3.944 deg, (1,1,1) 0, (1,2,5) 6.823 deg; over the points at least `window` from an
  end: window 3: 1.2e-6, 1.340, 0, 2.184 deg; window 4: 1.2e-6, 2.271, 0, 2.429 deg."""
import numpy as np
import pytest

import cross_section_cases as cc
import cross_section_oracle as co

DIAMETER_DEVIATION = 0.617                                   # the oracle's largest |diameter - 2 r| over the nine cylinder cases
LINE_ANGLES = {3: ((1.3e-6, 1.3e-6), (3.945, 1.341), (0.0, 0.0), (6.823, 2.184)),       # window -> per direction (all points, inner)
               4: ((1.3e-6, 1.3e-6), (3.945, 2.272), (0.0, 0.0), (6.823, 2.429))}
MARGIN = 1.3                                                 # assertions on measured figures allow 30 % over them
_RESULTS = {}


def result(name, **over):
    """The oracle's columns (integer and derived) of a named case, computed once."""
    key = (name, tuple(sorted(over.items())))
    if key not in _RESULTS:
        parsing, skeleton, kw = cc.case(name)
        r = co.cross_sections(parsing, skeleton, **dict(kw, **over))
        assert r["status"] == 0
        r.update(co.derived(r["count"], r["moments"], r["rim"], r["step"]))
        _RESULTS[key] = r
    return _RESULTS[key]


def moments_of(plane):
    """(count, [sum i, sum j, sum i^2, sum j^2, sum ij]) of a 0/1 (PLANE, PLANE) array indexed [i + 31, j + 31]."""
    i, j = np.nonzero(plane)
    i, j = i - cc.PLANE // 2, j - cc.PLANE // 2
    return int(plane.sum()), [int(i.sum()), int(j.sum()), int((i * i).sum()), int((j * j).sum()), int((i * j).sum())]


# ---- tangents ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_straight_line_gives_the_axis_exactly_and_the_basis_of_the_tie_rule(axis):
    r = result(f"line:{axis}")
    e = np.eye(3)
    assert np.array_equal(r["tangent"], np.tile(e[axis], (12, 1)))
    assert r["support"].tolist() == [5, 6, 7, 8, 9, 9, 9, 9, 8, 7, 6, 5]
    u, v = co.basis(r["tangent"])
    # the smallest |t_a|, the lowest index on a tie: axis 1 for t = e_0, axis 0 otherwise; v = t x u
    want_u = e[1] if axis == 0 else e[0]
    assert np.array_equal(u, np.tile(want_u, (12, 1))) and np.array_equal(v, np.tile(np.cross(e[axis], want_u), (12, 1)))
    # the plane perpendicular to the axis cuts the 9 x 9 tube: the samples whose nearest voxel is at most 4 from the line's
    s = np.array(cc.ANISO)
    sides = [np.floor(np.arange(-31, 32) * cc.LINE_STEP / s[a] + 0.5) for a in range(3) if a != axis]
    assert np.all(r["count"] == np.prod([int((np.abs(k) <= 4).sum()) for k in sides])) and np.all(r["rim"] == 0)


@pytest.mark.parametrize("k", range(len(cc.DIRECTIONS)))
@pytest.mark.parametrize("window", [3, 4])
def test_oblique_digital_lines(k, window):
    d = np.asarray(cc.DIRECTIONS[k], dtype=np.float64)
    r = result(f"oblique:{k}", window=window)
    t = r["tangent"]
    assert np.all(r["support"] >= 3)
    assert np.allclose((t * t).sum(axis=1), 1.0, rtol=0, atol=1e-15)
    # the sign rule: the component of largest magnitude is positive
    assert np.all(t[np.arange(len(t)), np.abs(t).argmax(axis=1)] > 0)
    angle = np.degrees(np.arccos(np.clip(t @ (d / np.linalg.norm(d)), -1.0, 1.0)))
    every, inner = LINE_ANGLES[window][k]
    print(f"direction {cc.DIRECTIONS[k]} window {window}: {angle.max():.4g} deg over all points, {angle[window:-window].max():.4g} inner")
    assert angle.max() <= MARGIN * every + 1e-9 and angle[window:-window].max() <= MARGIN * inner + 1e-9
    # deterministic, and blind to the order the voxels are met in: the line turned round gives the same tangents, turned round
    parsing, skeleton, _ = cc.case(f"oblique:{k}")
    back = co.cross_sections(parsing[::-1, ::-1, ::-1], skeleton[::-1, ::-1, ::-1], window=window)
    again = co.cross_sections(parsing, skeleton, window=window)
    assert np.array_equal(again["tangent"].view(np.int64), t.view(np.int64))
    np.testing.assert_allclose(back["tangent"][::-1], t, rtol=0, atol=1e-12)


# ---- cylinders --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", cc.CYLINDER_STEPS)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cylinder_area_and_diameters(axis, step):
    r = result(f"cylinder:{axis},{step}")
    assert len(r["label"]) == 20 and np.array_equal(r["tangent"], np.tile(np.eye(3)[axis], (20, 1)))
    assert r["valid"].all() and np.all(r["count"] > 0) and np.all(r["rim"] == 0)         # none invalid, none truncated
    delta = 0.5 * np.linalg.norm(cc.ANISO) + step / np.sqrt(2.0)
    bound = 2.0 * np.pi * cc.RADIUS * delta + np.pi * delta * delta
    error = np.abs(r["area"] - np.pi * cc.RADIUS ** 2).max()
    deviation = max(np.abs(r["diameter_major"] - 2 * cc.RADIUS).max(), np.abs(r["diameter_minor"] - 2 * cc.RADIUS).max())
    print(f"cylinder axis {axis} step {step}: area error {error:.4g} (bound {bound:.4g}), diameter deviation {deviation:.4g}")
    assert error <= bound
    assert deviation <= MARGIN * DIAMETER_DEVIATION
    assert np.all(r["diameter_major"] >= r["diameter_minor"])


# ---- flood fill -------------------------------------------------------------------------------------------------------------
def fill_iterations(plane):
    """Steps of growth by one 4-neighbour ring from the centre until nothing changes."""
    f = np.zeros(plane.shape, bool)
    f[cc.PLANE // 2, cc.PLANE // 2] = True
    for n in range(10000):
        g = f.copy()
        g[1:] |= f[:-1]; g[:-1] |= f[1:]; g[:, 1:] |= f[:, :-1]; g[:, :-1] |= f[:, 1:]
        g &= plane != 0
        if np.array_equal(g, f):
            return n
        f = g


def test_fill_follows_a_spiral_longer_than_a_wave():
    plane = cc.pattern("spiral")
    assert fill_iterations(plane) > 64 * 20                  # the corridor is about 1900 samples long
    r = result("plane:spiral")
    count, moments = moments_of(plane)
    assert count == 1921 and np.all(r["count"] == count) and np.all(r["moments"] == moments) and np.all(r["rim"] == 0)
    assert np.array_equal(r["tangent"], np.tile([1.0, 0.0, 0.0], (5, 1)))


def test_fill_keeps_the_centre_component_only():
    count, moments = moments_of(cc.disc(6))
    assert moments_of(cc.pattern("two_discs"))[0] > count
    r = result("plane:two_discs")
    assert np.all(r["count"] == count) and np.all(r["moments"] == moments) and r["valid"].all()


def test_a_section_that_reaches_the_grid_edge_is_truncated():
    r = result("plane:full")
    assert np.all(r["count"] == 63 * 63) and np.all(r["rim"] == 4 * 62) and not r["valid"].any()


def test_samples_outside_the_volume_are_outside_the_section():
    r = result("corner:")
    k = np.arange(5)
    assert np.all(r["count"] == 25) and np.all(r["rim"] == 0)
    assert np.all(r["moments"] == [5 * k.sum(), 5 * k.sum(), 5 * (k * k).sum(), 5 * (k * k).sum(), k.sum() ** 2])


def test_same_label_false_crosses_a_label_change():
    own, every = result("plane:labels"), result("plane_any:labels")
    assert np.all(own["count"] == cc.disc(6).sum()) and np.all(every["count"] == cc.disc(11).sum())
    assert np.all(every["moments"] == moments_of(cc.disc(11))[1])
    assert np.array_equal(own["tangent"], every["tangent"]) and np.array_equal(own["support"], every["support"])


# ---- invalid tangents -------------------------------------------------------------------------------------------------------
def test_invalid_windows():
    parsing = np.ones((5, 5, 5), np.int32)
    for voxels in ([(2, 2, 2)], [(2, 2, 2), (2, 2, 3)]):     # a single voxel, two voxels: n < 3
        skeleton = np.zeros((5, 5, 5), np.uint8)
        for v in voxels:
            skeleton[v] = 1
        r = co.cross_sections(parsing, skeleton)
        assert r["support"].tolist() == [len(voxels)] * len(voxels)
        assert not r["tangent"].any() and not r["count"].any() and not r["moments"].any() and not r["rim"].any()
    # three voxels of the window, but of three labels: each point sees itself alone
    skeleton = np.zeros((5, 5, 5), np.uint8)
    skeleton[2, 2, 1:4] = 1
    labels = parsing.copy()
    labels[2, 2, 1:4] = (1, 2, 3)
    r = co.cross_sections(labels, skeleton)
    assert r["support"].tolist() == [1, 1, 1] and not r["count"].any()
    # a scatter matrix that is all equal, all zero: the spacing squared underflows, max |C_ab| = 0
    r = co.cross_sections(parsing, skeleton, spacing=(1e-170, 1e-170, 1e-170), step=1.0)
    assert r["support"].tolist() == [3, 3, 3] and not r["tangent"].any() and not r["count"].any()
    # a window that is all skeleton has three equal eigenvalues: the tie rule picks axis 0, and the result is valid
    r = co.cross_sections(parsing, np.ones((5, 5, 5), np.uint8), window=1)
    centre = 2 * 25 + 2 * 5 + 2
    assert r["support"][centre] == 27 and r["tangent"][centre].tolist() == [1.0, 0.0, 0.0] and r["count"][centre] > 0


def test_a_label_outside_the_range_sets_the_status():
    parsing, skeleton, kw = cc.case("noise:")
    assert co.cross_sections(parsing, skeleton, num=3, **kw)["status"] == 0
    assert co.cross_sections(parsing, skeleton, num=2, **kw)["status"] == 1


# ---- the host columns of the package --------------------------------------------------------------------------------------------
def hand_rows():
    """Five hand-made rows: a single sample; a 3 x 3 block; a 1 x 4 bar along i off centre; a truncated row; an empty row."""
    count = [1, 9, 4, 9, 0]
    moments = [[0, 0, 0, 0, 0], [0, 0, 6, 6, 0], [10, 8, 30, 16, 20], [0, 0, 6, 6, 0], [0, 0, 0, 0, 0]]
    rim = [0, 0, 0, 2, 0]
    label = [1, 1, 3, 3, 2]
    return label, count, moments, rim


def test_derived_columns_from_hand_made_rows():
    from seunet_amd import morphometry as M
    label, count, moments, rim = hand_rows()
    h = 0.5
    cs = M.CrossSections.from_columns(np.zeros((5, 3)), label, [3] * 5, np.zeros((5, 3)), count, moments, rim, h, num=3)
    assert len(cs) == 5 and cs.num == 3 and cs.step == h
    assert cs.valid.tolist() == [True, True, True, False, False]
    assert np.array_equal(cs.area, np.array(count) * 0.25)
    # one sample: an h x h square, variance 1/12 both ways; 3 x 3: variance 6/9 + 1/12 = 3/4; the bar: 5/4 + 1/12 along i, 1/12 along j
    want_major = [4 * h * np.sqrt(1 / 12), 4 * h * np.sqrt(0.75), 4 * h * np.sqrt(1.25 + 1 / 12), 4 * h * np.sqrt(0.75), np.nan]
    want_minor = [4 * h * np.sqrt(1 / 12), 4 * h * np.sqrt(0.75), 4 * h * np.sqrt(1 / 12), 4 * h * np.sqrt(0.75), np.nan]
    np.testing.assert_allclose(cs.diameter_major, want_major, rtol=1e-14, equal_nan=True)
    np.testing.assert_allclose(cs.diameter_minor, want_minor, rtol=1e-13, equal_nan=True)
    want = co.derived(count, moments, rim, h)
    for k in co.FLOAT_COLUMNS:
        np.testing.assert_allclose(getattr(cs, k), want[k], rtol=1e-12, equal_nan=True, err_msg=k)
    assert np.array_equal(cs.valid, want["valid"])
    # a disc of radius 10 samples has the diameter 2 r h
    n, m5 = moments_of(cc.disc(10))
    d = M.CrossSections.from_columns(np.zeros((1, 3)), [1], [3], np.zeros((1, 3)), [n], [m5], [0], h)
    assert abs(d.diameter_major[0] - 10.0) < 0.1 and abs(d.diameter_minor[0] - 10.0) < 0.1
    with pytest.raises(ValueError):
        M.CrossSections.from_columns(np.zeros((0, 3)), [], [], np.zeros((0, 3)), [], np.zeros((0, 5)), [], 0.0)


def test_per_branch_aggregation_and_the_branch_table():
    from seunet_amd import morphometry as M
    label, count, moments, rim = hand_rows()
    h = 0.5
    cs = M.CrossSections.from_columns(np.zeros((5, 3)), label, [3] * 5, np.zeros((5, 3)), count, moments, rim, h, num=3)
    got = cs.per_branch()
    assert got["section_count"].tolist() == [2, 0, 1] and got["section_count"].dtype == np.int64
    assert got["area_mean"].tolist()[0] == 1.25 and got["area_min"][0] == 0.25 and got["area_max"][0] == 2.25 and got["area_median"][0] == 1.25
    assert got["area_mean"][2] == 1.0 and got["area_median"][2] == 1.0           # the truncated row of label 3 does not count
    assert all(np.isnan(got[k][1]) for k in M.SECTION_COLUMNS[1:])               # label 2 has no valid row
    assert got["diameter_major_mean"][0] == pytest.approx((cs.diameter_major[0] + cs.diameter_major[1]) / 2, rel=1e-15)
    want = co.per_branch(label, co.derived(count, moments, rim, h), 3)
    for k in M.SECTION_COLUMNS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, equal_nan=True, err_msg=k)
    # the branch table: the columns appear with `sections`, and stay None without
    import morphometry_oracle as mo
    rng = np.random.default_rng(3)
    parsing = rng.integers(0, 4, (4, 5, 6)).astype(np.int32)
    skeleton = (rng.random((4, 5, 6)) < 0.5).astype(np.uint8)
    tables, _ = mo.branch_stats(parsing, skeleton, 3)
    rows = mo.rows_from_one(tables)
    adjacency = mo.adjacency(parsing, 3)
    plain = M.BranchTable.from_stats(rows, adjacency)
    table = M.BranchTable.from_stats(rows, adjacency, sections=cs)
    for k in M.SECTION_COLUMNS:
        assert getattr(plain, k) is None and k not in plain.to_dict()
        np.testing.assert_array_equal(getattr(table, k), got[k])
        assert table.to_dict()[k] is getattr(table, k)
    assert set(table.to_dict()) - set(plain.to_dict()) == set(M.SECTION_COLUMNS)
    for k in mo.FLOAT_COLUMNS:
        np.testing.assert_array_equal(getattr(table, k), getattr(plain, k))


def test_argument_checks_need_no_gpu():
    from seunet_amd import morphometry as M
    for bad in (dict(step=0.0), dict(step=float("inf")), dict(step=-1.0), dict(window=0), dict(window=8), dict(window=2.5),
                dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, 1.0))):
        with pytest.raises(ValueError):
            M.cross_sections(np.zeros((2, 2, 2), np.int32), np.zeros((2, 2, 2), np.uint8), **bad)


def test_workspace_layout_is_the_closed_form():
    """One walk lays the workspace out for the query, the launchers and the layout report (op 18): a record, the point mask (one
    word per 64 voxels in raster order), the counts, the scan's block totals, each aligned to 256 bytes."""
    import ctypes as C
    from seunet_amd import _lib
    lib = _lib.load()
    f = lib.seunet_debug_volume_layout                       # diagnostic export, not in the public header
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t), C.c_int]
    up = lambda v: (v + 255) // 256 * 256
    for shape in ((1, 1, 1), (3, 4, 5), (9, 8, 65), (17, 5, 130), (96, 80, 72), (300, 512, 512)):
        n = shape[0] * shape[1] * shape[2]
        words = (n + 63) // 64
        want = [up(24), up(8 * words), up(4 * words), up(4 * ((words + 1023) // 1024))]
        buf = (C.c_size_t * 32)()
        assert f(18, *shape, buf, 16) == 4
        assert [int(buf[2 * i + 1]) for i in range(4)] == want and [int(buf[2 * i]) for i in range(4)] == [sum(want[:i]) for i in range(4)]
        assert int(lib.seunet_cross_section_workspace_bytes(*shape)) == sum(want)
    assert f(18, 2048, 2048, 512, None, 0) == 0 and int(lib.seunet_cross_section_workspace_bytes(2048, 2048, 512)) == 0
    assert int(lib.seunet_cross_section_workspace_bytes(0, 4, 4)) == 0 and int(lib.seunet_cross_section_sweep_points()) == 8192
