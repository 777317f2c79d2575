"""The airway walls on the GPU (csrc/airway_wall.hip, ``seunet_amd.airway_walls``) against the numpy oracle
tests/airway_wall_oracle.py: ``mask`` and ``codes`` bit for bit, ``edges`` and ``sums`` bit for bit through their int64 views; the
derived float64 columns, which the host forms from the sums, at rtol = 1e-12 (a handful of float64 operations per value, a rounding
bound near 1e-15; the margin covers another order of them).  The inputs are the named cases the host file checks the oracle on
(tests/airway_wall_cases.py) with both CT dtypes, the committed parse fixtures with a CT painted from the label's EDT, and the
smallest shapes that reach every path: extents of 1, no point at all, a number of points that is no multiple of a wave, more points
than one grid sweep (``seunet_airway_wall_sweep_points()``: one wave per point), the ends of ``n_search``, both ``same_label``,
sections given and computed, with and without the per-ray outputs."""
import os

import numpy as np
import pytest
import torch

import airway_wall_cases as wc
import airway_wall_oracle as wo
import cross_section_cases as cc
import cross_section_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12
_GOLDEN = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()               # (a writable copy: the shared volumes are read-only)


def same(got, want, min_rays=32):
    """An ``AirwayWalls`` against the oracle's dict."""
    m = len(want["label"])
    assert len(got) == m and got.ray_step == want["ray_step"] and got.n_search == want["n_search"] and got.step == want["step"]
    assert got.mask.dtype == np.uint64 and got.mask.shape == (m,)
    assert np.array_equal(got.mask, want["mask"]), ("mask", np.flatnonzero(got.mask != want["mask"])[:8])
    assert got.sums.dtype == np.float64 and got.sums.shape == (m, 6)
    assert np.array_equal(got.sums.view(np.int64), want["sums"].view(np.int64)), "sums"
    if got.codes is not None:
        assert got.codes.dtype == np.uint8 and got.codes.shape == (m, 64)
        assert np.array_equal(got.codes, want["codes"]), ("codes", np.argwhere(got.codes != want["codes"])[:8].tolist())
        assert got.edges.dtype == np.float64 and got.edges.shape == (m, 64, 2)
        assert np.array_equal(got.edges.view(np.int64), want["edges"].view(np.int64)), "edges"
    cols = wo.derived(want["mask"], want["sums"], min_rays)
    assert got.rays_valid.dtype == np.int32 and np.array_equal(got.rays_valid, cols["rays_valid"])
    for k in wo.FLOAT_COLUMNS:
        np.testing.assert_allclose(getattr(got, k), cols[k], rtol=RTOL, atol=0, equal_nan=True, err_msg=k)
    assert np.array_equal(got.valid, cols["valid"]) and np.array_equal(got.label, want["label"])


def given(A, sections, spacing, same_label=True):
    """A ``CrossSections`` from the oracle's dict."""
    return A.CrossSections.from_columns(sections["coord"], sections["label"], sections["support"], sections["tangent"], sections["count"],
                                        sections["moments"], sections["rim"], sections["step"], None, spacing, 4, same_label)


def check_case(A, name, as_float=False, return_rays=True, **over):
    c, want = wc.case(name), wc.want(name, **over)
    ct = c["ct"].astype(np.float32) if as_float else c["ct"]
    got = A.airway_walls(dev(ct), dev(c["parsing"]), None, c["spacing"], sections=given(A, wc.sections(name), c["spacing"], c["same_label"]),
                         return_rays=return_rays, **dict(c["kw"], **over))
    same(got, want)
    return got


# ---- the named cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("name", wc.NAMED)
def test_named_cases(A, name, as_float):
    got = check_case(A, name, as_float)
    assert got.same_label == wc.case(name)["same_label"] and got.codes is not None


@pytest.mark.parametrize("name", ["tube:oblique", "two_lumina:", "noise:"])
def test_sections_computed_on_the_device(A, name):
    """``sections=None``: the sections come from the skeleton and their device buffer is used where it lies."""
    c = wc.case(name)
    got = A.airway_walls(dev(c["ct"]), dev(c["parsing"]), dev(c["skeleton"]), c["spacing"], return_rays=True)
    same(got, wc.want(name))
    assert np.array_equal(got.coord, wc.sections(name)["coord"])


@pytest.mark.parametrize("name", ["blob:1", "noise:any"])
def test_without_the_rays(A, name):
    """``return_rays=False`` gives the same mask and sums and no per-ray output."""
    got = check_case(A, name, return_rays=False)
    assert got.codes is None and got.edges is None


def test_numpy_in_and_defaults(A):
    c = wc.case("noise:")
    got = A.airway_walls(np.array(c["ct"]), np.array(c["parsing"]), np.array(c["skeleton"]), c["spacing"])
    same(got, wc.want("noise:"))
    assert got.ray_step == 0.35 and got.n_search == 10 and got.min_contrast == 100.0 and got.min_rays == 32 and got.spacing == wc.ANISO


@pytest.mark.parametrize("n_search, max_wall", [(1, 0.35), (31, 10.8)])
def test_n_search_ends(A, n_search, max_wall):
    for name in ("noise:", "tube:1"):
        got = check_case(A, name, max_wall=max_wall)
        assert got.n_search == n_search


def test_other_parameters(A):
    check_case(A, "tube:2", ray_step=0.25, max_wall=3.0)
    check_case(A, "noise:", min_contrast=1.0)
    check_case(A, "noise_f32:", as_float=True, min_contrast=700.5, ray_step=0.5)
    c, want = wc.case("noise:"), wc.want("noise:")
    got = A.airway_walls(dev(c["ct"]), dev(c["parsing"]), dev(c["skeleton"]), c["spacing"], min_rays=5)
    same(got, want, min_rays=5)
    assert got.valid.sum() > (wo.derived(want["mask"], want["sums"], 32)["valid"]).sum()


# ---- the committed parse fixtures, the CT painted from the label's EDT ------------------------------------------------------------
def golden(case):
    if case not in _GOLDEN:
        from scipy import ndimage
        z = np.load(os.path.join(ROOT, "tests", "golden", "parse_known.npz"))
        parsing, skeleton = z[f"case{case}_parsing"].astype(np.int32), np.ascontiguousarray(z[f"case{case}_skeleton"])
        away = ndimage.distance_transform_edt(parsing == 0, sampling=wc.ANISO)
        ct = np.where(parsing != 0, wc.LUMEN, np.where(away <= 1.5, wc.WALL, wc.PARENCHYMA)).astype(np.int16)
        sections = co.cross_sections(parsing, skeleton, spacing=wc.ANISO)
        _GOLDEN[case] = cc.frozen(ct, parsing, skeleton) + (sections, wo.airway_walls(ct, parsing, sections, wc.directions(), wc.ANISO))
    return _GOLDEN[case]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_parse_fixtures(A, case):
    ct, parsing, skeleton, sections, want = golden(case)
    got = A.airway_walls(dev(ct), dev(parsing), dev(skeleton), wc.ANISO, return_rays=True)
    same(got, want)
    assert len(got) > 100 and (got.codes == 0).sum() > 100


# ---- edge shapes ----------------------------------------------------------------------------------------------------------------
def check_volume(A, ct, parsing, skeleton, spacing=wc.ANISO, **kw):
    sections = co.cross_sections(parsing, skeleton, spacing=spacing)
    want = wo.airway_walls(ct, parsing, sections, wc.directions(), spacing, **kw)
    got = A.airway_walls(dev(ct), dev(parsing), dev(skeleton), spacing, return_rays=True, **kw)
    same(got, want)
    return got


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 40), (1, 30, 1), (20, 1, 1), (1, 9, 11), (7, 1, 66)])
def test_extents_of_one(A, shape):
    """No sample has its eight corners in the volume: every ray is empty."""
    rng = np.random.default_rng(sum(shape))
    parsing = rng.integers(0, 3, shape).astype(np.int32)
    parsing[rng.random(shape) < 0.5] = 1
    skeleton = (rng.random(shape) < 0.7).astype(np.uint8)
    skeleton[0, 0, 0] = parsing[0, 0, 0] = 1
    got = check_volume(A, wc.noise_ct(shape), parsing, skeleton)
    assert len(got) >= 1 and not got.mask.any() and set(np.unique(got.codes)) <= {1, 6}


def test_no_points_and_an_empty_volume(A):
    c = wc.case("noise:")
    got = check_volume(A, c["ct"], c["parsing"], np.zeros(c["parsing"].shape, np.uint8))
    assert len(got) == 0 and got.mask.shape == (0,) and got.sums.shape == (0, 6) and got.edges.shape == (0, 64, 2)
    assert got.per_branch(3)["wall_sections"].tolist() == [0, 0, 0] and np.isnan(got.pi10()["pi10"])
    empty = A.airway_walls(torch.zeros((0, 4, 4), dtype=torch.int16).cuda(), torch.zeros((0, 4, 4), dtype=torch.int32).cuda(),
                           torch.zeros((0, 4, 4), dtype=torch.uint8).cuda())
    assert len(empty) == 0 and empty.codes is None


def test_point_counts_around_a_wave(A):
    """1, 63, 64, 65 and 130 points: a number of points that is no multiple of 64 or of the 4 waves of a workgroup."""
    for m in (1, 63, 64, 65, 130):
        parsing = np.ones((3, 5, 67), np.int32)
        parsing[:, 0, :] = 0
        inner = np.zeros((3, 4, 67), np.uint8)
        inner.reshape(-1)[np.arange(m) * 7 % inner.size] = 1
        skeleton = np.zeros(parsing.shape, np.uint8)
        skeleton[:, 1:, :] = inner
        got = check_volume(A, wc.noise_ct(parsing.shape, seed=m), parsing, skeleton)
        assert len(got) == m


def test_more_points_than_one_grid_sweep(A):
    """Every voxel of a (21, 20, 20) noise volume is a point: 8400 points against the 8192 waves of the grid, so the first 208
    waves take a second point; 8400 is no multiple of 64."""
    sweep = int(A._lib.load().seunet_airway_wall_sweep_points())
    shape = (21, 20, 20)
    rng = np.random.default_rng(11)
    parsing = rng.integers(1, 4, shape).astype(np.int32)
    assert sweep == 8192 and sweep < parsing.size < 2 * sweep and parsing.size % 64
    got = check_volume(A, wc.noise_ct(shape, seed=12), parsing, np.ones(shape, np.uint8))
    assert len(got) == parsing.size and len(np.unique(got.codes[sweep:])) >= 4      # (label noise without background: no ray is measured)


def test_a_second_call_gives_the_same_bits(A):
    from guarded_alloc import same_bits
    c = wc.case("two_lumina:")
    ct, p, s = dev(c["ct"]), dev(c["parsing"]), dev(c["skeleton"])
    first = A.airway_walls(ct, p, s, c["spacing"], return_rays=True)
    second = A.airway_walls(ct, p, s, c["spacing"], return_rays=True)
    same_bits(first.to_dict(), second.to_dict(), "second call")
    assert torch.equal(ct.cpu(), torch.from_numpy(np.array(c["ct"]))) and torch.equal(p.cpu(), torch.from_numpy(np.array(c["parsing"])))
    assert torch.equal(s.cpu(), torch.from_numpy(np.array(c["skeleton"])))


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(A):
    c = wc.case("noise:")
    ct, p, s = dev(c["ct"]), dev(c["parsing"]), dev(c["skeleton"])
    sections = given(A, wc.sections("noise:"), c["spacing"])
    with pytest.raises(ValueError, match="shape"):
        A.airway_walls(ct[:, :, :-1], p, s)
    with pytest.raises(ValueError, match="shape"):
        A.airway_walls(ct, p, s[:, :, :-1])
    with pytest.raises(TypeError, match="int16 or float32"):
        A.airway_walls(ct.double(), p, s)
    with pytest.raises(TypeError, match="int16 or float32"):
        A.airway_walls(np.array(c["ct"], dtype=np.int32), p, s)
    with pytest.raises(RuntimeError, match="no CPU path"):
        A.airway_walls(ct.cpu(), p, s)
    with pytest.raises(RuntimeError, match="no CPU path"):
        A.airway_walls(ct, p.cpu(), s)
    with pytest.raises(ValueError, match="skeleton"):
        A.airway_walls(ct, p)
    with pytest.raises(TypeError, match="CrossSections"):
        A.airway_walls(ct, p, s, sections={"label": []})
    with pytest.raises(ValueError, match="spacing"):
        A.airway_walls(ct, p, None, (1.0, 1.0, 1.0), sections=sections)
    for bad in (dict(ray_step=0.0), dict(ray_step=float("nan")), dict(max_wall=0.0), dict(max_wall=11.0), dict(max_wall=float("inf")),
                dict(min_contrast=0.0), dict(min_contrast=float("nan")), dict(min_contrast=1e-60), dict(min_rays=0), dict(min_rays=65),
                dict(min_rays=1.5), dict(spacing=(1.0, -1.0, 1.0))):
        with pytest.raises(ValueError):
            A.airway_walls(ct, p, s, **dict(dict(spacing=c["spacing"]), **bad))
    with pytest.raises(TypeError, match="AirwayWalls"):
        A.branch_morphometry(p, s, walls="yes")
    lib = A._lib.load()                                      # the entry point checks what the wrapper cannot pass wrongly
    assert lib.seunet_airway_walls(ct.data_ptr(), 2, p.data_ptr(), *p.shape, 1.0, 1.0, 1.0, 0.5, 0.5, 10, 100.0, 1, 1, 1, 1, 1, 1, None,
                                   None, None) != 0 and "ct_dtype" in A._lib.last_error()
    assert lib.seunet_airway_walls(ct.data_ptr(), 0, p.data_ptr(), *p.shape, 1.0, 1.0, 1.0, 0.5, 0.5, 32, 100.0, 1, 1, 1, 1, 1, 1, None,
                                   None, None) != 0 and "n_search" in A._lib.last_error()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_y_tree_end_to_end(A):
    """A Y of three tubes through skeletonize_3d, tree_parsing, cross_sections and airway_walls into branch_morphometry(walls=).
    The CT is painted from the mask's EDT with a wall 2.0 thick; the trunk, along axis 0, has the in-plane spacing 0.7."""
    from scipy import ndimage
    mask_np = np.array(cc.y_tree())
    away = ndimage.distance_transform_edt(mask_np == 0, sampling=wc.ANISO)
    painted = 2.0
    ct_np = np.where(mask_np != 0, wc.LUMEN, np.where(away <= painted, wc.WALL, wc.PARENCHYMA)).astype(np.int16)
    mask, ct = torch.from_numpy(mask_np).cuda(), torch.from_numpy(ct_np).cuda()
    skeleton = A.skeletonize_3d(mask)
    parsing, num = A.tree_parsing(mask, skeleton, return_num=True)
    assert num >= 3
    sections = A.cross_sections(parsing, skeleton, wc.ANISO)
    walls = A.airway_walls(ct, parsing, None, wc.ANISO, sections=sections, return_rays=True)
    p, s = parsing.cpu().numpy(), skeleton.cpu().numpy()
    want = wo.airway_walls(ct_np, p, co.cross_sections(p, s, spacing=wc.ANISO), wc.directions(), wc.ANISO)
    same(walls, want)
    same(A.airway_walls(ct, parsing, skeleton, wc.ANISO, return_rays=True), want)       # the sections computed: the same bits
    table = A.branch_morphometry(parsing, skeleton, wc.ANISO, walls=walls)
    rows = wo.per_branch(want["label"], wo.derived(want["mask"], want["sums"]), table.num)
    assert np.array_equal(table.wall_sections, rows["wall_sections"]) and table.wall_sections.sum() > 10
    for k in wo.BRANCH_COLUMNS:
        np.testing.assert_allclose(getattr(table, k), rows[k], rtol=RTOL, atol=0, equal_nan=True, err_msg=k)
    # nothing else changes with the keyword, and without it the wall columns stay None and out of to_dict()
    plain = A.branch_morphometry(parsing, skeleton, wc.ANISO)
    for k, v in plain.to_dict().items():
        assert np.array_equal(np.asarray(v), np.asarray(getattr(table, k)), equal_nan=isinstance(v, np.ndarray) and v.dtype.kind == "f"), k
    assert all(getattr(plain, k) is None and k not in plain.to_dict() for k in A.morphometry.WALL_COLUMNS)
    trunk = int(np.argmax(table.voxels))                     # the widest tube holds the most voxels
    print("trunk", trunk + 1, "sections", table.wall_sections[trunk], "median thickness", table.wall_thickness_median[trunk])
    assert table.wall_sections[trunk] >= 3 and abs(table.wall_thickness_median[trunk] - painted) <= 0.7
    fit = walls.pi10((0.0, 100.0))
    assert fit["branches"] == int((table.wall_sections > 0).sum())
