"""The airway cross-sections on the GPU (csrc/cross_section.hip, ``seunet_amd.cross_sections``) against the numpy oracle
tests/cross_section_oracle.py: every integer column bit for bit (``np.array_equal``, dtype included) and the float64 tangents bit
for bit through their integer views; the derived float64 columns, which the host forms from the integer ones, at rtol = 1e-12
(a handful of float64 operations per value, a rounding bound near 1e-15; the margin covers another order of them).  The inputs are
the committed parse fixtures, the synthetic cases the host file checks the oracle on (tests/cross_section_cases.py), label noise,
and the smallest shapes that reach every path: extents of 1, no point at all, a number of points that is no multiple of a wave,
more points than one grid sweep of the section pass (``seunet_cross_section_sweep_points()``: one wave per point), the largest
label, the smallest and largest window."""
import os

import numpy as np
import pytest
import torch

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


def same(got, want):
    """A ``CrossSections`` against the oracle's dict."""
    m = len(want["label"])
    assert len(got) == m and got.step == want["step"]
    for k in co.INT_COLUMNS:
        have = getattr(got, k)
        assert have.dtype == np.int32 and have.shape == want[k].shape, k
        assert np.array_equal(have, want[k]), (k, np.flatnonzero((have != want[k]).reshape(m, -1).any(axis=1))[:8])
    assert got.tangent.dtype == np.float64 and got.tangent.shape == (m, 3)
    assert np.array_equal(got.tangent.view(np.int64), want["tangent"].view(np.int64)), "tangent"
    derived = co.derived(want["count"], want["moments"], want["rim"], want["step"])
    for k in co.FLOAT_COLUMNS:
        np.testing.assert_allclose(getattr(got, k), derived[k], rtol=RTOL, atol=0, equal_nan=True, err_msg=k)
    assert np.array_equal(got.valid, derived["valid"])


def check(A, parsing, skeleton, **kw):
    """cross_sections on device tensors against the oracle; returns the GPU result."""
    want = co.cross_sections(parsing, skeleton, **kw)
    assert want["status"] == 0
    got = A.cross_sections(torch.from_numpy(np.array(parsing)).cuda(), torch.from_numpy(np.array(skeleton)).cuda(), **kw)
    same(got, want)
    return got


# ---- the committed parse fixtures ---------------------------------------------------------------------------------------------
def golden(case, key):
    if (case, key) not in _GOLDEN:
        z = np.load(os.path.join(ROOT, "tests", "golden", "parse_known.npz"))
        _GOLDEN[(case, key)] = cc.frozen(z[f"case{case}_{key}"].astype(np.int32), np.ascontiguousarray(z[f"case{case}_skeleton"]))
    return _GOLDEN[(case, key)]


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), cc.ANISO])
@pytest.mark.parametrize("key", ["parsing0", "parsing"])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_parse_fixtures(A, case, key, spacing):
    parsing, skeleton = golden(case, key)
    got = check(A, parsing, skeleton, spacing=spacing)
    assert len(got) > 100 and got.valid.sum() > 100


# ---- the synthetic cases of the host file ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.SYNTHETIC)
def test_synthetic_cases(A, name):
    parsing, skeleton, kw = cc.case(name)
    check(A, parsing, skeleton, **kw)


def test_numpy_in_and_defaults(A):
    parsing, skeleton, kw = cc.case("noise:")
    got = A.cross_sections(np.array(parsing), np.array(skeleton), **kw)      # (writable copies: the shared volumes are read-only)
    same(got, co.cross_sections(parsing, skeleton, **kw))
    assert got.step == 0.35 and got.window == 4 and got.same_label is True and got.num == 3 and got.spacing == cc.ANISO


# ---- edge shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 40), (1, 30, 1), (20, 1, 1), (1, 9, 11), (7, 1, 66)])
def test_extents_of_one(A, shape):
    rng = np.random.default_rng(sum(shape))
    parsing = rng.integers(0, 3, shape).astype(np.int32)
    parsing[rng.random(shape) < 0.5] = 1
    skeleton = (rng.random(shape) < 0.7).astype(np.uint8)
    skeleton[0, 0, 0] = parsing[0, 0, 0] = 1
    check(A, parsing, skeleton, spacing=cc.ANISO)


def test_no_points_and_an_empty_volume(A):
    parsing, _, _ = cc.case("noise:")
    got = check(A, parsing, np.zeros(parsing.shape, np.uint8))                   # a skeleton without voxels
    assert len(got) == 0 and got.coord.shape == (0, 3) and got.moments.shape == (0, 5) and got.area.shape == (0,)
    got = check(A, np.zeros(parsing.shape, np.int32), np.ones(parsing.shape, np.uint8))      # a skeleton without labels
    assert len(got) == 0
    got = A.cross_sections(torch.zeros((0, 4, 4), dtype=torch.int32).cuda(), torch.zeros((0, 4, 4), dtype=torch.uint8).cuda(), num=3)
    assert len(got) == 0 and got.tangent.shape == (0, 3)
    assert got.per_branch()["section_count"].tolist() == [0, 0, 0]


def test_point_counts_around_a_wave(A):
    """1, 63, 64, 65 and 130 points: a number of points that is no multiple of 64, of 4 waves, or of a word of the point mask."""
    for m in (1, 63, 64, 65, 130):
        parsing = np.ones((3, 5, 67), np.int32)
        skeleton = np.zeros(parsing.shape, np.uint8)
        skeleton.reshape(-1)[np.arange(m) * 7 % skeleton.size] = 1
        assert len(check(A, parsing, skeleton)) == m


def test_more_points_than_one_grid_sweep(A):
    """Every voxel of a (21, 20, 20) noise volume is a point: 8400 points against the 8192 waves of the section pass's grid, so
    the first 208 waves take a second point; 8400 is no multiple of 64."""
    sweep = int(A._lib.load().seunet_cross_section_sweep_points())
    shape = (21, 20, 20)
    rng = np.random.default_rng(11)
    parsing = rng.integers(1, 4, shape).astype(np.int32)
    assert sweep == 8192 and sweep < parsing.size < 2 * sweep and parsing.size % 64
    got = check(A, parsing, np.ones(shape, np.uint8), spacing=cc.ANISO)
    assert len(got) == parsing.size


def test_the_largest_label(A):
    cap = int(A._lib.load().seunet_label_stats_max_num())
    assert cap == 4095
    parsing, skeleton, kw = cc.case("noise:")
    parsing = np.where(parsing == 2, cap, parsing).astype(np.int32)
    got = check(A, parsing, skeleton, num=cap, **kw)
    assert (got.label == cap).sum() > 100 and got.num == cap


@pytest.mark.parametrize("window", [1, 7])
def test_window_ends(A, window):
    parsing, skeleton, kw = cc.case("noise:")
    check(A, parsing, skeleton, window=window, **kw)
    parsing, skeleton = golden(2, "parsing")
    check(A, parsing, skeleton, window=window)


def test_a_second_call_gives_the_same_bits(A):
    from guarded_alloc import same_bits
    parsing, skeleton = golden(1, "parsing")
    p, s = torch.from_numpy(np.array(parsing)).cuda(), torch.from_numpy(np.array(skeleton)).cuda()
    first = A.cross_sections(p, s, cc.ANISO)
    second = A.cross_sections(p, s, cc.ANISO)
    same_bits(first.to_dict(), second.to_dict(), "second call")
    assert torch.equal(p.cpu(), torch.from_numpy(np.array(parsing))) and torch.equal(s.cpu(), torch.from_numpy(np.array(skeleton)))


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(A):
    parsing, skeleton, kw = cc.case("noise:")
    p, s = torch.from_numpy(np.array(parsing)).cuda(), torch.from_numpy(np.array(skeleton)).cuda()
    with pytest.raises(ValueError, match="outside 0..2"):
        A.cross_sections(p, s, num=2)
    with pytest.raises(ValueError, match="outside 0..2"):                        # also where no skeleton voxel carries the label
        A.cross_sections(p, torch.zeros_like(s), num=2)
    negative = p.clone()
    negative[3, 3, 3] = -1
    with pytest.raises(ValueError, match="outside 0..3"):
        A.cross_sections(negative, s)
    cap = int(A._lib.load().seunet_label_stats_max_num())
    with pytest.raises(ValueError, match=str(cap)):
        A.cross_sections(p, s, num=cap + 1)
    with pytest.raises(ValueError, match="shape"):
        A.cross_sections(p, s[:, :, :-1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        A.cross_sections(p.cpu(), s)
    with pytest.raises(RuntimeError, match="no CPU path"):
        A.cross_sections(p, s.cpu())
    for bad in (dict(step=0.0), dict(step=float("nan")), dict(window=0), dict(window=8), dict(spacing=(1.0, -1.0, 1.0))):
        with pytest.raises(ValueError):
            A.cross_sections(p, s, **bad)
    with pytest.raises(TypeError):
        A.branch_morphometry(p, s, cross_sections="yes")


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_y_tree_end_to_end(A):
    """A Y of three tubes through skeletonize_3d, tree_parsing and branch_morphometry(cross_sections=True)."""
    mask = torch.from_numpy(np.array(cc.y_tree())).cuda()
    skeleton = A.skeletonize_3d(mask)
    parsing, num = A.tree_parsing(mask, skeleton, return_num=True)
    assert num >= 3
    table = A.branch_morphometry(parsing, skeleton, cc.ANISO, cross_sections=True)
    p, s = parsing.cpu().numpy(), skeleton.cpu().numpy()
    want = co.cross_sections(p, s, spacing=cc.ANISO)
    cols = co.derived(want["count"], want["moments"], want["rim"], want["step"])
    rows = co.per_branch(want["label"], cols, table.num)
    assert np.array_equal(table.section_count, rows["section_count"]) and table.section_count.sum() > 20
    for k in co.BRANCH_COLUMNS:
        np.testing.assert_allclose(getattr(table, k), rows[k], rtol=RTOL, atol=0, equal_nan=True, err_msg=k)
    # the same table from a CrossSections made beforehand, and nothing else changes with the keyword
    sections = A.cross_sections(parsing, skeleton, cc.ANISO)
    same(sections, want)
    given = A.branch_morphometry(parsing, skeleton, cc.ANISO, cross_sections=sections)
    plain = A.branch_morphometry(parsing, skeleton, cc.ANISO)
    for k, v in plain.to_dict().items():
        assert np.array_equal(np.asarray(v), np.asarray(getattr(given, k)), equal_nan=isinstance(v, np.ndarray) and v.dtype.kind == "f"), k
    for k in ("section_count",) + co.BRANCH_COLUMNS:
        assert getattr(plain, k) is None and np.array_equal(getattr(given, k), getattr(table, k), equal_nan=True), k
    # the trunk, of radius 4 voxels along axis 0, is the widest branch: its median area is pi r^2 under the in-plane spacing to 10 %
    # (the CPU oracles of the three steps give 24.01 against 24.63)
    trunk = int(np.nanargmax(table.area_median))
    assert abs(table.area_median[trunk] - np.pi * 16 * 0.7 * 0.7) < 0.1 * np.pi * 16 * 0.7 * 0.7
