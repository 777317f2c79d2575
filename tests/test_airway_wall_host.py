"""The airway-wall oracle (tests/airway_wall_oracle.py) against known answers, the committed direction table, and the host side of
``seunet_amd.morphometry`` (the derived columns, the per-branch aggregation, Pi10); no GPU.  tests/test_airway_wall_gpu.py then
holds the device to the oracle bit for bit on these same inputs (tests/airway_wall_cases.py)."""
import importlib.util
import math
import os

import numpy as np
import pytest

import airway_wall_cases as wc
import airway_wall_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import seunet_amd
    return seunet_amd.morphometry


# ---- the direction table ----------------------------------------------------------------------------------------------------------
def test_host_entry_points():
    import seunet_amd
    lib = seunet_amd._lib.load()
    assert lib.seunet_airway_wall_rays() == 64 and lib.seunet_airway_wall_samples() == 64
    assert lib.seunet_airway_wall_sweep_points() == 8192
    assert lib.seunet_airway_wall_directions(None) != 0 and "null" in seunet_amd._lib.last_error()


def test_direction_table():
    d = wc.directions()
    assert d.shape == (64, 2) and d.dtype == np.float64
    for r in range(64):
        # math.cos / math.sin of the angle folded into the first octant: the float64 nearest to 2 pi r / 64 is up to 4e-16 from it
        # for r near 32 or 64, which alone moves its cosine or sine by more than 2^-52; the folded angle is below 0.79 and within
        # 1.2e-16 of the true one, so the reference itself is good to well under 2^-52
        q = r % 16 if r % 16 <= 8 else 16 - r % 16
        c, s = math.cos(math.pi * q / 32.0), math.sin(math.pi * q / 32.0)
        if r % 16 > 8:
            c, s = s, c
        quadrant = r // 16                                   # a turn by 90 degrees: (c, s) -> (-s, c)
        for _ in range(quadrant):
            c, s = -s, c
        assert abs(d[r, 0] - c) <= 2.0 ** -52 and abs(d[r, 1] - s) <= 2.0 ** -52, r
        assert abs(math.hypot(d[r, 0], d[r, 1]) - 1.0) <= 1e-15, r
    for r in range(32):                                      # r and r + 32 are exact negatives
        assert d[r + 32, 0] == -d[r, 0] and d[r + 32, 1] == -d[r, 1], r
    for r in range(17):                                      # r and 16 - r swap components exactly
        assert d[r, 0] == d[16 - r, 1] and d[r, 1] == d[16 - r, 0], r
    for r in range(1, 32):                                   # r and 32 - r mirror in the second axis
        assert d[32 - r, 0] == -d[r, 0] and d[32 - r, 1] == d[r, 1], r


def test_generator_reproduces_the_header():
    spec = importlib.util.spec_from_file_location("gen_wall_table", os.path.join(ROOT, "scripts", "gen_wall_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(gen.HEADER).read() == gen.render()
    assert np.array_equal(np.array(gen.directions(), dtype=np.float64).view(np.int64), wc.directions().view(np.int64))


# ---- the cases reach what they are named for -----------------------------------------------------------------------------------
def test_cases_reach_every_code_and_path():
    codes = np.zeros(7, np.int64)
    kb1 = short = end = tie = 0
    for name in wc.NAMED:
        w = wc.want(name)
        codes += np.bincount(w["codes"].reshape(-1), minlength=7)
        kb1 += int((w["kb"] == 1).sum())
        short += int(((w["L"] >= 0) & (w["L"] < 64)).sum())
        end += int(((w["kp"] >= 0) & (w["kp"] == w["hi"]) & (w["codes"] == 2)).sum())
        tie += int(w["tie"].sum())
    assert (codes > 0).all(), codes.tolist()
    assert kb1 > 0 and short > 0 and end > 0 and tie > 0
    # what the named cases are made for
    assert (wc.want("crescent:")["codes"] == 1).all()                          # the centroid lies outside the lumen
    assert (wc.want("flat:")["codes"] == 3).all() and wc.want("flat:")["tie"].all()
    assert not (wc.want("thick:")["codes"] == 0).any()                         # no outer edge within max_wall
    assert (wc.want("two_lumina:")["codes"] == 4).sum() >= 100                  # the rays towards the other lumen
    for axis in ("0", "1", "2", "oblique"):                                    # the blob takes rays from its side only
        plain, blob = wc.want(f"tube:{axis}")["codes"], wc.want(f"blob:{axis}")["codes"]
        assert 0 < ((plain == 0) & (blob != 0)).sum() <= 8
    assert (wc.want("border:")["codes"] != 0).sum() >= 20


def test_int16_and_its_float32_copy_agree():
    c = wc.case("noise:")
    as_float = wo.airway_walls(c["ct"].astype(np.float32), c["parsing"], wc.sections("noise:"), wc.directions(), spacing=c["spacing"])
    w = wc.want("noise:")
    for k in ("mask", "codes"):
        assert np.array_equal(as_float[k], w[k])
    for k in ("edges", "sums"):
        assert np.array_equal(as_float[k].view(np.int64), w[k].view(np.int64))


# ---- the plain tube: R = 4.0, T = 2.0, in-plane spacing 0.7, dr = 0.35 ---------------------------------------------------------
def test_plain_tube_edges_and_wall_area():
    """Every edge within half the in-plane spacing of the true one: the bound that trilinear interpolation of an area-weighted edge
    gives (measured: 0.19 and 0.17 at most)."""
    w = wc.want("tube:0")
    assert w["ray_step"] == 0.35 and w["n_search"] == 10
    interior = slice(1, -1)
    codes, edges = w["codes"][interior], w["edges"][interior]
    assert codes.shape[0] >= 8 and (codes == 0).all()
    assert np.abs(edges[..., 0] - wc.R).max() <= 0.35 and np.abs(edges[..., 1] - (wc.R + wc.T)).max() <= 0.35
    cols = wo.derived(w["mask"], w["sums"])
    true = 100.0 * (1.0 - wc.R ** 2 / (wc.R + wc.T) ** 2)
    assert np.abs(cols["wall_area_percent"][interior] - true).max() <= 0.05 * true
    assert np.abs(cols["wall_thickness"][interior] - wc.T).max() <= 0.35


@pytest.mark.parametrize("name", wc.TUBES[1:])
def test_other_tubes(name):
    w = wc.want(name)
    full = (w["codes"] == 0).all(axis=1)
    assert full.sum() >= 8
    edges = w["edges"][full]
    assert np.abs(edges[..., 0] - wc.R).max() <= 0.35 and np.abs(edges[..., 1] - (wc.R + wc.T)).max() <= 0.35


def test_a_shift_of_the_ct_moves_no_edge():
    """data_cut's + 1024 changes no code and moves an edge only by the float32 rounding of the profile: a few ulp of 2048 (2.4e-4 HU)
    on crossing segments that span hundreds of HU per sample, so far below 1e-4 of the spacing's unit."""
    c = wc.case("tube:0")
    moved = wo.airway_walls(c["ct"] + np.int16(1024), c["parsing"], wc.sections("tube:0"), wc.directions(), spacing=c["spacing"])
    w = wc.want("tube:0")
    assert np.array_equal(moved["codes"], w["codes"])
    assert np.abs(moved["edges"] - w["edges"]).max() <= 1e-4


def test_butterfly_and_n_search():
    x = np.random.default_rng(0).random((3, 64))
    t = x.copy()
    for level in range(6):
        t = t + t[:, np.arange(64) ^ (1 << level)]
    assert np.array_equal(wo.butterfly(x), t[:, 0])
    assert wo.n_search(0.35, 3.5) == 10 and wo.n_search(0.35, 3.6) == 11 and wo.n_search(1.0, 1.0) == 1 and wo.n_search(0.1, 0.3) == 3


# ---- the host side of the package -----------------------------------------------------------------------------------------------
def test_derived_columns_and_per_branch(M):
    w = wc.want("noise:any")
    got = M.AirwayWalls.from_columns(wc.sections("noise:any")["coord"], w["label"], w["mask"], w["sums"], num=3, min_rays=8)
    cols = wo.derived(w["mask"], w["sums"], 8)
    assert np.array_equal(got.rays_valid, cols["rays_valid"]) and np.array_equal(got.valid, cols["valid"]) and got.valid.sum() > 10
    for k in wo.FLOAT_COLUMNS:
        np.testing.assert_allclose(getattr(got, k), cols[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    rows, have = wo.per_branch(w["label"], cols, 3), got.per_branch()
    assert np.array_equal(have["wall_sections"], rows["wall_sections"]) and have["wall_sections"].sum() == got.valid.sum()
    for k in wo.BRANCH_COLUMNS:
        np.testing.assert_allclose(have[k], rows[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    assert got.per_branch(5)["wall_sections"].tolist()[3:] == [0, 0]


def synthetic_walls(M, radii, intercept, slope, rows=5):
    """Branches whose walls lie exactly on sqrt(wall_area) = intercept + slope * inner_perimeter."""
    label = np.repeat(np.arange(1, len(radii) + 1), rows).astype(np.int32)
    r = np.repeat(np.asarray(radii, dtype=np.float64), rows)
    big = np.sqrt(r * r + (intercept + slope * 2.0 * np.pi * r) ** 2 / np.pi)
    sums = np.stack([64 * r, 64 * big, 64 * r * r, 64 * big * big, 64 * (big - r), np.zeros_like(r)], axis=1)
    return M.AirwayWalls.from_columns(np.zeros((label.size, 3), np.int32), label, np.full(label.size, 2 ** 64 - 1, np.uint64), sums)


def test_pi10(M):
    walls = synthetic_walls(M, [1.0, 1.5, 2.0, 2.5, 3.0, 0.5, 4.0], 1.2, 0.25)
    fit = walls.pi10()
    assert fit["branches"] == 5                              # perimeters 3.1 and 25.1 lie outside 6 .. 20
    assert abs(fit["intercept"] - 1.2) < 1e-9 and abs(fit["slope"] - 0.25) < 1e-9 and abs(fit["pi10"] - 3.7) < 1e-9
    assert walls.pi10((0.0, 100.0))["branches"] == 7
    one = walls.pi10((6.0, 7.0))
    assert one["branches"] == 1 and math.isnan(one["pi10"])
    assert math.isnan(synthetic_walls(M, [], 1.0, 1.0).pi10()["pi10"])


def test_parameter_errors_without_a_gpu(M):
    assert M.wall_search(0.35, 3.5) == 10 and M.wall_search(0.1, 3.1) == 31
    for ray_step, max_wall in ((0.1, 3.2), (0.0, 1.0), (1.0, 0.0), (float("nan"), 1.0), (1.0, float("inf")), (1e-9, 1.0)):
        with pytest.raises(ValueError):
            M.wall_search(ray_step, max_wall)
    with pytest.raises(ValueError, match="min_rays"):
        M.AirwayWalls.from_columns(np.zeros((0, 3)), [], [], np.zeros((0, 6)), min_rays=65)
    with pytest.raises(ValueError, match="min_rays"):
        M.AirwayWalls.from_columns(np.zeros((0, 3)), [], [], np.zeros((0, 6)), min_rays=0)
