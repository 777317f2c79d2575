"""The host side of the surface distances, without a GPU:

* tests/surface_oracle.py against scipy where it is installed: the border is ``M & ~binary_erosion(M)`` with the 6-neighbour
  cross, and the distances are ``distance_transform_edt(~border, sampling=s)`` read at the other border, bit for bit, on the cases
  the GPU tests use (``case`` below makes them once and keeps them);
* the percentile restatement equals ``np.percentile`` bit for bit, in the oracle and in ``seunet_amd.postprocess``;
* the distances of masks embedded in a larger volume equal those of the crop to the bounding box of ``A | B`` (what the emit pass
  relies on);
* the two workspace layouts (ops 13 and 14 of ``seunet_debug_volume_layout``) tile their workspaces, with closed-form byte counts;
* the error paths of the new entry points that return before any device work."""
import ctypes as C

import numpy as np
import pytest

import surface_oracle as so

ANISO = (1.25, 0.7, 0.7)
UNIT = (1.0, 1.0, 1.0)
_CASES = {}


def _random_pair(shape, density, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < density).astype(np.uint8), (rng.random(shape) < density).astype(np.uint8)


def _boxed():
    """Masks inside (24, 40, 200), non-empty only in boxes that start at 67 and 70 along axis 2: a box not aligned to words."""
    rng = np.random.default_rng(2467)
    a, b = np.zeros((24, 40, 200), np.uint8), np.zeros((24, 40, 200), np.uint8)
    a[1:23, 2:38, 67:131] = rng.random((22, 36, 64)) < 0.8
    b[0:24, 1:39, 70:140] = rng.random((24, 38, 70)) < 0.8
    return a, b


def _whole_against_one():
    a, b = np.ones((5, 6, 70), np.uint8), np.zeros((5, 6, 70), np.uint8)
    b[2, 3, 65] = 1
    return a, b


def _same():
    a, _ = _random_pair((6, 7, 66), 0.5, 66)
    return a, a.copy()


# name -> (maker of (a, b), spacing)
CASES = {
    "tail_3x4x130": (lambda: _random_pair((3, 4, 130), 0.5, 130), ANISO),             # rows of 3 words, 2-bit tail
    # 1200 words: the scan crosses a block (the block scan only; the chunk loop of the top scan: tests/test_volume_large_gpu.py)
    "flat_40x30x1": (lambda: _random_pair((40, 30, 1), 0.6, 4030), ANISO),
    "line_1x9x70": (lambda: _random_pair((1, 9, 70), 0.5, 1970), ANISO),
    "line_9x1x70": (lambda: _random_pair((9, 1, 70), 0.5, 9170), ANISO),
    "dense_20x20x70": (lambda: _random_pair((20, 20, 70), 0.8, 8070), UNIT),          # 35 534 distances, 3 distinct: ties
    "sparse_20x20x70": (lambda: _random_pair((20, 20, 70), 0.02, 270), ANISO),        # many distinct distances
    "boxed_24x40x200": (_boxed, ANISO),
    "whole_against_one": (_whole_against_one, ANISO),
    "same": (_same, ANISO),
}
SMALL = ["tail_3x4x130", "flat_40x30x1", "line_1x9x70", "line_9x1x70", "whole_against_one", "same"]


def case(name):
    """(a, b, spacing, D, n_a, n_b, voxels) of a named case; the oracle runs once per process."""
    if name not in _CASES:
        make, spacing = CASES[name]
        a, b = make()
        _CASES[name] = (a, b, spacing) + so.surface_distances(a, b, spacing)
    return _CASES[name]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ---- the oracle against scipy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_border_and_distances_equal_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    a, b, spacing, D, n_a, n_b, voxels = case(name)
    cross = ndimage.generate_binary_structure(3, 1)
    borders = []
    for m in (a, b):
        m = m != 0
        want = m & ~ndimage.binary_erosion(m, cross)
        assert np.array_equal(so.border(m), want)
        borders.append(want)
    d_ab = ndimage.distance_transform_edt(~borders[1], sampling=spacing)[borders[0]]
    d_ba = ndimage.distance_transform_edt(~borders[0], sampling=spacing)[borders[1]]
    assert (n_a, n_b) == (d_ab.size, d_ba.size)
    assert np.array_equal(bits(D), bits(np.concatenate([d_ab, d_ba])))
    assert np.array_equal(voxels, np.concatenate([np.flatnonzero(borders[0]), np.flatnonzero(borders[1])]))


def test_cases_have_the_properties_they_guard():
    a, b, _, D, n_a, n_b, _ = case("dense_20x20x70")
    assert (n_a, n_b, np.unique(D).size) == (17771, 17763, 3)                     # massive ties, many workgroups
    assert np.unique(case("sparse_20x20x70")[3]).size > 40
    a, b, _, D, n_a, n_b, _ = case("boxed_24x40x200")
    k = np.flatnonzero((a | b).any(axis=(0, 1)))
    assert (k[0], k[-1] + 1) == (67, 140) and (n_a, n_b, np.unique(D).size) == (31815, 39893, 53)
    a, b, _, D, n_a, n_b, _ = case("whole_against_one")
    assert n_b == 1 and n_a == a.size - 3 * 4 * 68                                # the shell of the volume
    assert not case("same")[3].any()
    assert case("flat_40x30x1")[0].size > 1024


# ---- the percentile -------------------------------------------------------------------------------------------------------------
def test_percentile_restatement_equals_numpy():
    from seunet_amd import postprocess as P
    rng = np.random.default_rng(5)
    for n in list(range(1, 60)) + [1000, 4097]:
        for ties in (False, True):
            x = rng.random(n) * 40.0
            if ties:
                x = np.round(x)
            srt = np.sort(x)
            for q in (0, 2.5, 50, 95, 99, 100):
                want = np.percentile(x, q)
                assert bits(so.percentile(x, q)) == bits(want), (n, q, ties)
                lo, hi, g = P._percentile_ranks(n, q)
                assert 0 <= lo <= hi <= n - 1
                assert bits(P._percentile_lerp(srt[lo], srt[hi], g)) == bits(want), (n, q, ties)


# ---- the box --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", [UNIT, ANISO])
def test_distances_of_the_crop_equal_those_of_the_embedded_masks(spacing):
    rng = np.random.default_rng(17)
    ran = 0
    for trial in range(4):
        inner = tuple(int(v) for v in rng.integers(2, 7, 3))
        lo = tuple(int(v) for v in rng.integers(0, 4, 3))
        outer = tuple(l + n + int(p) for l, n, p in zip(lo, inner, rng.integers(0, 4, 3)))
        a, b = np.zeros(outer, np.uint8), np.zeros(outer, np.uint8)
        sel = tuple(slice(l, l + n) for l, n in zip(lo, inner))
        a[sel] = rng.random(inner) < 0.6
        b[sel] = rng.random(inner) < 0.6
        if not (a.any() and b.any()):
            continue
        union = np.argwhere(a | b)
        box = tuple(slice(int(l), int(h) + 1) for l, h in zip(union.min(axis=0), union.max(axis=0)))
        full, crop = so.surface_distances(a, b, spacing), so.surface_distances(a[box], b[box], spacing)
        assert full[1:3] == crop[1:3] and np.array_equal(bits(full[0]), bits(crop[0])), (trial, spacing)
        ran += 1
    assert ran >= 3                                                # a draw with an empty mask is passed over


# ---- the library's host side ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    _lib.load()
    return _lib


def up(v, a=256):
    return (v + a - 1) // a * a


SHAPES = [(1, 1, 1), (3, 4, 130), (40, 30, 1), (20, 20, 70), (24, 40, 200), (300, 512, 512)]


def layout(L, op, s):
    f = L.load().seunet_debug_volume_layout                  # diagnostic export, not in the public header
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t), C.c_int]
    buf = (C.c_size_t * 32)()
    count = f(op, s[0], s[1], s[2], buf, 16)
    return count, [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(max(count, 0))]


def tiles(spans, total):
    at = 0
    for off, nbytes in spans:
        assert off == at and off % 256 == 0
        at += nbytes
    assert at == total


@pytest.mark.parametrize("s", SHAPES)
def test_count_workspace_layout(L, s):
    lib = L.load()
    words = s[0] * s[1] * ((s[2] + 63) // 64)
    blocks = (words + 1023) // 1024
    want = [up(40)] + [up(8 * words)] * 4 + [up(4 * words)] * 2 + [up(4 * blocks)] * 2
    count, spans = layout(L, 13, s)
    assert count == 9 and [b for _, b in spans] == want
    total = lib.seunet_surface_workspace_bytes(*s)
    assert total == 256 + 4 * up(8 * words) + 2 * up(4 * words) + 2 * up(4 * blocks)
    tiles(spans, total)


@pytest.mark.parametrize("s", SHAPES)
def test_emit_workspace_layout(L, s):
    lib = L.load()
    n = s[0] * s[1] * s[2]
    count, spans = layout(L, 14, s)
    assert count == 3 and [b for _, b in spans] == [up(n), up(4 * n), 4 * up(2 * n)]
    total = lib.seunet_surface_emit_workspace_bytes(*s)
    assert total == up(n) + up(4 * n) + lib.seunet_edt_sampling_workspace_bytes(*s)       # 13 bytes per voxel of the box
    tiles(spans, total)


def test_small_byte_counts(L):
    lib = L.load()
    for ntol in range(9):
        assert lib.seunet_surface_summary_bytes(ntol) == 8 * (2 * (3 + ntol) + 2 * 128 * (2 + ntol))
    for k in range(1, 9):
        assert lib.seunet_select_ranks_workspace_bytes(k) == 256 + up(4 * 256 * k)
    assert layout(L, 13, (2048, 2048, 512))[0] == 0 and layout(L, 14, (2048, 2048, 512))[0] == 0


def test_queries_reject_bad_arguments(L):
    lib = L.load()
    for f in (lib.seunet_surface_workspace_bytes, lib.seunet_surface_emit_workspace_bytes):
        for bad, word in (((0, 4, 4), "bad extents"), ((4, -1, 4), "bad extents"), ((32768, 1, 1), "32767"), ((2048, 2048, 512), "2^31")):
            assert f(*bad) == 0 and word in L.last_error(), (bad, L.last_error())
    for ntol in (-1, 9):
        assert lib.seunet_surface_summary_bytes(ntol) == 0 and "tolerances" in L.last_error()
    for k in (0, 9):
        assert lib.seunet_select_ranks_workspace_bytes(k) == 0 and "requests" in L.last_error()


def test_calls_reject_bad_arguments_before_any_device_work(L):
    """Null pointers, bad extents, bad spacing, bad boxes and more than 8 tolerances or requests: each returns non-zero with a
    message, from checks that precede every device call (the pointers below are never dereferenced)."""
    lib = L.load()
    p = 4096                                                       # a non-null stand-in for a device pointer
    n_a, n_b, box = C.c_longlong(0), C.c_longlong(0), (C.c_int * 6)(0, 4, 0, 4, 0, 4)
    count = lambda a=p, b=p, s=(4, 4, 4), na=C.byref(n_a), bx=box, ws=p: lib.seunet_surface_count(a, b, *s, na, C.byref(n_b), bx, ws, 1 << 20, None)
    assert count(a=None) != 0 and "null" in L.last_error()
    assert count(ws=None) != 0 and "null" in L.last_error()
    assert count(bx=None) != 0 and "null" in L.last_error()
    assert count(s=(4, 0, 4)) != 0 and "bad extents" in L.last_error()
    assert count(s=(4, 4, 32768)) != 0 and "32767" in L.last_error()
    assert count(s=(2048, 2048, 512)) != 0 and "2^31" in L.last_error()

    def emit(s=(4, 4, 4), bx=box, sp=(1.0, 1.0, 1.0), na=3, nb=3, dist=p, cws=p, ews=p):
        return lib.seunet_surface_emit(*s, bx, *sp, na, nb, dist, None, cws, 1 << 20, ews, 1 << 20, None)
    assert emit(dist=None) != 0 and "null" in L.last_error()
    assert emit(bx=None) != 0 and "null" in L.last_error()
    assert emit(cws=None) != 0 and "null" in L.last_error()
    assert emit(s=(0, 4, 4)) != 0 and "bad extents" in L.last_error()
    for sp in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        assert emit(sp=sp) != 0 and "spacing" in L.last_error(), sp
    for bad in ((0, 5, 0, 4, 0, 4), (2, 2, 0, 4, 0, 4), (0, 4, -1, 4, 0, 4), (0, 4, 0, 4, 3, 1)):
        assert emit(bx=(C.c_int * 6)(*bad)) != 0 and "box" in L.last_error(), bad
    assert emit(na=0) != 0 and "without voxels" in L.last_error()
    assert emit(nb=0) != 0 and "without voxels" in L.last_error()

    tol = (C.c_double * 9)(*([1.0] * 9))
    assert lib.seunet_surface_summary(p, 3, 3, tol, 9, p, None) != 0 and "tolerances" in L.last_error()
    assert lib.seunet_surface_summary(p, 3, 3, None, 1, p, None) != 0 and "null" in L.last_error()
    assert lib.seunet_surface_summary(p, 3, 3, tol, 1, None, None) != 0 and "null" in L.last_error()
    assert lib.seunet_surface_summary(None, 3, 3, tol, 1, p, None) != 0 and "null" in L.last_error()
    assert lib.seunet_surface_summary(p, -1, 3, tol, 1, p, None) != 0 and "negative" in L.last_error()

    arr = lambda *v: (C.c_longlong * len(v))(*v)
    sel = lambda values=p, n=10, b=arr(0), e=arr(10), r=arr(0), k=1, out=p, ws=p: lib.seunet_select_ranks(values, n, b, e, r, k, out, ws, 1 << 20, None)
    assert sel(values=None) != 0 and "null" in L.last_error()
    assert sel(out=None) != 0 and "null" in L.last_error()
    assert sel(b=None) != 0 and "null" in L.last_error()
    assert sel(k=0) != 0 and "requests" in L.last_error()
    nine = arr(*([0] * 9))
    assert sel(b=nine, e=arr(*([10] * 9)), r=nine, k=9) != 0 and "requests" in L.last_error()
    assert sel(n=0) != 0 and "values" in L.last_error()
    assert sel(e=arr(11)) != 0 and "segment" in L.last_error()
    assert sel(b=arr(5), e=arr(5)) != 0 and "segment" in L.last_error()
    assert sel(r=arr(10)) != 0 and "rank" in L.last_error()
    assert sel(r=arr(-1)) != 0 and "rank" in L.last_error()
    assert lib.seunet_select_ranks(p, 10, arr(0), arr(10), arr(0), 1, p, p, 8, None) != 0 and "workspace too small" in L.last_error()


def test_python_argument_errors_name_the_argument():
    """Checked before anything touches a device: the percentile, the tolerances and ``empty``."""
    import seunet_amd as A
    m = np.ones((2, 2, 2), np.uint8)
    with pytest.raises(ValueError, match="percentile"):
        A.surface_metrics(m, m, percentile=100.5)
    with pytest.raises(ValueError, match="percentile"):
        A.surface_metrics(m, m, percentile=-1)
    with pytest.raises(ValueError, match="spacing"):
        A.surface_metrics(m, m, spacing=(1, 0, 1))
    with pytest.raises(ValueError, match="spacing"):
        A.surface_distances(m, m, spacing=(1, 1))
    with pytest.raises(ValueError, match="tolerances"):
        A.surface_metrics(m, m, tolerances=tuple(range(9)))
    with pytest.raises(ValueError, match="empty"):
        A.surface_metrics(m, m, empty="zero")
