"""Component labelling, Euler number and Betti numbers: what can be checked without a GPU.

* the oracle (tests/betti_oracle.py) against known answers and against itself (two formulas for one number);
* the properties that make each case of tests/test_betti_gpu.py worth running, asserted here on the CPU;
* the workspace layouts of the new operations against closed-form byte counts;
* the error paths of the library, which return before any device work (this file runs where there is no device)."""
import ctypes as C
import functools

import numpy as np
import pytest

import betti_oracle as bo

# ---- the volumes of the GPU cases (tests/test_betti_gpu.py imports them) ---------------------------------------------------------------
RANDOM = {"tail_3x4x130": ((3, 4, 130), 0.5), "flat0_1x9x70": ((1, 9, 70), 0.5), "flat1_9x1x70": ((9, 1, 70), 0.5),
          "flat2_40x30x1": ((40, 30, 1), 0.5), "noise10": ((20, 21, 70), 0.1), "noise30": ((20, 21, 70), 0.3),
          "noise50": ((20, 21, 70), 0.5), "noise70": ((20, 21, 70), 0.7)}
NAMES = list(RANDOM) + ["zeros_5x6x70", "ones_5x6x70"] + list(bo.KNOWN) + ["serpentine"]
LARGE_SHAPE, LARGE_DENSITY = (1025, 1024, 2), 0.3


@functools.lru_cache(maxsize=None)
def volume(name):
    if name in RANDOM:
        shape, density = RANDOM[name]
        v = bo.noise(shape, density, 100 + list(RANDOM).index(name))
    elif name == "zeros_5x6x70":
        v = np.zeros((5, 6, 70), dtype=np.uint8)
    elif name == "ones_5x6x70":
        v = np.ones((5, 6, 70), dtype=np.uint8)
    elif name == "serpentine":
        return bo.serpentine()
    elif name == "large":
        v = bo.noise(LARGE_SHAPE, LARGE_DENSITY, 5)
    else:
        return bo.known(name)
    v.setflags(write=False)
    return v


# ---- known answers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bo.KNOWN))
@pytest.mark.parametrize("connectivity", [3, 1])
def test_known_betti_numbers(name, connectivity):
    assert bo.betti_numbers(bo.known(name), connectivity) == bo.KNOWN[name]


def test_euler_number_of_ball_torus_shell():
    for c in (3, 1):
        assert [bo.euler_number(bo.known(n), c) for n in ("ball", "torus", "shell")] == [1, 0, 2]


def test_corner_contact_is_one_piece_at_26_only():
    v = np.zeros((3, 3, 3), dtype=np.uint8)
    v[0, 0, 0] = v[1, 1, 1] = 1
    assert [bo.label(v, c)[1] for c in (1, 2, 3)] == [2, 2, 1]
    assert bo.betti_numbers(v, 3) == (1, 0, 0) and bo.betti_numbers(v, 1) == (2, 0, 0)


def test_edge_contact_is_one_piece_at_18_and_26():
    v = np.zeros((3, 3, 3), dtype=np.uint8)
    v[0, 0, 1] = v[1, 1, 1] = 1
    assert [bo.label(v, c)[1] for c in (1, 2, 3)] == [2, 1, 1]


def test_a_shell_cut_by_the_volume_border_has_no_cavity():
    whole = bo.known("shell")
    assert bo.betti_numbers(whole, 3)[2] == 1
    cut = whole[:, :, :13]                                     # through the centre: the cavity opens to the outside
    assert bo.betti_numbers(cut, 3)[2] == 0 and bo.betti_numbers(cut, 1)[2] == 0


# ---- cross-checks of the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_b1_is_not_negative(name):
    for c in (3, 1):
        assert bo.betti_numbers(volume(name), c)[1] >= 0


def test_label_order_is_the_rank_of_the_minimum_linear_index():
    for name in ("noise10", "noise30", "tail_3x4x130"):
        for c in (1, 2, 3):
            lab, num = bo.label(volume(name), c)
            _, first, _ = bo.table(lab, num)
            assert np.array_equal(first, np.sort(first)) and len(np.unique(first)) == num
            assert np.array_equal(lab.ravel()[first], np.arange(1, num + 1))


def test_table_against_a_loop():
    lab, num = bo.label(volume("noise10"), 3)
    size, first, box = bo.table(lab, num)
    for k in (0, num // 2, num - 1):
        idx = np.argwhere(lab == k + 1)
        assert size[k] == len(idx) and first[k] == np.flatnonzero(lab.ravel() == k + 1)[0]
        assert list(box[k]) == [idx[:, 0].min(), idx[:, 0].max(), idx[:, 1].min(), idx[:, 1].max(), idx[:, 2].min(), idx[:, 2].max()]


def test_euler_of_the_tile_loop_is_the_euler_of_the_crops():
    v = bo.tile_volume("dense")
    for c in (3, 1):
        chi = bo.euler_tiles(v, (16, 16, 24), c)
        tab, tiles = bo.tile_tables("dense", (16, 16, 24), c)
        assert tiles == (3, 4, 7) and len(chi) == 84
        assert np.array_equal(chi, tab[:, 0].astype(np.int64) - tab[:, 1] + tab[:, 2])
        assert chi[0] == bo.euler_number(v[:16, :16, :24], c) and chi[-1] == bo.euler_number(v[32:, 48:, 144:], c)


def test_remove_small_objects_oracle():
    v = volume("noise10")
    lab, num = bo.label(v, 3)
    size = bo.table(lab, num)[0]
    assert np.array_equal(bo.remove_small_objects(v, 1, 3), v)
    kept = bo.remove_small_objects(v, 50, 3)
    assert kept.sum() == size[size >= 50].sum() and 0 < kept.sum() < v.sum()


# ---- what makes each GPU case worth running -------------------------------------------------------------------------------------------
def test_random_cases_have_many_components_loops_and_cavities():
    b = {n: bo.betti_numbers(volume(n), 3) for n in ("noise10", "noise30", "noise50", "noise70")}
    assert b["noise10"][0] > 100 and b["noise70"][0] == 1
    assert max(v[1] for v in b.values()) > 1000 and b["noise70"][2] > 1000
    b1 = {n: bo.betti_numbers(volume(n), 1) for n in ("noise10", "noise50", "noise70")}
    assert b1["noise10"][0] > 1000 and b1["noise70"][1] > 1000
    for n in ("tail_3x4x130", "flat0_1x9x70", "flat1_9x1x70", "flat2_40x30x1"):
        assert bo.label(volume(n), 1)[1] > 1


def test_serpentine_is_one_long_component():
    s = volume("serpentine")
    assert s.shape == (8, 16, 200) and s.sum() > 32 * 200
    assert bo.betti_numbers(s, 3) == (1, 0, 0) and bo.betti_numbers(s, 1) == (1, 0, 0)
    assert s[:, :, 63].any() and s[:, :, 64].any() and s[:, :, 128].any()      # its links cross the 64-voxel spans


def test_large_case_has_more_than_65535_components_and_2_pow_20_words():
    v = volume("large")
    assert bo.label(v, 1)[1] > 65535
    assert v.shape[0] * v.shape[1] * ((v.shape[2] + 63) // 64) > 1 << 20


def test_tile_cases_cut_components_and_cavities_and_words():
    v = bo.tile_volume("shapes")
    assert bo.betti_numbers(v, 3) == (2, 1, 1)
    patch = bo.TILE_PATCHES[0]
    slices, tiles = bo.tile_slices(v.shape, patch)
    lab, _ = bo.label(v, 3)
    hole = bo.label(1 - v, 1)[0]
    cavity = hole == hole[32, 32, 96]                          # the inside of the shell
    assert hole[32, 32, 96] != hole[0, 0, 0]
    for part in (lab == 1, lab == 2, cavity):
        assert sum(bool(part[s].any()) for s in slices) >= 8   # across a tile corner: eight tiles
    tab = bo.tile_tables("shapes", patch, 3)[0]
    assert tab[:, 2].sum() == 0 and tab[:, 0].sum() >= 16      # no tile sees the cavity closed; every piece is cut
    for p in bo.TILE_PATCHES[:2]:
        assert all(n % q for n, q in zip(v.shape, p))          # a ragged last tile on every axis
    for p in bo.TILE_PATCHES[2:]:
        assert any(n % q for n, q in zip(v.shape, p)) and not all(n % q for n, q in zip(v.shape, p))   # ragged and exact axes mixed
    assert any(p[2] % 64 for p in bo.TILE_PATCHES) and 24 % 64 and 13 % 64   # tile borders strictly inside a 64-bit word
    assert np.prod(bo.tile_slices(v.shape, (7, 5, 13))[1]) == 720
    for which in ("sparse", "dense"):
        assert bo.tile_tables(which, patch, 3)[0][:, 0].max() > 1   # more than one component in a tile
    assert bo.tile_tables("dense", patch, 3)[0][:, 1].max() > 0


# ---- the library without a device --------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (3, 4, 5), (9, 8, 63), (9, 8, 65), (3, 5, 257), (2, 129, 3), (17, 5, 130), (64, 64, 64), (1025, 1024, 2)]
OPS = {"label": (15, 7), "euler": (16, 2), "betti": (17, 4)}


def up(v, a=256):
    return (v + a - 1) // a * a


def sub_buffers(name, s):
    n, w = s[0] * s[1] * s[2], s[0] * s[1] * ((s[2] + 63) // 64)
    if name == "label":
        return [4 * n, 4 * n, 8 * w, 4 * w, 4 * ((w + 1023) // 1024), 4 * (w + 1), 16]
    if name == "euler":
        return [8 * w, 32]
    return [4 * n, n, 8 * w, 32]


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    _lib.load()
    return _lib


def query(L, name, s, patch=None):
    lib = L.load()
    if name == "label":
        return int(lib.seunet_label_workspace_bytes(*s))
    return int(getattr(lib, f"seunet_{name}_workspace_bytes")(*s, *(patch or s)))


def layout(L, name, s):
    f = L.load().seunet_debug_volume_layout                  # diagnostic export, not in the public header
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t), C.c_int]
    buf = (C.c_size_t * 32)()
    count = f(OPS[name][0], s[0], s[1], s[2], buf, 16)
    return count, [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(max(count, 0))]


@pytest.mark.parametrize("name", list(OPS))
def test_sub_buffers_tile_the_workspace(L, name):
    for s in SHAPES:
        got, spans = layout(L, name, s)
        assert got == OPS[name][1], (name, s)
        assert [b for _, b in spans] == [up(b) for b in sub_buffers(name, s)], (name, s)
        assert spans[0][0] == 0
        for (off, nbytes), (nxt, _) in zip(spans, spans[1:]):
            assert off % 256 == 0 and off + nbytes == nxt
        assert sum(spans[-1]) == query(L, name, s) == sum(up(b) for b in sub_buffers(name, s)), (name, s)


def test_tile_counters_grow_with_the_tiles(L):
    s = (40, 50, 150)
    n, w = 40 * 50 * 150, 40 * 50 * 3
    assert query(L, "euler", s, (7, 5, 13)) == up(8 * w) + up(32 * 720)
    assert query(L, "betti", s, (7, 5, 13)) == up(4 * n) + up(n) + up(8 * w) + up(32 * 720)
    assert query(L, "betti", s, (400, 500, 1500)) == query(L, "betti", s)          # a patch past the volume is the volume


def test_layout_of_rejected_extents_is_empty(L):
    for name in OPS:
        assert layout(L, name, (2048, 2048, 512))[0] == 0 and layout(L, name, (0, 4, 4))[0] == 0


def test_error_paths_return_before_device_work(L):
    """No device here: a call that reached a memset or a launch would report a HIP error, not the message of its check."""
    lib = L.load()
    one = C.create_string_buffer(64)
    p = C.addressof(one)
    assert query(L, "label", (0, 4, 4)) == 0 and "label_workspace_bytes: bad extents (0, 4, 4)" in L.last_error()
    assert query(L, "label", (2048, 2048, 512)) == 0 and "fewer than 2^31" in L.last_error()
    assert query(L, "betti", (4, 4, 4), (0, 4, 4)) == 0 and "betti_workspace_bytes: bad patch (0, 4, 4)" in L.last_error()
    assert query(L, "euler", (4, 4, 0)) == 0 and "euler_workspace_bytes: bad extents" in L.last_error()
    assert lib.seunet_label(p, 4, 4, 4, 4, p, None, p, 1 << 20, None) == 1 and "label: connectivity 4" in L.last_error()
    assert lib.seunet_label(p, 4, -1, 4, 3, p, None, p, 1 << 20, None) == 1 and "label: bad extents" in L.last_error()
    assert lib.seunet_label(p, 4, 4, 4, 3, p, None, p, 16, None) == 1 and "label: workspace too small" in L.last_error()
    assert lib.seunet_remove_small_objects(p, 4, 4, 4, 2, 0, p, p, 1 << 20, None) == 1 and "connectivity 0" in L.last_error()
    assert lib.seunet_component_table(p, 4, 4, 4, 0, p, p, p, p, 1 << 20, None) == 1 and "0 components" in L.last_error()
    for f, what in ((lib.seunet_euler, "euler"), (lib.seunet_betti, "betti")):
        assert f(p, 4, 4, 4, 4, 4, 4, 2, p, p, 1 << 20, None) == 1 and f"{what}: connectivity 2" in L.last_error()
        assert f(p, 4, 4, 4, 4, 0, 4, 3, p, p, 1 << 20, None) == 1 and f"{what}: bad patch (4, 0, 4)" in L.last_error()
        assert f(p, 2048, 2048, 512, 4, 4, 4, 3, p, p, 1 << 20, None) == 1 and "fewer than 2^31" in L.last_error()
        assert f(p, 4, 4, 4, 4, 4, 4, 3, p, p, 16, None) == 1 and f"{what}: workspace too small" in L.last_error()


def test_wrapper_argument_errors():
    import seunet_amd as A
    v = np.zeros((4, 4, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match="connectivity"):
        A.betti_numbers(v, connectivity=2)
    with pytest.raises(ValueError, match="connectivity"):
        A.euler_number(v, connectivity=2)
    with pytest.raises(ValueError, match="connectivity"):
        A.label(v, connectivity=4)
    with pytest.raises(ValueError, match="connectivity"):
        A.betti_error(v, v, connectivity=2)
    assert A.components.label is A.label and A.components.remove_small_objects is A.remove_small_objects


def test_mean_abs_error_is_plain_numpy():
    from seunet_amd.components import mean_abs_error
    a = np.array([[1, 0, 2], [3, 1, 0]], dtype=np.int32)
    b = np.array([[1, 2, 0], [0, 1, 1]], dtype=np.int32)
    got = mean_abs_error(a, b)
    assert got.dtype == np.float64 and list(got) == [1.5, 1.0, 1.5]
