"""Host checks of the labelled surface meshing: known answers of the numpy oracle
(tests/mesh_label_oracle.py), the two bounds the kernels size their ballots with, and the workspace layout of the library (op 11
of the layout report).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import mesh_label_oracle as lo
import mesh_oracle as mo


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------

def test_eight_labels_in_one_cell():
    verts, faces, vert_ptr, face_ptr = lo.label_meshes(np.arange(1, 9).reshape(2, 2, 2))
    assert verts.shape == (24, 3) and faces.shape == (8, 3)
    assert vert_ptr.tolist() == list(range(0, 25, 3)) and face_ptr.tolist() == list(range(9))
    for k in range(1, 9):
        v, f = lo.mesh((verts, faces, vert_ptr, face_ptr), k)
        assert sorted(f.reshape(-1).tolist()) == [0, 1, 2]                     # one triangle over the label's own three vertices
        corner = np.array(np.unravel_index(k - 1, (2, 2, 2)), np.float32)
        assert np.allclose(np.abs(v - corner).sum(axis=1), 0.05, atol=1e-6)    # each 1 - level from its corner along one axis


def test_two_labels_without_background_share_every_edge():
    level = 0.95
    L = np.random.default_rng(1).integers(1, 3, (9, 10, 70))
    res = lo.label_meshes(L, level=level)
    assert np.diff(res[2]).tolist() == [8675, 8675]
    (v1, _), (v2, _) = lo.mesh(res, 1), lo.mesh(res, 2)
    t0, t1 = mo.offsets(level)
    # same grid edges in the same order; along the owning axis one label sits at `level`, the other at `1 - level`
    base1, base2 = np.floor(v1), np.floor(v2)
    assert np.array_equal(base1, base2)
    f1, f2 = (v1 - base1).sum(axis=1), (v2 - base2).sum(axis=1)
    lo_end_is_1 = np.isclose(f1, t1, atol=1e-4)             # (the fraction of a float32 near 70 carries 2^-17)
    assert np.allclose(f1, np.where(lo_end_is_1, t1, t0), atol=1e-4) and np.allclose(f2, np.where(lo_end_is_1, t0, t1), atol=1e-4)
    assert 0 < lo_end_is_1.sum() < len(v1)


def test_one_label_is_the_mask():
    v = mo.random_closed_volume(3)
    for label in (1, 7):
        res = lo.label_meshes(v.astype(np.int64) * label)
        want_v, want_f = mo.marching_cubes(v)
        got_v, got_f = lo.mesh(res, label)
        assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(got_f, want_f)
        assert res[2][:label].tolist() == [0] * label and len(res[2]) == label + 1


def test_absent_labels_have_empty_slices():
    L = np.zeros((4, 4, 4), np.int32)
    L[1, 1, 1], L[2, 2, 2] = 2, 5
    res = lo.label_meshes(L, num=7)
    assert np.diff(res[2]).tolist() == [0, 6, 0, 0, 6, 0, 0] and np.diff(res[3]).tolist() == [0, 8, 0, 0, 8, 0, 0]
    assert lo.label_meshes(np.zeros((1, 5, 5), np.int32) + 3)[0].shape == (0, 3)


def test_a_cell_has_at_most_eight_triangles_and_a_voxel_six_vertices():
    """The kernels rank a word's triangle items with 4 ballots (0 .. 15 per lane) and its vertex items with 3 (0 .. 7)."""
    worst, count = 0, 0
    for part in lo.set_partitions(8):                       # every block a label of its own: background only takes triangles away
        count += 1
        total = sum(int(mo.TRI_COUNT[sum(1 << c for c in range(8) if part[c] == b)]) for b in set(part))
        worst = max(worst, total)
    assert count == 4140 and worst == 8
    # a voxel owns three grid edges, an edge between labels p != q one vertex for each non-zero one
    L = np.array([[[1, 2], [3, 0]], [[4, 0], [0, 0]]])
    assert int((np.floor(lo.label_meshes(L)[0]) == 0).all(axis=1).sum()) == 6


# ---- the library's workspace layout ------------------------------------------------------------------------------------------

MESH_LABEL_OP = 11
LAYOUT_SHAPES = [(1, 1, 1), (3, 4, 5), (9, 8, 63), (9, 8, 65), (5, 6, 67), (24, 20, 70), (64, 64, 64), (300, 512, 512)]


def up(v, a=256):
    return (v + a - 1) // a * a


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    _lib.load()
    return _lib


def layout(lib, op, s):
    f = lib.seunet_debug_volume_layout
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t), C.c_int]
    buf = (C.c_size_t * 32)()
    count = f(op, s[0], s[1], s[2], buf, 16)
    return count, [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(max(count, 0))]


def test_layout_report_agrees_with_workspace_bytes(L):
    lib = L.load()
    for s in LAYOUT_SHAPES:
        count, spans = layout(lib, MESH_LABEL_OP, s)
        words = s[0] * s[1] * ((s[2] + 63) // 64)
        blocks = (words + 1023) // 1024
        # record, three count bit planes, two counts, word flags, two block sums, two label histograms, their block sums, their totals
        want = [24] + [8 * words] * 3 + [4 * words] * 2 + [words] + [4 * blocks] * 2 + [4 * 65536] * 2 + [4 * 64] * 2 + [16]
        assert count == len(want) == 14
        assert [b for _, b in spans] == [up(b) for b in want], s
        assert spans[0][0] == 0
        for (off, nbytes), (nxt, _) in zip(spans, spans[1:]):
            assert off + nbytes == nxt and off % 256 == 0 and nbytes > 0
        closed_form = 256 + 3 * up(8 * words) + 2 * up(4 * words) + up(words) + 2 * up(4 * blocks) + 2 * 4 * 65536 + 2 * 256 + 256
        assert sum(spans[-1]) == int(lib.seunet_mesh_label_workspace_bytes(*s)) == closed_form, s


def test_sort_workspace_bytes(L):
    lib = L.load()
    for V, F in ((0, 0), (1, 0), (24, 8), (1025, 3000), (135869, 169109)):
        m = max(V, F)
        bins = 256 * ((m + 1023) // 1024)
        want = 256 + up(4 * V) + up(4 * F) + up(2 * V) + up(2 * F) + up(2 * m) + up(4 * m) + up(4 * bins) + up(4 * ((bins + 1023) // 1024))
        assert int(lib.seunet_mesh_label_sort_bytes(V, F)) == want, (V, F)
    assert lib.seunet_mesh_label_sort_bytes(-1, 0) == 0 and "mesh_label_sort_bytes" in L.last_error()
    assert lib.seunet_mesh_label_sort_bytes(2 ** 31, 0) == 0


def test_rejected_extents(L):
    lib = L.load()
    assert lib.seunet_mesh_label_workspace_bytes(0, 4, 4) == 0
    assert "mesh_label_workspace_bytes" in L.last_error()
    assert lib.seunet_mesh_label_workspace_bytes(4, 4, 0) == 0
    assert "mesh_label_workspace_bytes" in L.last_error()
    assert lib.seunet_mesh_label_workspace_bytes(2048, 2048, 512) == 0
    assert "2^31" in L.last_error()
    assert layout(lib, MESH_LABEL_OP, (0, 4, 4))[0] == 0 and layout(lib, MESH_LABEL_OP, (2048, 2048, 512))[0] == 0
