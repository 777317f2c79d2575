"""Host checks of the surface meshing: the triangle table, known answers and topological properties of
the numpy oracle (tests/mesh_oracle.py), the generated header, and the workspace layout of the library.  No GPU."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import mesh_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def generator():
    spec = importlib.util.spec_from_file_location("gen_mesh_table", os.path.join(ROOT, "scripts", "gen_mesh_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def crossing_edges(c):
    return {e for e in range(12) if mo._fg(c, mo.EDGE_ENDS[e][0]) != mo._fg(c, mo.EDGE_ENDS[e][1])}


# ---- the table -----------------------------------------------------------------------------------------------------------------

def test_table_sizes():
    assert max(len(t) for t in mo.TABLE) == 5
    assert sum(len(t) for t in mo.TABLE) == 820
    assert mo.TABLE[0] == [] and mo.TABLE[255] == []


@pytest.mark.parametrize("c", range(256))
def test_table_configuration(c):
    tris = mo.TABLE[c]
    used = {e for t in tris for e in t}
    assert used == crossing_edges(c)                                     # every sign-changing edge, and no other
    assert used == {e for t in mo.TABLE[255 - c] for e in t}              # the complement uses the same vertex set
    directed = [(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)]
    for a, b in set(directed):
        assert a != b
        if (b, a) in directed:                                           # an interior diagonal: once in each direction
            assert directed.count((a, b)) == 1 and directed.count((b, a)) == 1
            assert not mo._share_face(a, b)                              # never inside a cube face
        else:                                                            # a face segment: once in the cell, inside a face
            assert directed.count((a, b)) == 1
            assert mo._share_face(a, b)


def test_generator_and_oracle_derive_the_same_table():
    assert generator().table() == mo.TABLE


def test_committed_header_is_the_generators_output():
    g = generator()
    with open(g.HEADER) as f:
        assert f.read() == g.render()


# ---- known answers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0.95, 0.5, 0.25])
def test_single_voxel(level):
    v = np.zeros((3, 3, 3), np.uint8)
    v[1, 1, 1] = 1
    verts, faces = mo.marching_cubes(v, level)
    assert verts.shape == (6, 3) and faces.shape == (8, 3) and verts.dtype == np.float32 and faces.dtype == np.int32
    r = np.linalg.norm(verts.astype(np.float64) - 1.0, axis=1)
    assert np.allclose(r, 1.0 - level, rtol=0, atol=2e-7)                # float32 coordinates near 1
    exact = np.where(verts == np.floor(verts), verts, np.where(verts < 1, level, 2 - level)).astype(np.float64)
    want = 4.0 / 3.0 * (1.0 - level) ** 3
    # 8 triple products of coordinates below 2 (each below 8, a few roundings each), summed and divided by 6
    assert abs(mo.signed_volume(exact, faces) - want) <= 8 * 8 * 8 * np.finfo(np.float64).eps / 6


def test_vertex_coordinates_are_rounded_once():
    v = np.zeros((2, 2, 70), np.uint8)
    v[0, 0, 65] = 1
    verts, _ = mo.marching_cubes(v, 0.95)
    t0, t1 = np.float32(0.95), np.float32(1.0 - 0.95)
    assert set(verts[:, 2].tolist()) == {float(np.float32(64) + t0), float(np.float32(65) + t1), 65.0}


def test_box_has_euler_characteristic_two():
    v = np.zeros((6, 7, 8), np.uint8)
    v[2:4, 2:5, 2:6] = 1
    verts, faces = mo.marching_cubes(v)
    edges = {tuple(sorted(e)) for e in mo.directed_edges(faces).tolist()}
    assert len(verts) - len(edges) + len(faces) == 2
    assert mo.signed_volume(verts, faces) > 0


def test_no_cells_no_mesh():
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        verts, faces = mo.marching_cubes(np.random.default_rng(5).random(shape) < 0.5)
        assert verts.shape == (0, 3) and faces.shape == (0, 3)


# ---- random volumes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(10))
def test_closed_volumes_give_closed_oriented_manifolds(seed):
    v = mo.random_closed_volume(seed)
    assert v.any()
    verts, faces = mo.marching_cubes(v)
    d = mo.directed_edges(faces)
    key = d[:, 0] * len(verts) + d[:, 1]
    assert len(np.unique(key)) == len(key)                                # every directed edge once ...
    assert np.array_equal(np.sort(key), np.sort(d[:, 1] * len(verts) + d[:, 0]))   # ... and its reverse once
    assert mo.signed_volume(verts, faces) > 0
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))        # no vertex without a face
    _, _, boundary = mo.adjacency(faces, len(verts))
    assert not boundary.any()


@pytest.mark.parametrize("seed", range(4))
def test_euler_characteristic_is_two_per_component(seed):
    """A closed orientable edge-manifold surface made of spheres only would give 2 per component; handles lower it by 2 each,
    so V - E + F is even and at most twice the number of components."""
    v = mo.random_closed_volume(seed)
    verts, faces = mo.marching_cubes(v)
    edges = {tuple(sorted(e)) for e in mo.directed_edges(faces).tolist()}
    chi = len(verts) - len(edges) + len(faces)
    comps = mo.mesh_components(len(verts), faces)
    assert chi % 2 == 0 and chi <= 2 * comps


def test_euler_characteristic_sums_over_components():
    """Separate convex blobs: every mesh component is a sphere, V - E + F = 2 per component."""
    v = np.zeros((12, 12, 12), np.uint8)
    v[1:3, 1:4, 1:3] = 1
    v[6:9, 6:8, 5:10] = 1
    v[9, 2, 2] = 1
    v[4, 9, 2:5] = 1
    verts, faces = mo.marching_cubes(v)
    edges = {tuple(sorted(e)) for e in mo.directed_edges(faces).tolist()}
    assert mo.mesh_components(len(verts), faces) == 4
    assert len(verts) - len(edges) + len(faces) == 2 * 4


def test_open_mesh_has_boundary_vertices():
    v = np.ones((4, 4, 4), np.uint8)
    v[1:3, 1:3, :] = 0                                                   # a channel that runs out of both faces
    verts, faces = mo.marching_cubes(v)
    _, _, boundary = mo.adjacency(faces, len(verts))
    assert boundary.any() and not boundary.all()
    moved = mo.smooth(verts, faces, 3)
    assert np.array_equal(moved[boundary != 0].view(np.uint32), verts[boundary != 0].view(np.uint32))


def test_adjacency_and_smoothing_of_a_tetrahedron():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    indptr, indices, boundary = mo.adjacency(faces, 4)
    assert indptr.tolist() == [0, 3, 6, 9, 12] and indices.tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    assert not boundary.any()
    lam = np.float32(0.2)
    third = (np.float32(0) + verts[1] + verts[2] + verts[3]) / np.float32(3)
    want0 = verts[0] + lam * (third - verts[0])
    assert np.array_equal(mo.smooth(verts, faces, 1)[0], want0)
    assert np.array_equal(mo.smooth(verts, faces, 0), verts)


def test_stl_record_layout():
    verts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [1, 1, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 0, 3]], np.int32)
    rec = mo.stl_records(verts, faces)
    assert rec.shape == (2, 50) and rec.dtype == np.uint8
    f = np.frombuffer(rec.tobytes(), mo.STL_DTYPE)
    assert f["normal"].tolist() == [[0, 0, 1], [0, 0, 0]] and f["attr"].tolist() == [0, 0]
    assert np.array_equal(f["v"][0], verts[[0, 1, 2]])
    moved = np.frombuffer(mo.stl_records(verts, faces, (1, 1, 1), (2, 2, 0.5)).tobytes(), mo.STL_DTYPE)
    assert np.array_equal(moved["v"][0], [[-2, -2, -0.5], [2, -2, -0.5], [-2, 2, -0.5]])


# ---- the library's workspace layout ------------------------------------------------------------------------------------------

MESH_OP = 10
LAYOUT_SHAPES = [(1, 1, 1), (3, 4, 5), (9, 8, 63), (9, 8, 65), (5, 6, 67), (40, 40, 70), (64, 64, 64), (300, 512, 512)]


def up(v, a=256):
    return (v + a - 1) // a * a


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    _lib.load()
    return _lib


def test_layout_report_agrees_with_workspace_bytes(L):
    lib = L.load()
    f = lib.seunet_debug_volume_layout
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t), C.c_int]
    for s in LAYOUT_SHAPES:
        buf = (C.c_size_t * 32)()
        count = f(MESH_OP, s[0], s[1], s[2], buf, 16)
        spans = [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(count)]
        words = s[0] * s[1] * ((s[2] + 63) // 64)
        blocks = (words + 1023) // 1024
        want = [16] + [8 * words] * 4 + [4 * words] * 2 + [4 * blocks] * 2   # totals, bits, three edge masks, counts, block sums
        assert [b for _, b in spans] == [up(b) for b in want], s
        assert spans[0][0] == 0
        for (off, nbytes), (nxt, _) in zip(spans, spans[1:]):
            assert off + nbytes == nxt
        assert sum(spans[-1]) == int(lib.seunet_mesh_workspace_bytes(*s)), s


def test_rejected_extents(L):
    lib = L.load()
    assert lib.seunet_mesh_workspace_bytes(0, 4, 4) == 0
    assert "mesh_workspace_bytes" in L.last_error()
    assert lib.seunet_mesh_workspace_bytes(2048, 2048, 512) == 0
    assert "2^31" in L.last_error()
