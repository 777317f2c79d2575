"""Surface meshing on the GPU (csrc/mesh.hip, seunet_amd.mesh) against the numpy oracle tests/mesh_oracle.py, bit for bit:
extraction, adjacency, smoothing, STL records, and the reference's whole mesh step.  Every expected value comes from the oracle
or from numpy, never from the code under test.  The oracle's results are computed once per volume and shared."""
import io
import os

import numpy as np
import pytest
import torch

import mesh_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def noise(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def make_volume(name):
    if name == "empty":
        return np.zeros((4, 5, 6), np.uint8)
    if name == "single":
        v = np.zeros((3, 3, 3), np.uint8)
        v[1, 1, 1] = 1
        return v
    if name == "flat0":
        return noise((1, 5, 5), 0.5, 1)
    if name == "flat1":
        return noise((5, 1, 5), 0.5, 2)
    if name in ("word67", "word130"):                       # rows that cross a 64-lane word, foreground in lanes 63 and 64
        v = noise((5, 6, 67) if name == "word67" else (4, 5, 130), 0.5, 3)
        v[1, 2, 63] = v[1, 2, 64] = 1
        v[2, 3, 63], v[2, 3, 64] = 1, 0
        v[3, 1, 63], v[3, 1, 64] = 0, 1
        return v
    if name == "many":                                      # 3200 words: more than one block of the scan
        return noise((40, 40, 70), 0.3, 4)
    if name == "open":                                      # foreground on every face of the border: an open mesh
        v = noise((9, 10, 70), 0.4, 5)
        v[0, 3:6, 10:30] = v[-1, 2:5, 40:69] = 1
        v[2:5, 0, 5:20] = v[3:7, -1, 50:66] = 1
        v[1:4, 2:6, 0] = v[4:8, 5:9, -1] = 1
        return v
    if name == "slabs":                                     # rows whose 2 x 2 neighbourhood is all 0 / all 1 are skipped
        v = noise((14, 6, 70), 0.5, 6)
        v[2:6] = 0
        v[8:12] = 1
        return v
    raise KeyError(name)


_CACHE = {}


def case(name, level=0.95):
    """(volume, oracle verts, oracle faces), computed once."""
    key = (name, level)
    if key not in _CACHE:
        v = make_volume(name)
        _CACHE[key] = (v,) + mo.marching_cubes(v, level)
    return _CACHE[key]


def adjacency_of(name):
    key = (name, "adjacency")
    if key not in _CACHE:
        _, verts, faces = case(name)
        _CACHE[key] = mo.adjacency(faces, len(verts))
    return _CACHE[key]


def same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- extraction ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["empty", "flat0", "flat1", "single", "word67", "word130", "many", "open", "slabs"])
@pytest.mark.parametrize("level", [0.95, 0.5])
def test_extraction_equals_the_oracle(A, name, level):
    v, verts, faces = case(name, level)
    got_v, got_f = A.marching_cubes(dev(v), level)
    assert got_v.is_cuda and got_f.is_cuda
    same(got_v, verts)
    same(got_f, faces)
    if name in ("empty", "flat0", "flat1"):
        assert tuple(got_v.shape) == (0, 3) and tuple(got_f.shape) == (0, 3)
    if name == "slabs":
        assert v[2:6].sum() == 0 and v[8:12].all()
    if name == "open":
        assert adjacency_of("open")[2].any()


def test_all_256_fillings_of_one_cell(A):
    for c in range(256):
        v = np.array([(c >> b) & 1 for b in range(8)], np.uint8).reshape(2, 2, 2)   # corner bit 4*d0 + 2*d1 + d2
        verts, faces = mo.marching_cubes(v)
        assert len(faces) == len(mo.TABLE[c])
        got_v, got_f = A.marching_cubes(dev(v))
        same(got_v, verts)
        same(got_f, faces)


def test_non_contiguous_and_bool_inputs(A):
    v, verts, faces = case("word67")
    wide = dev(np.concatenate([v, 1 - v], axis=2))[:, :, :v.shape[2]]
    assert not wide.is_contiguous()
    for t in (wide, dev(v).bool(), dev(v) * 7):
        got_v, got_f = A.marching_cubes(t)
        same(got_v, verts)
        same(got_f, faces)


def test_two_calls_give_identical_bytes(A):
    v, _, _ = case("many")
    t = dev(v)
    a, b = A.marching_cubes(t), A.marching_cubes(t)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    s1, s2 = A.smooth_mesh(*a, n_iter=2), A.smooth_mesh(*b, n_iter=2)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))


def test_numpy_round_trip(A):
    v, verts, faces = case("word130")
    got_v, got_f = A.marching_cubes(v.astype(np.int16) * 3)
    assert isinstance(got_v, np.ndarray) and isinstance(got_f, np.ndarray)
    same(got_v, verts)
    same(got_f, faces)


# ---- adjacency and smoothing ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["many", "open"])
def test_adjacency_equals_the_oracle(A, name):
    _, verts, faces = case(name)
    indptr, indices, boundary = adjacency_of(name)
    got = A.mesh_adjacency(dev(faces), len(verts))
    same(got[0], indptr)
    same(got[1], indices)
    same(got[2], boundary)


TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.3, 0.4, 0.5]], np.float32)      # vertex 4: no face
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


@pytest.mark.parametrize("name", ["many", "open", "tetrahedron"])
def test_smoothing_equals_the_oracle(A, name):
    if name == "tetrahedron":                               # every vertex has degree 3
        verts, faces = TETRA_V, TETRA_F
        boundary = np.zeros(5, np.uint8)
    else:
        _, verts, faces = case(name)
        boundary = adjacency_of(name)[2]
    v, f = dev(verts), dev(faces)
    for n_iter in (1, 20):
        want = mo.smooth(verts, faces, n_iter, 0.2)
        got = A.smooth_mesh(v, f, n_iter=n_iter, relaxation_factor=0.2)
        same(got, want)
        if name == "open":                                  # boundary vertices stay, bit for bit
            assert boundary.any()
            same(got.cpu().numpy()[boundary != 0], verts[boundary != 0])
    same(A.smooth_mesh(v, f), mo.smooth(verts, faces, 20, 0.2))              # the defaults
    same(A.smooth_mesh(v, f, n_iter=0), verts)
    same(v, verts)                                                           # the input is left alone


# ---- STL --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["word67", "many"])
def test_stl_records_equal_the_oracle(A, name):
    _, verts, faces = case(name)
    same(A.stl_records(dev(verts), dev(faces)), mo.stl_records(verts, faces))
    centre, scale = (1.5, 2.25, 30.1), (0.07, 0.07, 0.125)
    same(A.stl_records(dev(verts), dev(faces), centre, scale), mo.stl_records(verts, faces, centre, scale))
    same(A.transform_mesh(dev(verts), centre, scale), mo.affine(verts, centre, scale))


def test_stl_of_a_zero_area_triangle(A):
    verts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [4, 0, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 3], [1, 1, 2]], np.int32)
    got = A.stl_records(verts, faces)
    same(got, mo.stl_records(verts, faces))
    f = np.frombuffer(got.tobytes(), mo.STL_DTYPE)
    assert f["normal"].tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0]]


def test_write_stl(A, tmp_path):
    _, verts, faces = case("word67")
    path = os.path.join(tmp_path, "mesh.stl")
    n = A.write_stl(path, dev(verts), dev(faces), header=b"seunet")
    raw = open(path, "rb").read()
    assert n == len(raw) == 84 + 50 * len(faces)
    assert raw[:80] == b"seunet".ljust(80, b"\0") and int(np.frombuffer(raw[80:84], "<u4")[0]) == len(faces)
    rec = np.frombuffer(raw[84:], mo.STL_DTYPE)
    assert np.array_equal(rec["v"], verts[faces]) and not rec["attr"].any()
    buf = io.BytesIO()
    A.write_stl(buf, verts, faces)
    assert buf.getvalue()[84:] == raw[84:] and buf.getvalue()[:80] == bytes(80)


# ---- the reference's mesh step ---------------------------------------------------------------------------------------------------

def tree():
    """A small airway-like tree: a trunk along axis 2 that splits into two branches."""
    g = np.indices((48, 40, 40)).astype(np.float64)
    v = np.zeros((48, 40, 40), bool)
    for z in range(4, 22):
        v |= (g[0] - 24) ** 2 + (g[1] - 20) ** 2 + (g[2] - z) ** 2 < 3.2 ** 2
    for k in range(14):
        for side in (-1, 1):
            v |= (g[0] - (24 + side * 1.1 * k)) ** 2 + (g[1] - (20 + 0.3 * side * k)) ** 2 + (g[2] - (22 + k)) ** 2 < 2.3 ** 2
    return v.astype(np.uint8)


def test_prediction_mesh_is_the_composition_of_its_parts(A):
    mask = tree()
    spacing = (0.7, 0.8, 1.25)
    t = dev(mask)
    skel = A.skeletonize_3d(t)
    centre = np.mean(np.argwhere(skel.cpu().numpy()), axis=0, dtype=np.float64).astype(np.float32)
    assert skel.any()
    same(A.mesh.mean_coordinate(skel), centre)

    verts, faces = mo.marching_cubes(mask)
    scale = (np.asarray(spacing, np.float64) / 10.0).astype(np.float32)
    moved = mo.affine(verts, centre, scale)
    got_v, got_f = A.prediction_mesh(t, spacing)
    same(got_f, faces)
    same(got_v, mo.smooth(moved, faces, 20, 0.2))
    raw_v, raw_f = A.prediction_mesh(t, spacing, smooth=False, skeleton=skel)
    same(raw_v, moved)
    same(raw_f, faces)

    flip_v, flip_f = A.prediction_mesh(t, spacing, flip=True)
    want_v, want_f = A.prediction_mesh(t.flip(0), spacing)
    same(flip_v, want_v.cpu().numpy())
    same(flip_f, want_f.cpu().numpy())
    assert not torch.equal(flip_f, got_f) or not torch.equal(flip_v, got_v)

    np_v, np_f = A.prediction_mesh(mask, spacing)
    assert isinstance(np_v, np.ndarray) and isinstance(np_f, np.ndarray)
    same(np_v, got_v.cpu().numpy())
    same(np_f, faces)


# ---- errors --------------------------------------------------------------------------------------------------------------------------

def test_errors(A):
    t = dev(make_volume("single"))
    for level in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            A.marching_cubes(t, level)
    with pytest.raises(ValueError):
        A.marching_cubes(t[0])
    with pytest.raises(ValueError):
        A.marching_cubes(np.zeros((4, 4), np.uint8))
    with pytest.raises(RuntimeError):
        A.marching_cubes(t.cpu())
    with pytest.raises(ValueError):
        A.smooth_mesh(dev(TETRA_V), dev(TETRA_F + 2))        # an index past the last vertex
    with pytest.raises(ValueError):
        A.write_stl(io.BytesIO(), TETRA_V, TETRA_F, header=bytes(81))
