"""The labelled surface meshing on the GPU (csrc/mesh_label.hip, seunet_amd.mesh.label_meshes / branch_meshes) against the numpy
oracle tests/mesh_label_oracle.py, bit for bit: positions, vertex and face numbering, orientation and the label pointers.  The
volumes are seeded and the smallest at which each mechanism can fail (word boundaries, two-label grid edges across bit 63 / 64,
more than one sort block, two radix digits, gaps and trailing empty labels)."""
import numpy as np
import pytest
import torch

import mesh_label_oracle as lo
import mesh_oracle as mo

pytestmark = pytest.mark.gpu

_WANT = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def volume(shape, labels, density, seed):
    L = lo.random_labels(shape, labels, density, seed)
    if shape[2] > 65:                                        # two different labels across the word boundary, one of them low
        L[1, 2, 63], L[1, 2, 64], L[2, 2, 63], L[2, 2, 64] = 1, 2, labels, 1
    return L


def want(key, make, num=None):
    """A volume and the oracle's meshes of it, computed once."""
    if key not in _WANT:
        L = make()
        _WANT[key] = (L, lo.label_meshes(L, num))
    return _WANT[key]


def same(got, res, what=""):
    verts, faces, vert_ptr, face_ptr = res
    assert isinstance(got.vert_ptr, np.ndarray) and got.vert_ptr.dtype == np.int64 and got.face_ptr.dtype == np.int64
    assert np.array_equal(got.vert_ptr, vert_ptr) and np.array_equal(got.face_ptr, face_ptr), what
    gv, gf = host(got.verts), host(got.faces)
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gv.shape == verts.shape and gf.shape == faces.shape, what
    assert np.array_equal(gf, faces), what
    assert np.array_equal(bits(gv), bits(verts)), what


SHAPES = {
    "5x6x67": ((5, 6, 67), 3, 0.5), "4x5x130": ((4, 5, 130), 3, 0.5), "9x10x70": ((9, 10, 70), 5, 0.5),
    "24x20x70": ((24, 20, 70), 300, 0.7),
    "28x20x70": ((28, 20, 70), 3, 0.3),                       # 1120 words: more than one scan block of words
}


def case(name):
    shape, labels, density = SHAPES[name]
    return want(name, lambda: volume(shape, labels, density, sum(shape)))


def test_eight_labels_in_one_cell(A):
    L = np.arange(1, 9, dtype=np.int32).reshape(2, 2, 2)
    got = A.label_meshes(torch.from_numpy(L).cuda())
    same(got, lo.label_meshes(L))
    assert got.verts.shape == (24, 3) and got.faces.shape == (8, 3) and got.num == 8


def test_every_filling_of_one_cell_with_two_labels(A):
    """Configuration c for label 1 and 255 - c for label 2, all 256 cells side by side with a background gap between them."""
    L = np.zeros((2, 2, 3 * 256), np.int32)
    for c in range(256):
        for bit, d in enumerate(mo.CORNERS):
            L[d[0], d[1], 3 * c + d[2]] = 1 if (c >> bit) & 1 else 2
    same(A.label_meshes(torch.from_numpy(L).cuda()), lo.label_meshes(L))
    for c in (0, 1, 0x69, 0x96, 0xfe, 0xff):                  # and on their own, without neighbours
        one = np.ascontiguousarray(L[:, :, 3 * c:3 * c + 2])
        same(A.label_meshes(torch.from_numpy(one).cuda(), num=2), lo.label_meshes(one, 2), c)


@pytest.mark.parametrize("shape", [(1, 5, 5), (5, 1, 5), (5, 5, 1)])
def test_an_extent_of_one_has_no_mesh(A, shape):
    L = lo.random_labels(shape, 4, 0.8, 5)
    L.reshape(-1)[0] = 4
    got = A.label_meshes(torch.from_numpy(L).cuda())
    assert got.verts.shape == (0, 3) and got.faces.shape == (0, 3)
    assert got.vert_ptr.tolist() == [0] * 5 and got.face_ptr.tolist() == [0] * 5
    same(got, lo.label_meshes(L))


def test_no_label_at_all(A):
    z = torch.zeros((4, 5, 6), dtype=torch.int32, device="cuda")
    got = A.label_meshes(z)
    assert got.verts.shape == (0, 3) and got.faces.shape == (0, 3) and got.vert_ptr.tolist() == [0] and got.num == 0
    got = A.label_meshes(z, num=3)
    assert got.vert_ptr.tolist() == [0] * 4 and got.face_ptr.tolist() == [0] * 4


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_oracle(A, name):
    L, res = case(name)
    got = A.label_meshes(torch.from_numpy(L).cuda())
    print(name, "V", len(res[0]), "F", len(res[1]), "num", len(res[2]) - 1)
    same(got, res, name)


def test_gaps_and_trailing_empty_labels(A):
    def make():
        L = lo.random_labels((9, 10, 70), 3, 0.5, 11)
        return np.choose(L, [0, 2, 7, 300]).astype(np.int32)
    L, res = want("gaps", make, 300)
    dev = torch.from_numpy(L).cuda()
    same(A.label_meshes(dev), res)
    same(A.label_meshes(dev, num=300), res)
    assert set(np.flatnonzero(np.diff(res[2])) + 1) == {2, 7, 300}
    _, res305 = want("gaps305", make, 305)
    got = A.label_meshes(dev, num=305)
    same(got, res305)
    assert got.num == 305 and got.mesh(303)[0].shape == (0, 3) and got.mesh(303)[1].shape == (0, 3)


def test_explicit_num_equals_the_found_one(A):
    L, res = case("9x10x70")
    dev = torch.from_numpy(L).cuda()
    found, given = A.label_meshes(dev), A.label_meshes(dev, num=int(L.max()))
    same(found, res)
    same(given, res)


def test_dtypes_and_a_non_contiguous_slice(A):
    L, res = case("9x10x70")
    for dtype in (torch.int64, torch.int16, torch.uint8):
        same(A.label_meshes(torch.from_numpy(L).cuda().to(dtype)), res, dtype)
    big = torch.zeros((9, 20, 75), dtype=torch.int32, device="cuda")
    big[:, ::2, 3:73] = torch.from_numpy(L).cuda()
    view = big[:, ::2, 3:73]
    assert not view.is_contiguous()
    same(A.label_meshes(view), res)


def test_numpy_round_trip(A):
    L, res = case("5x6x67")
    for a in (L, L.astype(np.int64), L.astype(np.uint16), L.astype(np.int8)):
        got = A.label_meshes(a)
        assert isinstance(got.verts, np.ndarray) and isinstance(got.faces, np.ndarray)
        same(got, res, a.dtype)
    got = A.branch_meshes(L, smooth=False)
    assert isinstance(got.verts, np.ndarray)
    same(got, res)


def test_two_calls_give_identical_bytes(A):
    L, _ = case("24x20x70")
    dev = torch.from_numpy(L).cuda()
    a, b = A.label_meshes(dev), A.label_meshes(dev)
    assert torch.equal(a.verts.view(torch.int32), b.verts.view(torch.int32)) and torch.equal(a.faces, b.faces)
    assert np.array_equal(a.vert_ptr, b.vert_ptr) and np.array_equal(a.face_ptr, b.face_ptr)


def test_every_label_equals_marching_cubes_of_its_mask(A):
    L, res = case("9x10x70")
    dev = torch.from_numpy(L).cuda()
    got = A.label_meshes(dev)
    for k in range(1, got.num + 1):
        v, f = got.mesh(k)
        mv, mf = A.marching_cubes(dev == k)
        assert torch.equal(v.view(torch.int32), mv.view(torch.int32)) and torch.equal(f, mf), k
        assert f.dtype == torch.int32
    with pytest.raises(IndexError):
        got.mesh(0)


@pytest.mark.parametrize("n_iter", [1, 20])
@pytest.mark.parametrize("moved", [False, True])
def test_branch_meshes(A, n_iter, moved):
    L, _ = case("9x10x70")
    centre, spacing = ((4.25, 5.5, 33.0), (0.7, 0.7, 1.25)) if moved else (None, None)
    key = ("branch", n_iter, moved)
    if key not in _WANT:
        _WANT[key] = lo.branch_meshes(L, spacing, centre, n_iter=n_iter)
    got = A.branch_meshes(torch.from_numpy(L).cuda(), spacing, centre, n_iter=n_iter)
    same(got, _WANT[key])
    if moved:                                                # one of the two alone
        same(A.branch_meshes(torch.from_numpy(L).cuda(), spacing=spacing, smooth=False), lo.branch_meshes(L, spacing, smooth=False))
        same(A.branch_meshes(torch.from_numpy(L).cuda(), centre=centre, smooth=False), lo.branch_meshes(L, centre=centre, smooth=False))


def test_one_smoothing_of_the_concatenation_equals_smoothing_per_label(A):
    L, _ = case("9x10x70")
    got = A.label_meshes(torch.from_numpy(L).cuda())
    whole = A.smooth_mesh(got.verts, got.faces, 3, 0.15)
    for k in range(1, got.num + 1):
        v, f = got.mesh(k)
        own = A.smooth_mesh(v.contiguous(), f.contiguous(), 3, 0.15)
        assert torch.equal(own.view(torch.int32), whole[int(got.vert_ptr[k - 1]):int(got.vert_ptr[k])].view(torch.int32)), k


def test_errors_are_value_errors_and_leave_the_library_usable(A):
    L, res = case("5x6x67")
    dev = torch.from_numpy(L).cuda()
    bad = dev.clone()
    bad[2, 3, 40] = -1
    with pytest.raises(ValueError, match="negative"):
        A.label_meshes(bad)
    with pytest.raises(ValueError, match="above num = 2"):
        A.label_meshes(dev, num=2)
    with pytest.raises(ValueError, match="65535"):
        A.label_meshes(dev, num=65536)
    with pytest.raises(ValueError):
        A.label_meshes(dev, num=-1)
    far = dev.clone()
    far[0, 0, 0] = 65536
    with pytest.raises(ValueError, match="65535"):
        A.label_meshes(far)
    far[0, 0, 0] = 2 ** 31 - 1
    with pytest.raises(ValueError, match="65535"):
        A.label_meshes(far)
    with pytest.raises(ValueError):
        A.label_meshes(dev, level=1.0)
    with pytest.raises(ValueError):
        A.label_meshes(dev[0])
    top = dev.clone()
    top[0, 0, 0] = 65535                                      # the largest label there is
    got = A.label_meshes(top)
    assert got.num == 65535 and np.array_equal(host(got.mesh(65535)[1]), lo.mesh(lo.label_meshes((host(top) == 65535) * 1), 1)[1])
    same(A.label_meshes(dev), res)


def test_v_or_3f_beyond_int32_is_refused_by_the_library(A):
    """The wrapper raises before it calls; the entry point refuses on its own account (no launch happens)."""
    lib = A._lib.load()
    assert lib.seunet_mesh_label_emit(1, 4, 4, 4, 1, 0.95, 2 ** 31, 0, None, None, 1, 0, None, 0, None) != 0
    assert "int32" in A._lib.last_error()
    assert lib.seunet_mesh_label_emit(1, 4, 4, 4, 1, 0.95, 3, 2 ** 31 // 3 + 1, None, None, 1, 0, None, 0, None) != 0
    assert "int32" in A._lib.last_error()
