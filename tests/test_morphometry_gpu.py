"""The branch morphometry on the GPU (csrc/morphometry.hip, seunet_amd.morphometry) against the numpy oracle
tests/morphometry_oracle.py: every integer table bit for bit (``np.array_equal``, dtype included), the derived float64 columns at
rtol = 1e-12 (they are sums of at most 26 non-negative float64 terms, a rounding bound near 3e-15; the margin covers another
summation order).  Shapes are the smallest that reach every path: extents of 1, rows shorter and longer than a wave, runs of
equal labels across row, plane and wave ends, labels that share a slot of the volume pass's 256-row LDS table, a skeleton at every address modulo 16,
more voxels than the volume pass has workgroups x 256 and than one sweep of the skeleton pass (4096 workgroups x 4096 bytes), and
sums beyond 2^32."""
import os

import numpy as np
import pytest
import torch

import morphometry_oracle as mo
import skeleton_oracle as so

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACING = (0.7, 0.8, 1.25)
RTOL = 1e-12
EDGE_SHAPES = ((1, 1, 1), (1, 1, 70), (2, 3, 67), (3, 5, 7), (5, 1, 130))
_FIX = {}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def same_tables(got, want_rows0):
    want = mo.rows_from_one(want_rows0)
    assert sorted(got) == sorted(mo.INT_TABLES)
    for k in mo.INT_TABLES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def check(A, parsing, skeleton, num, sqdist=None):
    """branch_stats on device tensors against the oracle; returns the GPU tables."""
    want, status = mo.branch_stats(parsing, skeleton, num, sqdist)
    assert status == 0
    got = A.branch_stats(torch.from_numpy(parsing).cuda(), torch.from_numpy(skeleton).cuda(), num,
                         None if sqdist is None else torch.from_numpy(sqdist).cuda())
    same_tables(got, want)
    return got


# ---- the committed parse fixtures ---------------------------------------------------------------------------------------------
def fixture(A, case, key):
    """(parsing, skeleton, sqdist of the GPU EDT, num, oracle tables), computed once and left unchanged."""
    if (case, key) not in _FIX:
        z = np.load(os.path.join(ROOT, "tests", "golden", "parse_known.npz"))
        parsing = z[f"case{case}_{key}"].astype(np.int32)
        skeleton = np.ascontiguousarray(z[f"case{case}_skeleton"])
        sq = A.distance_transform_edt(torch.from_numpy(np.ascontiguousarray(z[f"case{case}_label"])).cuda(), return_distances=False,
                                      return_sqdist=True).cpu().numpy()
        num = int(parsing.max())
        want, status = mo.branch_stats(parsing, skeleton, num, sq)
        assert status == 0
        for a in (parsing, skeleton, sq):
            a.setflags(write=False)
        _FIX[(case, key)] = (parsing, skeleton, sq, num, want)
    return _FIX[(case, key)]


@pytest.mark.parametrize("key", ["parsing", "parsing0"])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_fixtures(A, case, key):
    parsing, skeleton, sq, num, want = fixture(A, case, key)
    p, s, q = (torch.from_numpy(a.copy()).cuda() for a in (parsing, skeleton, sq))
    keep = [t.clone() for t in (p, s, q)]
    first = A.branch_stats(p, s, num, q)
    same_tables(first, want)
    again = A.branch_stats(p, s, None, q)                    # num from the volume; a second call gives the same bits
    for k in mo.INT_TABLES:
        assert np.array_equal(first[k], again[k]), k
    assert all(torch.equal(a, b) for a, b in zip((p, s, q), keep))
    host = [a.copy() for a in (parsing, skeleton, sq)]
    from_numpy = A.branch_stats(host[0], host[1], num, host[2])      # numpy in, numpy out
    assert all(isinstance(v, np.ndarray) for v in from_numpy.values())
    assert all(np.array_equal(a, b) for a, b in zip(host, (parsing, skeleton, sq)))
    same_tables(from_numpy, want)
    rows = mo.rows_from_one(want)

    table = A.branch_morphometry(p, s, SPACING, num, q)
    assert all(torch.equal(a, b) for a, b in zip((p, s, q), keep))
    for k in mo.INT_TABLES:
        assert np.array_equal(getattr(table, k), rows[k]), k
    derived = mo.derived(rows, SPACING)
    for k in mo.FLOAT_COLUMNS:
        assert getattr(table, k).dtype == np.float64
        np.testing.assert_allclose(getattr(table, k), derived[k], rtol=RTOL, atol=0, equal_nan=True, err_msg=k)
    parent, generation, n_children = mo.branch_tree(rows["voxels"].tolist(), mo.adjacency(parsing, num))
    assert np.array_equal(table.parent, parent) and np.array_equal(table.generation, generation)
    assert np.array_equal(table.n_children, n_children)
    assert table.n_branches == int((rows["voxels"] > 0).sum()) and table.max_generation == int(generation.max())
    assert table.n_leaves == int(((generation >= 0) & (n_children == 0)).sum())
    assert table.total_length == pytest.approx(float(derived["length"].sum()), rel=RTOL)
    assert table.branches_per_generation.tolist() == np.bincount(generation[generation >= 0]).tolist()


# ---- edge shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num", [3, 700])                  # 700: labels that share a slot of the volume pass's LDS table (k and k + 256)
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_edge_shapes_random_labels(A, shape, num):
    rng = np.random.default_rng(sum(shape) + num)
    parsing = rng.integers(0, num + 1, shape).astype(np.int32)
    skeleton = (rng.random(shape) < 0.5).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)     # any non-zero byte is set
    sqdist = rng.integers(0, 1000, shape).astype(np.int32)
    check(A, parsing, skeleton, num, sqdist)
    got = check(A, parsing, skeleton, num, None)
    assert not got["r2_sum"].any() and np.all(got["r2_min"] == mo.INT32_MAX) and np.all(got["r2_max"] == -1)


@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_edge_shapes_block_labels(A, shape):
    num = 3
    n = int(np.prod(shape))
    parsing = (1 + (np.arange(n) // 100) % num).astype(np.int32).reshape(shape)      # runs of 100 across rows, planes and waves
    rng = np.random.default_rng(n)
    skeleton = (rng.random(shape) < 0.6).astype(np.uint8)
    check(A, parsing, skeleton, num, rng.integers(0, 1000, shape).astype(np.int32))
    check(A, parsing, np.ones(shape, np.uint8), num, None)


@pytest.mark.parametrize("shape", [(2, 3, 67), (3, 40, 130)])
def test_skeleton_at_any_address(A, shape):
    """The skeleton pass loads 16 aligned bytes per lane; a skeleton that starts at another address is read from its first byte on."""
    rng = np.random.default_rng(sum(shape))
    num = 5
    n = int(np.prod(shape))
    parsing = rng.integers(0, num + 1, shape).astype(np.int32)
    skeleton = (rng.random(shape) < 0.5).astype(np.uint8)
    skeleton.reshape(-1)[[0, -1]] = 1
    parsing.reshape(-1)[[0, -1]] = 3
    sqdist = rng.integers(0, 1000, shape).astype(np.int32)
    want, _ = mo.branch_stats(parsing, skeleton, num, sqdist)
    p, q = torch.from_numpy(parsing).cuda(), torch.from_numpy(sqdist).cuda()
    for skew in (1, 5, 8, 15):
        room = torch.full((n + 32,), 255, dtype=torch.uint8, device="cuda")     # set bytes on both sides of the volume
        view = room[skew:skew + n].view(shape)
        view.copy_(torch.from_numpy(skeleton))
        assert view.data_ptr() % 16 == skew and view.is_contiguous()
        same_tables(A.branch_stats(p, view, num, q), want)


def test_more_than_one_sweep_of_the_skeleton_pass(A):
    shape = (65, 512, 512)                                   # 17 039 360 voxels, more than 4096 workgroups x 4096 bytes
    parsing = torch.zeros(shape, dtype=torch.int32, device="cuda")
    skeleton = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    parsing[0, 0, 0:3], parsing[64, 511, 500:512], parsing[64, 510, 511] = 1, 2, 2
    skeleton[0, 0, 0:3], skeleton[64, 511, 500:512], skeleton[64, 510, 511] = 1, 1, 1
    got = A.branch_stats(parsing, skeleton, 2)
    # by hand: a line of 3 and a line of 12 with one more voxel above its last one (a face link of class 2, no diagonal: shortcut)
    assert got["voxels"].tolist() == [3, 13] and got["skeleton_voxels"].tolist() == [3, 13]
    links = np.zeros((2, 13), dtype=np.int64)
    links[0, 0], links[1, 0], links[1, 2] = 2, 11, 1
    assert np.array_equal(got["links"], links) and not got["cross_links"].any()
    assert got["coord_sum"].tolist() == [[0, 0, 3], [13 * 64, 12 * 511 + 510, sum(range(500, 512)) + 511]]
    assert got["box_min"].tolist() == [[0, 0, 0], [64, 510, 500]] and got["box_max"].tolist() == [[0, 0, 2], [64, 511, 511]]


# ---- links ------------------------------------------------------------------------------------------------------------------------
def test_straight_lines_touching_the_faces(A):
    m = 5
    for c, d in enumerate(mo.OFFSETS):
        v = np.zeros((m, m, m), dtype=np.int32)
        start = [0 if d[a] >= 0 else m - 1 for a in range(3)]
        for t in range(m):
            v[tuple(start[a] + t * d[a] for a in range(3))] = 1
        got = check(A, v, v.astype(np.uint8), 1)
        want = np.zeros(13, dtype=np.int64)
        want[c] = m - 1
        assert np.array_equal(got["links"][0], want) and not got["cross_links"].any()


def test_corners_cross_links_and_label_zero(A):
    v = np.zeros((3, 3, 3), dtype=np.int32)
    v[1, 1, 0] = v[1, 1, 1] = v[1, 2, 1] = 1                 # the L-corner: 2 links, not 3
    assert check(A, v, v.astype(np.uint8), 1)["links"].sum() == 2
    v = np.zeros((3, 3, 3), dtype=np.int32)
    v[0, 0, 0] = v[1, 1, 1] = 1
    assert check(A, v, v.astype(np.uint8), 2)["links"][0, 12] == 1
    v[0, 1, 1] = 2                                           # an intermediate voxel of another label drops the corner diagonal
    got = check(A, v, (v > 0).astype(np.uint8), 2)
    assert got["links"].sum() == 0 and got["cross_links"].sum(axis=1).tolist() == [2, 2]
    v = np.zeros((1, 2, 70), dtype=np.int32)                 # two labels meet along a line that crosses a wave end
    v[0, 0, 3:64], v[0, 0, 64:69] = 1, 2
    sk = (v > 0).astype(np.uint8)
    sk[0, 1, 10:20] = 1                                      # skeleton voxels on label 0 are ignored
    got = check(A, v, sk, 2)
    assert got["links"][:, 0].tolist() == [60, 4] and got["cross_links"][:, 0].tolist() == [1, 1]
    assert got["skeleton_voxels"].tolist() == [61, 5]


# ---- labels -------------------------------------------------------------------------------------------------------------------------
def test_label_range(A):
    zeros = np.zeros((2, 3, 67), dtype=np.int32)
    got = A.branch_stats(zeros, np.ones(zeros.shape, np.uint8), 0)
    assert all(v.shape[0] == 0 for v in got.values())
    assert A.branch_stats(zeros, np.ones(zeros.shape, np.uint8))["voxels"].shape == (0,)
    t = A.branch_morphometry(zeros)
    assert (t.num, t.n_branches, t.max_generation, t.total_length) == (0, 0, -1, 0.0)

    v = zeros.copy()                                         # labels missing in the middle of the range keep the empty values
    v[0, 1, 5:30], v[1, 2, 60:], v[1, 0, 0] = 2, 4095, 9
    sk = np.ones(v.shape, np.uint8)
    got = check(A, v, sk, 4095, np.full(v.shape, 7, np.int32))
    assert got["voxels"][[1, 8, 4094]].tolist() == [25, 1, 7] and got["voxels"].sum() == 33
    assert got["box_min"][2].tolist() == [2, 3, 67] and got["box_max"][2].tolist() == [-1, -1, -1]
    assert got["r2_min"][2] == mo.INT32_MAX and got["r2_max"][2] == -1 and got["r2_min"][4094] == 7
    assert got["box_min"][4094].tolist() == [1, 2, 60] and got["box_max"][4094].tolist() == [1, 2, 66]

    with pytest.raises(ValueError):
        A.branch_stats(v, sk, 4096)
    with pytest.raises(ValueError):
        A.branch_stats(v, sk, 4094)                          # a label above num
    w = v.copy()
    w[0, 0, 0] = -1
    with pytest.raises(ValueError):
        A.branch_stats(w, sk, 4095)
    with pytest.raises(ValueError):
        A.branch_stats(v, sk[:, :, :60], 4095)
    with pytest.raises(ValueError):
        A.branch_stats(v, sk, 4095, np.zeros((2, 3, 66), np.int32))
    with pytest.raises(ValueError):
        A.branch_morphometry(v, sk, SPACING, 4096)


# ---- 64-bit sums; also the single-label contention case and more than one sweep of both grids --------------------------------------
def test_sums_beyond_32_bits(A):
    n0, n1, n2 = 9, 64, 4096
    parsing = torch.ones((n0, n1, n2), dtype=torch.int32, device="cuda")
    skeleton = torch.ones((n0, n1, n2), dtype=torch.uint8, device="cuda")
    sqdist = torch.full((n0, n1, n2), 2 ** 20, dtype=torch.int32, device="cuda")
    got = A.branch_stats(parsing, skeleton, 1, sqdist)
    n = n0 * n1 * n2
    # closed forms of the definition for a full box of one label (the oracle's arrays would take seconds at this size)
    assert got["voxels"].tolist() == [n] and got["skeleton_voxels"].tolist() == [n]
    sums = [n1 * n2 * (n0 * (n0 - 1) // 2), n0 * n2 * (n1 * (n1 - 1) // 2), n0 * n1 * (n2 * (n2 - 1) // 2)]
    assert sums[2] > 2 ** 32 and got["coord_sum"].tolist() == [sums]
    assert got["box_min"].tolist() == [[0, 0, 0]] and got["box_max"].tolist() == [[n0 - 1, n1 - 1, n2 - 1]]
    links = [0] * 13                                         # every diagonal has an occupied intermediate voxel: face links only
    links[0], links[2], links[8] = n0 * n1 * (n2 - 1), n0 * (n1 - 1) * n2, (n0 - 1) * n1 * n2
    assert got["links"].tolist() == [links] and not got["cross_links"].any()
    assert got["r2_sum"].tolist() == [n * 2 ** 20] and n * 2 ** 20 > 2 ** 41
    assert got["r2_min"].tolist() == [2 ** 20] and got["r2_max"].tolist() == [2 ** 20]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_y_tree(A):
    label = so.make_case("tree")                             # the synthetic Y tree of the skeleton tests' stamps
    lab = torch.from_numpy(label).cuda()
    skel = A.skeletonize_3d(lab)
    parsing, num = A.tree_parsing(lab, skel, return_num=True)
    t = A.branch_morphometry(parsing, skel, SPACING)
    same = A.branch_morphometry(parsing, spacing=SPACING)    # the defaults thin parsing != 0 and take its squared EDT
    for k in mo.INT_TABLES:
        assert np.array_equal(getattr(t, k), getattr(same, k)), k
    p, s = parsing.cpu().numpy(), skel.cpu().numpy()
    inside = (s != 0) & (p > 0)
    assert t.num == num == int(p.max())
    assert t.voxels.sum() == int(label.sum())
    assert t.skeleton_voxels.sum() == int(inside.sum())
    assert t.links.sum() + t.cross_links.sum() // 2 == mo.total_links(inside)
    root = int(np.argmax(t.voxels))
    assert t.generation[root] == 0 and t.parent[root] == 0
    for k in range(t.num):
        if t.voxels[k] > 0 and k != root:
            assert t.parent[k] >= 1 and t.generation[k] == t.generation[t.parent[k] - 1] + 1, k
    assert t.n_leaves >= 2 and t.total_length > 0 and t.n_branches == int((t.voxels > 0).sum())
    assert np.all(t.radius_inscribed_min[t.skeleton_voxels > 0] >= 1.0)          # a skeleton voxel lies inside the label
