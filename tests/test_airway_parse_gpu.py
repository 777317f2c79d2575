"""``airway_parse`` on the GPU: the dense stages against scipy, bitwise, and the whole call against
tests/golden/topology_known.npz (the reference's own functions with stable sorts, scripts/make_golden_topology.py)."""
import os

import numpy as np
import pytest
import torch

import skeleton_oracle as so

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z = np.load(os.path.join(GOLDEN, "topology_known.npz"))
NCASE = int(Z["ncase"])
FLAT_KEYS = ("index", "fatherindex", "start", "has_end", "end", "member_count", "members")
# (2, 3, 1) and (1, 2, 64): one word per row with and without a tail, and fewer words than one workgroup of the pack holds
MORPH_SHAPES = [(1, 1, 1), (1, 1, 70), (3, 4, 5), (5, 6, 64), (4, 5, 65), (7, 9, 129), (20, 24, 134), (2, 3, 1), (1, 2, 64)]


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def case(ci):
    p = f"case{ci}_"
    return {k[len(p):]: Z[k] for k in Z.files if k.startswith(p)}


def scipy_ops():
    from scipy import ndimage
    return {"dilate": lambda v: ndimage.binary_dilation(v),
            "erode0": lambda v: ndimage.binary_erosion(v),
            "erode1": lambda v: ndimage.binary_erosion(v, border_value=1),
            "close": lambda v: ndimage.binary_erosion(ndimage.binary_dilation(v), border_value=1)}


def gpu_ops(A):
    return {"dilate": A.binary_dilation, "erode0": lambda v: A.binary_erosion(v, border_value=0),
            "erode1": lambda v: A.binary_erosion(v, border_value=1), "close": A.binary_closing}


def check_morphology(A, v):
    want, got = scipy_ops(), gpu_ops(A)
    t = torch.from_numpy(v).cuda()
    for name in want:
        out = got[name](t)
        assert out.dtype == torch.uint8 and out.shape == t.shape
        assert np.array_equal(out.cpu().numpy(), want[name](v).astype(np.uint8)), (name, v.shape)
        assert torch.equal(got[name](t), out), name                                   # two runs equal
    assert np.array_equal(t.cpu().numpy(), v)                                         # the input is unchanged
    assert torch.equal(A.binary_closing(t), A.binary_erosion(A.binary_dilation(t), border_value=1))


@pytest.mark.parametrize("shape", MORPH_SHAPES)
def test_morphology_is_scipys(A, shape):
    rng = np.random.default_rng(sum(shape))
    for fill in (0.05, 0.5, 0.95):
        check_morphology(A, (rng.random(shape) < fill).astype(np.uint8))
    check_morphology(A, np.zeros(shape, np.uint8))
    check_morphology(A, np.ones(shape, np.uint8))


def test_morphology_of_single_voxels(A):
    """One voxel on, and one voxel off, at bits 0, 63, 64 and n2 - 1 of a row and on each face of the volume."""
    shape = (4, 5, 130)
    spots = [(1, 2, 0), (1, 2, 63), (1, 2, 64), (1, 2, 129), (0, 2, 70), (3, 2, 70), (1, 0, 70), (1, 4, 70), (2, 2, 70)]
    for p in spots:
        v = np.zeros(shape, np.uint8)
        v[p] = 1
        check_morphology(A, v)
        check_morphology(A, 1 - v)


def test_morphology_takes_non_zero_as_one_and_numpy(A):
    v = (np.random.default_rng(3).random((5, 6, 70)) < 0.3).astype(np.uint8) * 7
    from scipy import ndimage
    out = A.binary_dilation(v)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8
    assert np.array_equal(out, ndimage.binary_dilation(v != 0).astype(np.uint8))
    assert np.array_equal(A.binary_dilation(torch.from_numpy(v).cuda()).cpu().numpy(), out)


def _cube_shell(n, lo, hi):
    v = np.zeros((n, n, n), np.uint8)
    v[lo:hi, lo:hi, lo:hi] = 1
    v[lo + 1:hi - 1, lo + 1:hi - 1, lo + 1:hi - 1] = 0
    return v


def fill_cases():
    cases = {"shell": so.make_case("shell")}
    open_face = np.zeros((8, 9, 10), np.uint8)                  # a box whose cavity lies in face i0 = 0: not a hole
    open_face[0:6, 2:8, 2:9] = 1
    open_face[0:5, 3:7, 3:8] = 0
    cases["cavity_on_a_face"] = open_face
    thick = np.zeros((11, 11, 11), np.uint8)                    # walls two voxels thick; the gap through them is diagonal only
    thick[1:10, 1:10, 1:10] = 1
    thick[3:8, 3:8, 3:8] = 0
    thick[2, 5, 5] = 0                                          # inner layer of the wall i0 = 1..2
    thick[1, 6, 5] = 0                                          # outer layer, one step aside: they share an edge, not a face
    cases["diagonal_gap"] = thick
    nested = _cube_shell(15, 1, 14)
    nested |= _cube_shell(15, 4, 11)
    nested[7, 7, 7] = 1
    cases["nested"] = nested
    cases["zero"] = np.zeros((3, 4, 70), np.uint8)
    return cases


@pytest.mark.parametrize("name", list(fill_cases()))
def test_fill_holes_is_scipys(A, name):
    from scipy import ndimage
    v = fill_cases()[name]
    want = ndimage.binary_fill_holes(v).astype(np.uint8)
    t = torch.from_numpy(v).cuda()
    got = A.binary_fill_holes(t)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(t.cpu().numpy(), v) and torch.equal(A.binary_fill_holes(t), got)
    if name == "cavity_on_a_face":
        assert np.array_equal(want, v)                          # nothing is filled
    if name == "diagonal_gap":
        assert want[3:8, 3:8, 3:8].all() and want[2, 5, 5] == 1 and want[1, 6, 5] == 0
    if name in ("shell", "nested"):
        assert want.sum() > v.sum()


@pytest.mark.parametrize("kind", ["sparse", "dense", "blobs"])
@pytest.mark.parametrize("shape", [(9, 8, 63), (9, 8, 65), (17, 5, 130)])
def test_maximum_3d_is_unchanged(A, shape, kind):
    import components_oracle as co
    from test_components_gpu import _volume
    v = _volume(kind, shape, 31 * sum(shape) + len(kind))
    try:
        want = co.maximum_3d(v)
    except IndexError:
        with pytest.raises(IndexError):
            A.maximum_3d(v)
        return
    assert np.array_equal(A.maximum_3d(v), want)


def test_large_connected_domain26_is_unchanged(A):
    gold = np.load(os.path.join(GOLDEN, "lung_known.npz"))
    for key in ("e", "e2"):
        assert np.array_equal(A.large_connected_domain26(gold[f"{key}_label"]), gold[f"{key}_ldc"])


def test_slice_moments_are_numpys(A):
    v = (np.random.default_rng(11).random((9, 13, 70)) < 0.4).astype(np.uint8)
    v[:, :, 33] = 0
    t = torch.from_numpy(v).cuda()
    for k in (0, 69, 33, 64):
        i0, i1 = np.nonzero(v[:, :, k])
        assert A.prep.slice_moments(t, k) == (len(i0), int(i0.sum()), int(i1.sum())), k
    assert A.prep.slice_moments(t, 33) == (0, 0, 0)
    big = np.ones((300, 301, 2), np.uint8)                      # more than one block, sums past 2^24
    i0, i1 = np.nonzero(big[:, :, 1])
    assert A.prep.slice_moments(big, 1) == (len(i0), int(i0.sum()), int(i1.sum()))
    with pytest.raises(ValueError):
        A.prep.slice_moments(t, 70)


def test_scatter_labels(A):
    shape = (3, 4, 70)
    n = int(np.prod(shape))
    rng = np.random.default_rng(5)
    lin = rng.permutation(n)[:300].astype(np.int64)
    val = rng.integers(1, 400, 300).astype(np.int32)
    cd, parse = A.prep.scatter_labels(lin, val, shape)
    want = np.zeros(n, np.int32)
    want[lin] = val
    assert cd.dtype == torch.int32 and parse.dtype == torch.uint8
    assert np.array_equal(cd.cpu().numpy().ravel(), want) and np.array_equal(parse.cpu().numpy().ravel(), (want != 0).astype(np.uint8))
    for bad in (n, -1, 1 << 40):
        with pytest.raises(ValueError, match="outside the volume"):
            A.prep.scatter_labels(np.append(lin, bad), np.append(val, 9), shape)
    cd, parse = A.prep.scatter_labels(np.zeros(0, np.int64), np.zeros(0, np.int32), shape)
    assert int(cd.abs().sum()) == 0 and int(parse.sum()) == 0


def assert_table(A, got, rec, name):
    flat = A.topology.flatten(got)
    for k in FLAT_KEYS:
        assert np.array_equal(flat[k], rec[f"{name}_{k}"]), (name, k)


@pytest.mark.parametrize("ci", range(NCASE))
def test_airway_parse_stage_by_stage(A, ci):
    r = case(ci)
    label = torch.from_numpy((r["label"] != 0).astype(np.uint8)).cuda()
    before = label.clone()
    st = A.prep.airway_parse_stages(label)
    assert st["order"] == int(r["order"])
    assert np.array_equal(st["label_trans"].cpu().numpy(), r["label_trans"])
    assert np.array_equal(st["skeleton"].cpu().numpy(), r["skeleton"])
    assert np.array_equal(st["B0"], r["B0"]) and np.array_equal(st["B"], r["B"]) and st["mainpart"] == int(r["mainpart"])
    assert np.array_equal(st["basev"].view(np.int64), r["basev"].view(np.int64))
    assert_table(A, st["table1"], r, "table1")
    assert_table(A, st["merged"], r, "merged")
    assert [c for c, _ in st["codes"]] == list(r["codes"]) and [f for _, f in st["codes"]] == list(r["father_codes"])
    assert np.array_equal(st["cd"].cpu().numpy(), r["cd"].astype(np.int32))
    assert np.array_equal(st["skeleton_parse"].cpu().numpy(), (r["cd"] != 0).astype(np.uint8))
    assert st["parsing"].dtype == torch.int32 and np.array_equal(st["parsing"].cpu().numpy(), r["parsing"].astype(np.int32))
    assert torch.equal(label, before)


@pytest.mark.parametrize("ci", range(NCASE))
def test_airway_parse_public_call(A, ci):
    r = case(ci)
    want = r["parsing"].astype(np.int32)
    got, branches = A.airway_parse(r["label"], return_branches=True)              # numpy in (int16, any non-zero) -> numpy out
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want)
    assert len(branches) == len(r["merged_index"]) == int(want.max())
    assert [b["grade"] for b in branches] == list(r["codes"]) and [b["father_grade"] for b in branches] == list(r["father_codes"])
    assert [b["index"] for b in branches] == list(r["merged_index"])
    t = torch.from_numpy((r["label"] != 0).astype(np.uint8) * 3).cuda()            # tensor in -> tensor out; non-zero counts as 1
    out = A.airway_parse(t, merge_t=5)
    assert isinstance(out, torch.Tensor) and out.is_cuda and np.array_equal(out.cpu().numpy(), want)
    # the result is the `parsing` argument of evaluation_case
    label = (r["label"] != 0).astype(np.uint8)
    td, bd, dsc, pre, sen, spe = A.evaluation_case(label, label, r["skeleton"], got)
    assert all(np.isfinite(v) for v in (td, bd, dsc, pre, sen, spe)) and 0.0 <= bd <= 100.0 and dsc == 100.0


def test_airway_parse_errors_name_their_stage(A):
    with pytest.raises(ValueError, match="orientation.*empty"):
        A.airway_parse(np.zeros((5, 6, 70), np.uint8))
    rod = np.zeros((9, 9, 40), np.uint8)                        # one straight rod: a single branch
    rod[3:6, 3:6, 2:38] = 1
    with pytest.raises(ValueError, match="grade"):
        A.airway_parse(rod)
