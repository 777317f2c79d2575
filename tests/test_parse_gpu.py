"""GPU airway tree parsing (csrc/parse.hip through seunet_amd.prep) against the reference's recorded results
(tests/golden/parse_known.npz) and tests/parse_oracle.py: every stage bitwise, the kernel edges at the smallest shapes that
reach them, the errors, and the chain into evaluation_case."""
import os

import numpy as np
import pytest
import torch

import parse_oracle as po
import skeleton_oracle as so

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "parse_known.npz"))
    return [{k[len(f"case{i}_"):]: z[k] for k in z.files if k.startswith(f"case{i}_")} for i in range(int(z["ncase"]))]


CASES = _cases()
IDS = range(len(CASES))


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("ci", IDS)
def test_skeleton_parsing_equals_the_reference(A, ci):
    c = CASES[ci]
    t = dev(c["skeleton"])
    before = t.clone()
    parse, cd, num = A.skeleton_parsing(t)
    assert parse.dtype == torch.uint8 and cd.dtype == torch.int32 and parse.device == t.device
    assert torch.equal(t, before)
    assert num == int(c["num0"])
    assert np.array_equal(host(parse), c["skeleton_parse"])
    assert np.array_equal(host(cd), c["cd"].astype(np.int32))
    again = A.skeleton_parsing(t)
    assert torch.equal(again[0], parse) and torch.equal(again[1], cd) and again[2] == num


@pytest.mark.parametrize("ci", IDS)
def test_tree_parsing_func_equals_the_reference(A, ci):
    c = CASES[ci]
    args = [dev(c["skeleton_parse"]), dev(c["label"]), dev(c["cd"].astype(np.int32))]
    before = [a.clone() for a in args]
    got = A.tree_parsing_func(*args)
    assert got.dtype == torch.int32 and tuple(got.shape) == c["label"].shape
    assert all(torch.equal(a, b) for a, b in zip(args, before))
    assert np.array_equal(host(got), c["parsing0"].astype(np.int32))
    assert torch.equal(A.tree_parsing_func(*args), got)
    as_numpy = A.tree_parsing_func(c["skeleton_parse"], c["label"], c["cd"])
    assert isinstance(as_numpy, np.ndarray) and np.array_equal(as_numpy, c["parsing0"])


@pytest.mark.parametrize("ci", IDS)
def test_label_adjacency_equals_the_reference(A, ci):
    c = CASES[ci]
    counts, ad = A.label_adjacency(dev(c["parsing0"].astype(np.int32)), int(c["num0"]))
    assert counts.dtype == np.int64 and ad.dtype == np.uint8
    assert np.array_equal(counts, c["counts0"]) and np.array_equal(ad, c["ad0"])
    assert int(np.argsort(counts.astype(np.float64))[-1]) + 1 == int(c["trachea0"])


@pytest.mark.parametrize("ci", IDS)
def test_tree_parsing_equals_the_reference(A, ci):
    c = CASES[ci]
    label, skeleton = dev(c["label"]), dev(c["skeleton"])
    before = label.clone(), skeleton.clone()
    got, num = A.tree_parsing(label, skeleton, return_num=True)
    assert got.dtype == torch.int32 and num == int(c["num"])
    assert np.array_equal(host(got), c["parsing"].astype(np.int32))
    assert torch.equal(label, before[0]) and torch.equal(skeleton, before[1])
    assert torch.equal(A.tree_parsing(label, skeleton), got)
    plain, num0 = A.tree_parsing(label, skeleton, refine=False, return_num=True)
    assert num0 == int(c["num0"]) and np.array_equal(host(plain), c["parsing0"].astype(np.int32))


def test_faces_edges_and_corners_see_the_mirror(A):
    """Skeleton voxels on every face, edge and corner of 7x9x70; the last axis crosses a 64-voxel span."""
    rng = np.random.default_rng(3)
    v = (rng.random((7, 9, 70)) < 0.01).astype(np.uint8)
    for i0 in (0, 6):
        for i1 in (0, 8):
            v[i0, i1, 5:66] = 1                                    # four edges along the last axis, across voxel 63 / 64
            v[i0, i1, 0] = v[i0, i1, 69] = 1                        # the corners
    v[0, 2:7, 20] = v[6, 4, 30:50] = v[3, 0, 2:30] = v[2, 8, 40:69] = v[1:6, 4, 0] = v[2, 2:8, 69] = 1   # lines in the six faces
    v[0, 0:9, 0] = v[0:7, 8, 69] = 1                                # edges along the other two axes
    v[0:5, 2, 10] = v[2:7, 6, 25] = v[3, 0:6, 35] = v[4, 3:9, 55] = v[2, 2, 0:7] = v[4, 6, 60:70] = 1   # lines that end on a face
    want = po.skeleton_parsing(v)
    assert want[2] >= 3 and not np.array_equal(want[1], po.skeleton_parsing(v, mode="constant")[1])
    parse, cd, num = A.skeleton_parsing(dev(v))
    assert num == want[2] and np.array_equal(host(cd), want[1]) and np.array_equal(host(parse), want[0])


def test_small_components_and_the_second_numbering(A):
    v = np.zeros((8, 9, 20), np.uint8)
    v[1, 1, 1:4] = 1          # 3 voxels, first in raster order: takes number 1 in the first labelling and goes
    v[1, 4, 2:6] = 1          # exactly 4: goes
    v[3, 2, 1:6] = 1          # exactly 5: stays, and is number 1 of the second labelling
    v[5, 5, 3:15] = 1         # number 2
    parse, cd, num = A.skeleton_parsing(dev(v))
    cd = host(cd)
    assert num == 2 and (cd[3, 2, 1:6] == 1).all() and (cd[5, 5, 3:15] == 2).all() and int((cd != 0).sum()) == 17
    want = po.skeleton_parsing(v)
    assert np.array_equal(cd, want[1]) and np.array_equal(host(parse), want[0])
    _, cd4, num4 = A.skeleton_parsing(dev(v), min_voxels=4)
    assert num4 == 3 and np.array_equal(host(cd4), po.skeleton_parsing(v, min_voxels=4)[1])


@pytest.fixture(scope="module")
def blocks():
    """40^3 cut into 4x4x3 blocks (about 1400) with labels up to beyond 1024, every eighth number unused, some voxels zero."""
    i0, i1, i2 = np.meshgrid(np.arange(40), np.arange(40), np.arange(40), indexing="ij")
    idx = ((i0 // 4) * 10 + i1 // 4) * 14 + i2 // 3
    vol = (1 + idx + idx // 7).astype(np.int32)
    vol[np.random.default_rng(11).random(vol.shape) < 0.1] = 0
    num = int(vol.max()) + 5
    counts = np.bincount(vol.ravel(), minlength=num + 1)[1:].astype(np.int64)
    ad = np.zeros((num, num), np.uint8)
    for ax in range(3):
        a = np.moveaxis(vol, ax, 0)[:-1].ravel()
        b = np.moveaxis(vol, ax, 0)[1:].ravel()
        m = (a > 0) & (b > 0) & (a != b)
        ad[a[m] - 1, b[m] - 1] = 1
        ad[b[m] - 1, a[m] - 1] = 1
    return vol, num, counts, ad


def test_label_adjacency_with_many_labels(A, blocks):
    vol, num, want_counts, want_ad = blocks
    assert num > 1024 and (want_counts == 0).any() and (num + 1 + 63) // 64 > 16
    counts, ad = A.label_adjacency(dev(vol), num)
    assert np.array_equal(counts, want_counts) and np.array_equal(ad, want_ad)
    assert np.array_equal(ad, ad.T) and not ad.diagonal().any()
    counts2, ad2 = A.label_adjacency(vol, num)                      # numpy in
    assert np.array_equal(counts2, want_counts) and np.array_equal(ad2, want_ad)


def test_relabel(A, blocks):
    vol, num, _, _ = blocks
    lut = np.random.default_rng(5).integers(0, 3000, num + 1).astype(np.int32)
    t = dev(vol)
    got = A.relabel(t, lut)
    assert got.dtype == torch.int32 and np.array_equal(host(got), lut[vol]) and np.array_equal(host(t), vol)
    assert np.array_equal(A.relabel(vol, lut), lut[vol])


def test_single_voxel_thick_volume(A):
    """n0 = 1: the mirror along axis 0 triples every sum, so skeleton_parsing removes everything (as the reference does); the
    other stages are checked on branches numbered by hand."""
    skel = np.zeros((1, 30, 70), np.uint8)
    skel[0, 15, 2:68] = 1
    skel[0, 3:13, 30] = 1
    skel[0, 18:28, 40] = 1
    skel[0, 25, 5:8] = 1
    label = np.zeros_like(skel)
    label[0, 1:29, 1:69] = 1
    want = po.skeleton_parsing(skel)
    parse, cd, num = A.skeleton_parsing(dev(skel))
    assert num == want[2] == 0 and not host(cd).any() and not host(parse).any()
    cd = np.zeros(skel.shape, np.int32)
    cd[0, 15, 2:68], cd[0, 3:13, 30], cd[0, 18:28, 40], cd[0, 25, 5:8] = 2, 1, 3, 4
    want = po.tree_parsing_func(skel, label, cd)
    got = A.tree_parsing_func(dev(skel), dev(label), dev(cd))
    assert np.array_equal(host(got), want) and len(np.unique(want)) == 5
    counts, ad = A.label_adjacency(got, 4)
    assert np.array_equal(counts, po.label_counts(want, 4)) and np.array_equal(ad, po.adjacent_map(want, 4)) and ad.any()


def test_errors(A):
    z8 = torch.zeros((4, 5, 6), dtype=torch.uint8, device="cuda")
    z32 = torch.zeros((4, 5, 6), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="empty"):
        A.tree_parsing_func(z8, z8 + 1, z32)
    with pytest.raises(ValueError):
        A.tree_parsing(z8 + 1, z8)
    with pytest.raises(ValueError, match="4095"):
        A.label_adjacency(z32, 5000)
    with pytest.raises(ValueError, match="outside"):
        A.label_adjacency(z32 + 7, 6)
    flat8 = torch.zeros((4, 4), dtype=torch.uint8, device="cuda")
    for call in (lambda: A.skeleton_parsing(flat8), lambda: A.skeleton_parsing(np.zeros((4, 4))), lambda: A.tree_parsing(flat8),
                 lambda: A.tree_parsing_func(flat8, flat8, flat8.int()), lambda: A.label_adjacency(flat8.int(), 3)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: A.skeleton_parsing(z8.cpu()), lambda: A.tree_parsing(z8.cpu()), lambda: A.tree_parsing_func(z8.cpu(), z8, z32),
                 lambda: A.label_adjacency(z32.cpu(), 3)):
        with pytest.raises(RuntimeError):
            call()


def test_chain_from_the_label_to_the_metrics(A):
    import components_oracle as co
    v, skel, _ = so.solved("tree")
    label = dev(v)
    skeleton = A.skeletonize_3d(label)
    assert np.array_equal(host(skeleton), skel)
    parsing = A.tree_parsing(label)
    assert torch.equal(parsing, A.tree_parsing(label, skeleton))
    want = po.tree_parsing(v, skel)
    assert np.array_equal(host(parsing), want["parsing"])
    pred = v.copy()
    pred[:, :, 100:] = 0
    got = A.evaluation_case(dev(pred), label, skeleton, parsing)
    assert tuple(got) == tuple(co.evaluation_case(pred, v, skel, want["parsing"]))
