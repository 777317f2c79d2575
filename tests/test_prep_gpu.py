"""Stage-2/3 preparation on the GPU (csrc/edt.hip through se-unet-airseg_amd/prep.py) against the reference: scipy's EDT and
feature transform on tie-heavy volumes, and lib_weight / save_weight_break / the crop candidate statements run from the
reference's own source (tests/golden/prep_known.npz, scripts/make_golden_prep.py).  Integer and index work and the IEEE
float chains are compared bitwise (float16 / float64 through integer views)."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "prep_known.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_edt_bitwise_on_fixture_volumes(A, g):
    for i in range(int(g["nedt"])):
        vol = g[f"edt{i}_vol"]
        sq, dist, ind = A.distance_transform_edt(dev(vol), return_indices=True, return_sqdist=True)
        ref_ind = g[f"edt{i}_ind"].astype(np.int32)
        assert np.array_equal(ind.cpu().numpy(), ref_ind), i
        assert np.array_equal(dist.cpu().numpy().view(np.int64), g[f"edt{i}_dist"].view(np.int64)), i
        ref_sq = ((ref_ind - np.indices(vol.shape)).astype(np.int64) ** 2).sum(0)
        assert np.array_equal(sq.cpu().numpy(), ref_sq), i
        assert torch.equal(A.distance_transform_edt(dev(vol)), dist)


def test_device_sqrt_is_correctly_rounded():
    """A 1025^3 volume with one zero corner has every squared distance i^2 + j^2 + k^2 with i, j, k <= 1024: all integers up
    to 1024^2 that are squared distances at all (sums of three squares) and most of those up to 3 * 1024^2.  Every distance
    is compared with np.sqrt of its integer."""
    import seunet_amd as A
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 1025
    vol = torch.ones((n, n, n), dtype=torch.uint8, device="cuda")
    vol[0, 0, 0] = 0
    sq, dist = A.distance_transform_edt(vol, return_sqdist=True)
    del vol
    top = 3 * 1024 ** 2
    ref = torch.from_numpy(np.sqrt(np.arange(top + 1, dtype=np.float64))).cuda()
    sq = sq.view(-1).long()
    assert int(sq.max()) == top
    assert torch.equal(dist.view(-1).view(torch.int64), ref[sq].view(torch.int64))
    seen = torch.bincount(sq, minlength=top + 1).cpu().numpy() > 0
    k = np.arange(top + 1)
    m = k.copy()
    while True:                                   # Legendre: k is a sum of three squares unless k = 4^a (8b + 7)
        q = (m % 4 == 0) & (m > 0)
        if not q.any():
            break
        m[q] //= 4
    assert np.array_equal(seen[:1024 ** 2 + 1], (m % 8 != 7)[:1024 ** 2 + 1])
    assert seen.sum() > 0.75 * (top + 1)


def test_hard_mining_candidates_match_the_reference(A, g):
    for c in range(int(g["ncase"])):
        p = f"case{c}_"
        loc_skel, loc_small = A.hard_mining_candidates(dev(g[p + "label"]), dev(g[p + "skeleton"]), dev(g[p + "pred"]))
        for cs, key in ((loc_skel, "loc_skeleton"), (loc_small, "loc_small")):
            ref = np.where(g[p + key])
            assert len(cs[0]) == len(ref[0]), (c, key)
            for a, b in zip(cs.to_numpy(), ref):
                assert np.array_equal(a, b), (c, key)


def test_lib_weight_bitwise(A, g):
    for c in range(int(g["ncase"])):
        p = f"case{c}_"
        w = A.lib_weight(dev(g[p + "label"]))
        assert w.dtype == torch.float16
        assert np.array_equal(w.cpu().numpy().view(np.int16), g[p + "lib"].view(np.int16)), c


def test_break_weight_bitwise(A, g):
    for c in range(int(g["ncase"])):
        p = f"case{c}_"
        w, br = A.break_weight(dev(g[p + "label"]), dev(g[p + "pred"]), dev(g[p + "skeleton"]))
        assert np.array_equal(w.cpu().numpy().view(np.int16), g[p + "w_br"].view(np.int16)), c
        loc = A.CandidateSet.from_mask(br)
        ref = tuple(g[p + "loc_break"].astype(np.int64))
        assert len(loc[0]) == len(ref[0]), c
        for a, b in zip(loc.to_numpy(), ref):
            assert np.array_equal(a, b), c
        if bool(g[p + "maxf_zero"]):
            assert not bool(w.any()) and len(loc[0]) == 0


def test_from_case_samplers_equal_the_list_fed_ones(A, golden_dir):
    h = np.load(os.path.join(golden_dir, "pipeline_hm_known.npz"))
    img, label, skeleton = h["img"], h["label"], h["skeleton"]
    pred = h["pred"].astype(np.uint8)
    cube, b = int(h["cube"]), int(h["batch"])
    from scipy import ndimage                     # (as tests/test_pipeline_gpu.py builds the lists)
    dis = ndimage.distance_transform_edt(label)
    loc_skel, loc_small = np.where(skeleton * (1 - h["pred"])), np.where((dis * skeleton) < 2)
    br_skel = np.zeros(label.shape, np.uint8)
    br_skel[tuple(h["br_skel"])] = 1
    loc_break = np.where(br_skel == 1)
    d = {k: dev(v) for k, v in (("img", img), ("label", label), ("skel", skeleton), ("pred", pred), ("w2", h["weight16"]),
                                ("w3", h["weight3"]), ("br", br_skel))}
    pairs = [(A.AirwayHMDataGPU(d["img"], d["label"], d["w2"], loc_skel, loc_small, b, cube=cube),
              A.AirwayHMDataGPU.from_case(d["img"], d["label"], d["w2"], d["skel"], d["pred"], b, cube=cube)),
             (A.AirwayHMData3GPU(d["img"], d["label"], d["w3"], d["skel"], loc_skel, loc_small, loc_break, b, cube=cube),
              A.AirwayHMData3GPU.from_case(d["img"], d["label"], d["w3"], d["skel"], d["pred"], b, cube=cube, br_skel=d["br"]))]
    for old, new in pairs:
        for seed in (1, 2, 3):
            outs = []
            for ds in (old, new):
                random.seed(seed)
                np.random.seed(50 + seed)
                outs.append(ds.sample())
            assert outs[0]["kinds"] == outs[1]["kinds"]
            for k in outs[0]:
                if k != "kinds":
                    assert torch.equal(outs[0][k], outs[1][k]), k


def test_large_case_against_brute_force(A):
    shape = (300, 512, 512)
    gen = torch.Generator(device="cuda").manual_seed(7)
    vol = (torch.rand(shape, generator=gen, device="cuda") >= 2e-5).to(torch.uint8)
    vol[150, :, 256] = 0                                    # a line of sites and a plane of sites with ties around them
    vol[:, 40, :][::37, ::41] = 0
    sq, ind = A.distance_transform_edt(vol, return_distances=False, return_indices=True, return_sqdist=True)
    sq2, ind2 = A.distance_transform_edt(vol, return_distances=False, return_indices=True, return_sqdist=True)
    assert torch.equal(sq, sq2) and torch.equal(ind, ind2)
    zeros = (vol == 0).nonzero().long()                     # (m, 3)
    assert 1000 < zeros.shape[0] < 200000
    pick = torch.randint(0, vol.numel(), (256,), generator=gen, device="cuda")
    coords = torch.stack([pick // (512 * 512), (pick // 512) % 512, pick % 512], 1)
    brute = ((coords[:, None, :] - zeros[None, :, :]) ** 2).sum(-1).min(1).values
    assert torch.equal(sq.view(-1)[pick].long(), brute)
    grid = [torch.arange(s, device="cuda").view([-1 if i == a else 1 for i in range(3)]) for a, s in enumerate(shape)]
    idx = ind.long()
    assert bool((vol[idx[0], idx[1], idx[2]] == 0).all())
    d2 = sum((idx[a] - grid[a]) ** 2 for a in range(3))
    assert torch.equal(d2, sq.long())


def test_error_paths(A):
    with pytest.raises(ValueError, match="no zero voxel"):
        A.distance_transform_edt(torch.ones((4, 5, 6), dtype=torch.uint8, device="cuda"))
    big = torch.ones((32768, 1, 2), dtype=torch.uint8, device="cuda")
    big[0] = 0
    with pytest.raises(RuntimeError, match="32767"):
        A.distance_transform_edt(big)
    label = torch.zeros((6, 7, 8), dtype=torch.uint8, device="cuda")
    label[2:4, 2:5, 3:6] = 1
    with pytest.raises(ValueError, match="skeleton is empty"):
        A.break_weight(label, torch.zeros_like(label), torch.zeros_like(label))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        A.lib_weight(label.cpu())
