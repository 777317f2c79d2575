"""CT preprocessing on the device (seunet_amd.preprocess, csrc/lung.hip): bitwise against the reference's recorded values
(tests/golden/lung_known.npz) stage by stage, and against the restatement tests/lung_oracle.py on volumes made here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lung_oracle as LO  # noqa: E402
import seunet_amd as A  # noqa: E402
from seunet_amd import preprocess as P  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lung_known.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def counts_of(a):
    return np.bincount(a.ravel().view(np.uint16).astype(np.int64), minlength=65536)


@pytest.mark.parametrize("key", ("a", "b", "c"))
def test_fixture_stage_by_stage(gold, key):
    ct = gold[f"{key}_ct"]
    t = torch.from_numpy(ct).cuda()
    counts = P.value_counts(t, P.HU_SHIFT)
    assert np.array_equal(counts, counts_of((ct + np.int16(1024)).astype(np.int16)))
    h1 = P.histogram_from_counts(counts)
    assert np.array_equal(h1[0], gold[f"{key}_hist1_y"]) and np.array_equal(h1[1], gold[f"{key}_hist1_x"])
    aaa = float(gold[f"{key}_aaa"])
    aaa = None if np.isnan(aaa) else aaa
    cp = P._shift_clamp(t, aaa)
    T = float(gold[f"{key}_T"])
    assert A.th_2t(cp) == T
    L = A.get_l(cp, T)
    assert L.dtype == torch.uint8 and np.array_equal(L.cpu().numpy(), gold[f"{key}_L"])
    L1 = A.maximum_3d(L)
    assert np.array_equal(L1.cpu().numpy(), gold[f"{key}_L1"].astype(np.uint8))
    x = P._combine(L, L1, 0)
    assert np.array_equal(x.cpu().numpy(), gold[f"{key}_LxL1"].astype(np.uint8))
    L2 = A.maximum_3d(x)
    assert np.array_equal(L2.cpu().numpy(), gold[f"{key}_L2"].astype(np.uint8))
    mask = P._combine(L1, L2, 1)
    assert np.array_equal(mask.cpu().numpy(), gold[f"{key}_Mask"].astype(np.uint8))
    # the whole call, numpy in / numpy out and tensor in / tensor out
    data_cut, lung_mask, box = A.preprocess_ct(ct)
    assert data_cut.dtype == np.int16 and np.array_equal(data_cut, gold[f"{key}_data_cut"])
    assert lung_mask.dtype == np.uint8 and np.array_equal(lung_mask, gold[f"{key}_lung_mask"])
    assert box.dtype == np.int64 and np.array_equal(box, gold[f"{key}_box"])
    dt, lt, bt = A.preprocess_ct(t)
    assert dt.is_cuda and lt.is_cuda and np.array_equal(dt.cpu().numpy(), data_cut) and np.array_equal(lt.cpu().numpy(), lung_mask)
    assert np.array_equal(bt, box)


def test_fixture_prediction_mode(gold):
    cp, m, b = A.preprocess_ct(gold["d_ct"], mode="prediction")
    assert m is None and b is None
    assert cp.dtype == np.int16 and np.array_equal(cp, gold["d_data_cut"])


def test_fixture_no_lung_raises(gold):
    ct = gold["f_ct"]
    cp = (ct + np.int16(1024)).astype(np.int16)
    assert A.th_2t(cp) == float(gold["f_T"])
    assert not A.get_l(cp, float(gold["f_T"])).any()
    with pytest.raises(IndexError):
        A.preprocess_ct(ct)


def test_fixture_cut_mask(gold):
    for key in ("e", "e2"):
        assert np.array_equal(A.large_connected_domain26(gold[f"{key}_label"]), gold[f"{key}_ldc"])
        out = A.cut_mask(gold[f"{key}_label"], gold[f"{key}_box"])
        assert out.dtype == np.uint8 and np.array_equal(out, gold[f"{key}_mask_cut"])
    with pytest.raises(IndexError):
        A.large_connected_domain26(gold["e3_label"])
    with pytest.raises(IndexError):
        A.cut_mask(gold["e3_label"], gold["e3_box"])


def blob_volume(rng, shape, n_blobs, holes=True):
    """int16 slices of random rectangles and discs (many of equal size), with holes, holes at the border, diagonal contacts."""
    X, Y, Z = shape
    v = np.full(shape, -1000, np.int16)
    x, y = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    for z in range(Z):
        s = np.full((X, Y), -1000, np.int16)
        for _ in range(n_blobs):
            w, h = int(rng.choice([8, 12, 40, 60])), int(rng.choice([8, 12, 50, 70]))
            x0, y0 = int(rng.integers(-5, X - 5)), int(rng.integers(-5, Y - 5))
            s[max(x0, 0):x0 + w, max(y0, 0):y0 + h] = 40
            if holes and w > 20 and h > 20:
                hw, hh = w - 10, h - 10
                s[max(x0 + 5, 0):x0 + 5 + hw, max(y0 + 5, 0):y0 + 5 + hh] = -900 + int(rng.integers(0, 50))
        q = min(20, X // 4, Y // 4)
        for _ in range(3):                        # diagonal contacts: squares meeting at a corner
            c0, c1 = int(rng.integers(0, X - 2 * q)), int(rng.integers(0, Y - 2 * q))
            s[c0:c0 + q, c1:c1 + q] = -950
            s[c0 + q:c0 + 2 * q, c1 + q:c1 + 2 * q] = -950
        if rng.random() < 0.3:
            s[(x - X / 2) ** 2 + (y - Y / 2) ** 2 <= (min(X, Y) / 3) ** 2] = 40
            s[(x - X / 2) ** 2 + (y - Y / 2) ** 2 <= (min(X, Y) / 5) ** 2] = -900
        v[:, :, z] = s
    return v


@pytest.mark.parametrize("seed,shape,min_area", [(1, (96, 110, 25), 300), (2, (64, 70, 12), 100), (3, (120, 100, 40), 500),
                                                 (4, (33, 47, 7), 10), (5, (80, 80, 64), 0)])
def test_random_get_l_against_restatement(seed, shape, min_area):
    rng = np.random.default_rng(seed)
    v = blob_volume(rng, shape, 12)
    for T in (-950.0, -500.0, 40.0, 40.5):
        got = A.get_l(v, T, min_area)
        assert np.array_equal(got, LO.get_l(v, T, min_area)), (seed, T)


def test_random_equal_size_components():
    rng = np.random.default_rng(11)
    X, Y, Z = 90, 96, 20
    v = np.full((X, Y, Z), -1000, np.int16)
    for z in range(Z):                             # a lattice of equal squares with equal holes: every argmax is a tie
        step = int(rng.choice([15, 18, 24]))
        for i in range(0, X - 12, step):
            for j in range(0, Y - 12, step):
                v[i:i + 12, j:j + 12, z] = 40
                v[i + 3:i + 9, j + 3:j + 9, z] = -900
    for min_area in (0, 20, 40):
        assert np.array_equal(A.get_l(v, 0.0, min_area), LO.get_l(v, 0.0, min_area))


def test_random_preprocess_against_restatement():
    for seed in (21, 22):
        rng = np.random.default_rng(seed)
        X, Y, Z = 176, 192, 28
        x, y = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
        ct = np.full((X, Y, Z), -1000, np.int16)
        ct[:, :, :] = np.where(((x - X / 2) / (X / 2 + 3)) ** 2 + ((y - Y / 2) / (Y / 2 + 3)) ** 2 > 1, -2048, -1000)[:, :, None]
        body = ((x - X / 2) / (X * 0.45)) ** 2 + ((y - Y / 2) / (Y * 0.44)) ** 2 <= 1
        ct[body] = 40 + rng.integers(-30, 30, size=(int(body.sum()), Z)).astype(np.int16)
        for side in (-1, 1):
            lung = ((x - X / 2) / (X * 0.25)) ** 2 + ((y - Y / 2 - side * Y * 0.2) / (Y * 0.14)) ** 2 <= 1
            ct[lung] = -1000 + rng.integers(0, 150, size=(int(lung.sum()), Z)).astype(np.int16)
        try:
            want = LO.preprocess_ct(ct)
        except IndexError:
            with pytest.raises(IndexError):
                A.preprocess_ct(ct)
            continue
        got = A.preprocess_ct(ct)
        for g, w in zip(got, want[:3]):
            assert np.array_equal(g, w), seed


def test_large_synthetic_case_on_device():
    X, Y, Z = 512, 512, 400
    dev = torch.device("cuda")
    x = torch.arange(X, device=dev, dtype=torch.float32).view(X, 1)
    y = torch.arange(Y, device=dev, dtype=torch.float32).view(1, Y)
    z = torch.arange(Z, device=dev, dtype=torch.float32).view(1, 1, Z)
    fov = ((x - 256) ** 2 + (y - 256) ** 2 > 250 ** 2).unsqueeze(2)
    body = (((x - 256) / 230) ** 2 + ((y - 256) / 200) ** 2 <= 1).unsqueeze(2)
    f = 0.55 + 0.45 * torch.sin(np.pi * (z + 0.5) / Z)
    ct = torch.full((X, Y, Z), -1000, dtype=torch.int16, device=dev)
    ct[body.expand(X, Y, Z)] = 40
    for side in (-1, 1):
        lung = (((x - 240) / 120).unsqueeze(2) / f) ** 2 + (((y - 256 - side * 100) / 70).unsqueeze(2) / f) ** 2 <= 1
        tex = (-1000 + 2 * ((x + y).to(torch.int64) % 76)).to(torch.int16).unsqueeze(2).expand(X, Y, Z)
        ct[lung] = tex[lung]
    ct[fov.expand(X, Y, Z)] = -2048
    got = A.preprocess_ct(ct)
    want = LO.preprocess_ct(ct.cpu().numpy())
    for g, w in zip(got[:2], want[:2]):
        assert np.array_equal(g.cpu().numpy(), w)
    assert np.array_equal(got[2], want[2])
    again = A.preprocess_ct(ct)                                # two runs bitwise equal
    assert all(torch.equal(a, b) for a, b in zip(got[:2], again[:2])) and np.array_equal(got[2], again[2])


def test_two_runs_equal_and_errors(gold):
    ct = gold["c_ct"]
    a = A.get_l(torch.from_numpy(ct).cuda(), float(gold["c_T"]))
    b = A.get_l(torch.from_numpy(ct).cuda(), float(gold["c_T"]))
    assert torch.equal(a, b)
    with pytest.raises(TypeError):
        A.get_l(torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda"), 0.0)
    with pytest.raises(ValueError):
        A.get_l(torch.zeros((4, 4), dtype=torch.int16, device="cuda"), 0.0)
