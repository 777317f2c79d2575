"""CT preprocessing: the host arithmetic of seunet_amd.preprocess against numpy and the reference's
recorded values (tests/golden/lung_known.npz, scripts/make_golden_lung.py); the restatement in tests/lung_oracle.py against
the same fixture; argument handling that needs no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lung_oracle as LO  # noqa: E402
from seunet_amd import preprocess as P  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lung_known.npz")
PREPRO = ("a", "b", "c")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def counts_of(a):
    return np.bincount(a.ravel().view(np.uint16).astype(np.int64), minlength=65536)


def same_hist(h1, h2):
    assert h1[0].dtype == h2[0].dtype and h1[1].dtype == h2[1].dtype
    assert np.array_equal(h1[0], h2[0])
    assert np.array_equal(h1[1].view(np.uint64), h2[1].view(np.uint64))         # edge bits


def test_histogram_from_counts_equals_numpy_histogram():
    rng = np.random.default_rng(7)
    arrays = []
    for k in range(120):
        lo = int(rng.integers(-32768, 32767))
        hi = int(min(32767, lo + int(rng.choice([1, 2, 3, 299, 300, 301, 1000, 65535]))))
        arrays.append(rng.integers(lo, hi + 1, size=int(rng.integers(1, 3000)), dtype=np.int64).astype(np.int16))
    arrays += [np.full(17, -5, np.int16), np.array([32767], np.int16), np.array([-32768, 32767], np.int16),
               (np.arange(-40000, 40000, 7) + 0).astype(np.int16),                          # wrapped values
               (rng.integers(-3000, 3000, 5000).astype(np.int16) + np.int16(1024)).astype(np.int16),
               np.array([3, 4], np.int16), np.array([-800, -800, -799], np.int16)]
    for a in arrays:
        for bins in (300, 50):
            same_hist(P.histogram_from_counts(counts_of(a), bins), np.histogram(a.ravel(), bins))


@pytest.mark.parametrize("key", PREPRO)
def test_host_arithmetic_reproduces_the_reference(gold, key):
    h1 = (gold[f"{key}_hist1_y"], gold[f"{key}_hist1_x"])
    ct = gold[f"{key}_ct"]
    shifted = (ct + np.int16(1024)).astype(np.int16)
    counts = counts_of(shifted)
    same_hist(P.histogram_from_counts(counts), h1)
    aaa = float(gold[f"{key}_aaa"])
    if np.isnan(aaa):
        assert shifted.min() > P.PAD_TH
        c2 = counts
    else:
        got = P.padding_value(h1)
        assert got == aaa and type(got) is np.float64
        c2 = P.clamped_counts(counts, aaa)
        clamped = shifted.copy()
        clamped[clamped <= -800] = aaa
        assert np.array_equal(c2, counts_of(clamped))
    h2 = P.histogram_from_counts(c2)
    same_hist(h2, (gold[f"{key}_hist2_y"], gold[f"{key}_hist2_x"]))
    T = P.threshold_from_hist(h2)
    assert T == float(gold[f"{key}_T"])
    m = gold[f"{key}_Mask"].astype(bool)
    xx, yy, zz = np.where(m)
    box = P.crop_box([xx.min(), yy.min(), zz.min()], [xx.max(), yy.max(), zz.max()], m.shape)
    assert box.dtype == gold[f"{key}_box"].dtype and np.array_equal(box, gold[f"{key}_box"])


@pytest.mark.parametrize("key", PREPRO)
def test_restatement_matches_the_reference(gold, key):
    data_cut, lung_mask, box, inter = LO.preprocess_ct(gold[f"{key}_ct"])
    assert inter["T"] == float(gold[f"{key}_T"])
    for k in ("L", "L1", "L2", "Mask"):
        assert np.array_equal(np.asarray(inter[k]).astype(np.uint8), gold[f"{key}_{k}"].astype(np.uint8)), k
    assert np.array_equal(box, gold[f"{key}_box"])
    assert data_cut.dtype == np.int16 and np.array_equal(data_cut, gold[f"{key}_data_cut"])
    assert np.array_equal(lung_mask, gold[f"{key}_lung_mask"])


def test_restatement_prediction_mode_and_failures(gold):
    cp, _, _, _ = LO.preprocess_ct(gold["d_ct"], "prediction")
    assert np.array_equal(cp, gold["d_data_cut"])
    ct = gold["f_ct"]
    cp = (ct + np.int16(1024)).astype(np.int16)
    T = LO.th_2t(cp)
    assert T == float(gold["f_T"])
    L = LO.get_l(cp, T)
    assert np.array_equal(L, gold["f_L"]) and not L.any()
    with pytest.raises(IndexError):
        LO.preprocess_ct(ct)
    for key in ("e", "e2"):
        assert np.array_equal(LO.large_connected_domain26(gold[f"{key}_label"]), gold[f"{key}_ldc"])
        assert np.array_equal(LO.cut_mask(gold[f"{key}_label"], gold[f"{key}_box"]), gold[f"{key}_mask_cut"])
    with pytest.raises(IndexError):
        LO.large_connected_domain26(gold["e3_label"])


def test_fixture_is_small():
    assert os.path.getsize(GOLD) < (1 << 20)


def test_argument_checks_without_a_gpu():
    with pytest.raises(TypeError):
        P.preprocess_ct(np.zeros((4, 4, 4), np.float32))
    with pytest.raises(TypeError):
        P.th_2t(np.zeros((4, 4, 4), np.int32))
    with pytest.raises(RuntimeError):
        P.get_l(torch.zeros((4, 4, 4), dtype=torch.int16), 0.0)          # a CPU tensor: no CPU path
    with pytest.raises(ValueError):
        P.preprocess_ct(np.zeros((4, 4, 4), np.int16), mode="train")
    with pytest.raises(ValueError):
        P.histogram_from_counts(np.zeros(65536, np.int64))
