"""``surface_distances``, ``order_statistics`` and ``surface_metrics`` on the device against tests/surface_oracle.py (DESIGN.md
section 3m).  Distances, counts and voxel indices are compared bit for bit (float64 through int64 views); maxima, percentiles
and tolerance counts exactly; the three means against ``math.fsum`` under the worst-case bound of any summation order.  The cases
(tests/test_surface_host.py, one oracle run per process) are the smallest at which each mechanism can go wrong: rows with a
tail, a scan that crosses its block, extents of 1, massive ties over many workgroups, many distinct values, a box that is not
aligned to words, the shell of the volume against one voxel, and equal masks."""
import numpy as np
import pytest
import torch

import surface_oracle as so
from test_surface_host import CASES, bits, case

pytestmark = pytest.mark.gpu

TOLERANCES = (0.0, 0.7, 1.0, 1.25, 2.0, 3.5, 10.0, 1e9)


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", list(CASES))
def test_distances_counts_and_voxels_equal_the_oracle(A, name):
    a, b, spacing, D, n_a, n_b, voxels = case(name)
    got, ga, gb, gv = A.surface_distances(dev(a), dev(b), spacing, return_voxels=True)
    assert (ga, gb) == (n_a, n_b)
    assert got.dtype == torch.float64 and gv.dtype == torch.int32 and got.is_cuda and gv.is_cuda
    assert np.array_equal(gv.cpu().numpy(), voxels)
    assert np.array_equal(bits(got.cpu().numpy()), bits(D))
    plain = A.surface_distances(dev(a), dev(b), spacing)
    assert len(plain) == 3 and plain[1:] == (n_a, n_b) and np.array_equal(bits(plain[0].cpu().numpy()), bits(D))


def check_metrics(got, want, D, n_a, n_b):
    assert (got.n_a, got.n_b) == (n_a, n_b)
    for k in ("hd", "hd_percentile", "hd_percentile_pooled"):
        print(k, getattr(got, k), want[k])
        assert bits(getattr(got, k)) == bits(want[k]), k
    print("nsd", got.nsd, want["nsd"])
    assert got.nsd == want["nsd"] and [round(v * (n_a + n_b)) for v in got.nsd] == list(want["nsd_counts"])
    for k, part in (("asd_ab", D[:n_a]), ("asd_ba", D[n_a:]), ("assd", D)):
        bound = so.mean_bound(part)
        print(k, getattr(got, k), want[k], "bound", bound)
        assert abs(getattr(got, k) - want[k]) <= bound, (k, getattr(got, k), want[k], bound)


@pytest.mark.parametrize("name", list(CASES))
def test_metrics_equal_the_oracle(A, name):
    a, b, spacing, D, n_a, n_b, _ = case(name)
    want = so.metrics(D, n_a, n_b, 95.0, TOLERANCES)
    got = A.surface_metrics(dev(a), dev(b), spacing, tolerances=TOLERANCES)
    check_metrics(got, want, D, n_a, n_b)
    again = A.surface_metrics(dev(a), dev(b), spacing, tolerances=TOLERANCES)
    assert again == got and bits(again.assd) == bits(got.assd) and bits(again.asd_ab) == bits(got.asd_ab)     # the same bits
    if name == "same":
        assert got.hd == 0.0 and got.assd == 0.0 and got.nsd == (1.0,) * len(TOLERANCES)


@pytest.mark.parametrize("q", [0, 50, 100, 2.5])
def test_other_percentiles(A, q):
    a, b, spacing, D, n_a, n_b, _ = case("sparse_20x20x70")
    want = so.metrics(D, n_a, n_b, q, (1.0,))
    check_metrics(A.surface_metrics(dev(a), dev(b), spacing, percentile=q), want, D, n_a, n_b)


def test_default_arguments(A):
    a, b, _, _, _, _, _ = case("tail_3x4x130")
    D, n_a, n_b, _ = so.surface_distances(a, b)
    got = A.surface_metrics(dev(a), dev(b))
    check_metrics(got, so.metrics(D, n_a, n_b), D, n_a, n_b)
    assert len(got.nsd) == 1


# ---- order statistics -----------------------------------------------------------------------------------------------------------
def wide_values(n, seed):
    """Non-negative doubles whose exponents span the whole range, with +0.0, a subnormal, 1e300 and runs of duplicates."""
    rng = np.random.default_rng(seed)
    x = rng.random(n) * 10.0 ** rng.integers(-300, 300, n).astype(np.float64)
    special = np.array([0.0, 5e-324, 1e300, 2.2250738585072014e-308, 1.0, 1.0, 1.0])
    where = rng.permutation(n)[:min(n, special.size)]
    x[where] = special[:where.size]
    if n >= 16:
        x[rng.integers(0, n, n // 4)] = x[rng.integers(0, n)]              # a long run of one value
        x[rng.integers(0, n, n // 8)] = 0.0
    assert (x >= 0).all() and np.isfinite(x).all() and not np.signbit(x).any()
    return x


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1025, 70001])
def test_order_statistics_equal_sort(A, n):
    x = wide_values(n, n)
    srt = np.sort(x)
    ranks = sorted({0, n // 2, n - 1})
    got = A.order_statistics(dev(x), ranks)
    assert got.dtype == torch.float64 and got.is_cuda
    assert np.array_equal(bits(got.cpu().numpy()), bits(srt[ranks]))
    # eight requests at once over overlapping and adjoining segments
    cut = [0, n // 3, n // 2, (2 * n) // 3, n]
    segs = [(0, n), (0, n), (cut[0], max(cut[1], 1)), (max(cut[1], 1) - 1, max(cut[2], 1)), (cut[2], n), (n // 4, max((3 * n) // 4, n // 4 + 1)),
            (n - 1, n), (0, n)]
    rk = [0, n - 1, 0, (segs[3][1] - segs[3][0]) // 2, (n - cut[2]) - 1, (segs[5][1] - segs[5][0]) // 2, 0, n // 2]
    want = np.array([np.sort(x[b:e])[r] for (b, e), r in zip(segs, rk)])
    got = A.order_statistics(dev(x), rk, segs)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_order_statistics_rejects_bad_arguments(A):
    x = dev(np.arange(10, dtype=np.float64))
    with pytest.raises(ValueError, match="values"):
        A.order_statistics(x.float(), [0])
    with pytest.raises(ValueError, match="ranks"):
        A.order_statistics(x, list(range(9)))
    with pytest.raises(ValueError, match="ranks"):
        A.order_statistics(x, [10])
    with pytest.raises(ValueError, match="segments"):
        A.order_statistics(x, [0], [(3, 3)])
    with pytest.raises(ValueError, match="segments"):
        A.order_statistics(x, [0, 1], [(0, 10)])


# ---- errors and edge behaviour --------------------------------------------------------------------------------------------------
def test_an_empty_mask(A):
    a = dev(np.ones((3, 4, 5), np.uint8))
    z = torch.zeros_like(a)
    for p, l, n in ((a, z, (54, 0)), (z, a, (0, 54)), (z, z, (0, 0))):              # 54 = 60 voxels less the 1 x 2 x 3 inside
        with pytest.raises(ValueError, match="without voxels"):
            A.surface_metrics(p, l)
        with pytest.raises(ValueError, match="without voxels"):
            A.surface_distances(p, l)
        m = A.surface_metrics(p, l, tolerances=(1.0, 2.0), empty="inf")
        inf = float("inf")
        assert m == A.SurfaceMetrics(inf, inf, inf, inf, inf, inf, (0.0, 0.0), n[0], n[1])


def test_bad_arguments_name_the_argument(A):
    a = dev(np.ones((3, 4, 5), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        A.surface_metrics(a, a[:, :, :4])
    with pytest.raises(ValueError, match="shape"):
        A.surface_distances(a[0], a[0])
    with pytest.raises(ValueError, match="spacing"):
        A.surface_metrics(a, a, spacing=(1.0, float("inf"), 1.0))
    with pytest.raises(ValueError, match="spacing"):
        A.surface_distances(a, a, spacing=-1)
    for q in (-0.5, 100.5, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            A.surface_metrics(a, a, percentile=q)


def test_numpy_in_numpy_out_and_any_dtype(A):
    a, b, spacing, D, n_a, n_b, voxels = case("tail_3x4x130")
    got, ga, gb, gv = A.surface_distances(a.astype(np.float32) * 3.0, b.astype(bool), spacing, return_voxels=True)
    assert isinstance(got, np.ndarray) and isinstance(gv, np.ndarray) and (ga, gb) == (n_a, n_b)
    assert np.array_equal(bits(got), bits(D)) and np.array_equal(gv, voxels)
    check_metrics(A.surface_metrics(a, b.astype(np.int64) * 7, spacing, tolerances=TOLERANCES), so.metrics(D, n_a, n_b, 95.0, TOLERANCES), D,
                  n_a, n_b)
