"""The surface distances, the order statistics and the boundary metrics over dirty scratch memory, with red zones around every
buffer (tests/guarded_alloc.py), as tests/test_scratch_and_bounds_edt_sampling_gpu.py runs the EDT: three runs -- the outputs and
the workspaces pre-filled with 0x00, 0xFF and seeded random bytes, the inputs copied into red-zoned buffers -- must leave every
red zone as it was, give the same bits, and equal the oracle (tests/surface_oracle.py), never another run of the code under test.
The cases have rows with a tail, a box that is not aligned to words and one that is the whole volume.

Limit (the one tests/guarded_alloc.py documents, shared with the other mask operations of ``postprocess``): the wrappers
normalise a mask with ``(a != 0).to(torch.uint8).contiguous()``, a copy made inside torch, so the kernels read that copy and
an over-read beside a mask would not reach the red zones of the guarded input.  The workspaces, the record and every output are
guarded, and ``order_statistics`` reads its guarded input directly."""
import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import surface_oracle as so
from test_surface_host import bits, case
from test_surface_gpu import TOLERANCES, check_metrics, wide_values

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
NAMES = ("tail_3x4x130", "boxed_24x40x200", "whole_against_one")


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return guard(torch.from_numpy(np.ascontiguousarray(a)).cuda())


@pytest.mark.parametrize("name", NAMES)
def test_surface_distances(A, name):
    a, b, spacing, D, n_a, n_b, voxels = case(name)
    got, ga, gb, gv = three_fills(lambda: A.surface_distances(dev(a), dev(b), spacing, return_voxels=True), "surface distances")
    assert (ga, gb) == (n_a, n_b) and np.array_equal(gv.cpu().numpy(), voxels) and np.array_equal(bits(got.cpu().numpy()), bits(D))


@pytest.mark.parametrize("name", NAMES)
def test_surface_metrics(A, name):
    a, b, spacing, D, n_a, n_b, _ = case(name)
    got = three_fills(lambda: A.surface_metrics(dev(a), dev(b), spacing, tolerances=TOLERANCES), "surface metrics")
    check_metrics(got, so.metrics(D, n_a, n_b, 95.0, TOLERANCES), D, n_a, n_b)


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_order_statistics(A, n):
    x = wide_values(n, 7 * n)
    ranks = [0, n // 2, n - 1, n // 3]
    segs = [(0, n), (0, n), (0, n), (n // 3, n)]
    got = three_fills(lambda: A.order_statistics(dev(x), ranks, segs), "order statistics")
    want = np.array([np.sort(x[b:e])[r] for (b, e), r in zip(segs, ranks)])
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
