"""The wrappers behind ``airway_parse`` (binary morphology, hole fill, slice moments, label scatter, the whole call) over dirty
scratch memory, with red zones around every buffer (tests/guarded_alloc.py), exactly as tests/test_scratch_and_bounds_volume_gpu.py
runs the other volume operations: three runs -- scratch and outputs pre-filled with 0x00, 0xFF and seeded random bytes, inputs
copied into red-zoned buffers -- must leave every red zone as it was, give the same bits, and equal scipy / the recorded
fixture, never another run of the code under test.  Shapes cross a 64-voxel word, a 4-word block and extent-1 axes."""
import os

import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import skeleton_oracle as so

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z = np.load(os.path.join(GOLDEN, "topology_known.npz"))
_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return guard(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 70), (4, 5, 65), (3, 5, 257), (7, 9, 129)])
def test_morphology(A, shape):
    from scipy import ndimage
    v = (np.random.default_rng(sum(shape)).random(shape) < 0.5).astype(np.uint8)

    def op():
        t = dev(v)
        return A.binary_dilation(t), A.binary_erosion(t), A.binary_erosion(t, border_value=1), A.binary_closing(t)
    dil, er0, er1, clo = three_fills(op, "morphology")
    assert np.array_equal(host(dil), ndimage.binary_dilation(v).astype(np.uint8))
    assert np.array_equal(host(er0), ndimage.binary_erosion(v).astype(np.uint8))
    assert np.array_equal(host(er1), ndimage.binary_erosion(v, border_value=1).astype(np.uint8))
    assert np.array_equal(host(clo), ndimage.binary_erosion(ndimage.binary_dilation(v), border_value=1).astype(np.uint8))


@pytest.mark.parametrize("name", ["shell", "noise", "empty", "line"])
def test_fill_holes(A, name):
    from scipy import ndimage
    v = so.make_case(name)
    got = three_fills(lambda: A.binary_fill_holes(dev(v)), "fill_holes")
    assert np.array_equal(host(got), ndimage.binary_fill_holes(v).astype(np.uint8))


def test_slice_moments_and_scatter_labels(A):
    shape = (5, 7, 66)
    v = (np.random.default_rng(9).random(shape) < 0.5).astype(np.uint8)
    n = v.size
    lin = np.random.default_rng(10).permutation(n)[:200].astype(np.int64)
    val = np.arange(1, 201, dtype=np.int32)

    def op():
        t = dev(v)
        return [A.prep.slice_moments(t, k) for k in (0, 64, 65)], A.prep.scatter_labels(lin, val, shape)
    moments, (cd, parse) = three_fills(op, "parse lists")
    for k, m in zip((0, 64, 65), moments):
        i0, i1 = np.nonzero(v[:, :, k])
        assert m == (len(i0), int(i0.sum()), int(i1.sum()))
    want = np.zeros(n, np.int32)
    want[lin] = val
    assert np.array_equal(host(cd).ravel(), want) and np.array_equal(host(parse).ravel(), (want != 0).astype(np.uint8))


@pytest.mark.parametrize("ci", (2, 3))
def test_airway_parse(A, ci):
    label = (Z[f"case{ci}_label"] != 0).astype(np.uint8)
    got = three_fills(lambda: A.airway_parse(dev(label)), "airway_parse")
    assert np.array_equal(host(got), Z[f"case{ci}_parsing"].astype(np.int32))


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
