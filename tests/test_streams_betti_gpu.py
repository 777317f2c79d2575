"""Labelling, the size filter, the Euler number and the Betti numbers / errors on a side stream, behind a producer that is still busy
when the operation is called (tests/side_stream.py), as tests/test_streams_surface_gpu.py runs the surface distances: the inputs
hold poison (another valid input) until a delayed copy on a fresh non-blocking stream delivers the real data, and the operation is
called under that stream while the delay is pending.  A launch, memset or copy on stream 0, or a host read that waits for another
stream, would see the poison.  Results must equal the same call made beforehand on the default stream bit for bit, and the oracle."""
import numpy as np
import pytest
import torch

from guarded_alloc import same_bits
from side_stream import run_behind_delay, to_device

import betti_oracle as bo
from test_betti_host import volume

pytestmark = pytest.mark.gpu

NAME = "noise30"


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def both(real, poison, op, label, no_host_sync=False):
    """The side-stream result of ``op`` after asserting that it has the bits of the default-stream result (also the warm-up)."""
    real = [np.array(v) for v in real]                         # (writable copies: the shared volumes are read-only)
    want = op(*[to_device(v) for v in real])
    torch.cuda.synchronize()
    got = run_behind_delay(lambda: real, lambda: poison, op, no_host_sync=no_host_sync, label=label)
    same_bits(got, want, f"{label}: side stream against default stream")
    return got


def turned(a):
    """Poison for a volume: the same volume turned round along its three axes (other components, other numbers)."""
    return np.ascontiguousarray(a[::-1, ::-1, ::-1])


def test_label_does_not_wait(A):
    v = volume(NAME)
    lab, num = both([v], [turned(v)], lambda m: A.label(m, 1, return_num=True), "label", no_host_sync=True)
    want, n = bo.label(v, 1)
    assert int(num) == n and np.array_equal(lab.cpu().numpy(), want)


def test_label_with_table(A):
    v = volume(NAME)
    lab, num, tab = both([v], [turned(v)], lambda m: A.label(m, 3, return_num=True, return_table=True), "label table")
    want, n = bo.label(v, 3)
    assert num == n and np.array_equal(lab.cpu().numpy(), want)
    for g, w in zip((tab.size, tab.first, tab.box), bo.table(want, n)):
        assert np.array_equal(g.cpu().numpy(), w)


def test_remove_small_objects_does_not_wait(A):
    v = volume(NAME)
    got = both([v], [turned(v)], lambda m: A.remove_small_objects(m, 3, 1), "remove small objects", no_host_sync=True)
    assert np.array_equal(got.cpu().numpy(), bo.remove_small_objects(v, 3, 1))


@pytest.mark.parametrize("connectivity", [3, 1])
def test_euler_and_betti_numbers(A, connectivity):
    v = volume(NAME)
    got = both([v], [turned(v)], lambda m: (A.euler_number(m, connectivity), A.betti_numbers(m, connectivity)), "betti numbers")
    assert got == (bo.euler_number(v, connectivity), bo.betti_numbers(v, connectivity))


def test_betti_error(A):
    a, b = bo.tile_volume("sparse"), bo.tile_volume("dense")
    patch = (16, 16, 24)
    got = both([a, b], [turned(b), turned(a)], lambda p, q: A.betti_error(p, q, patch, 3, whole=True), "betti error")
    tiles, tp, tl, err, total = bo.betti_error(a, b, patch, 3)
    assert got.tiles == tiles and np.array_equal(got.pred.cpu().numpy(), tp) and np.array_equal(got.label.cpu().numpy(), tl)
    assert np.array_equal(got.error, err) and got.total_error == total
