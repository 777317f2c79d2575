"""Labelling, the component table, the size filter, the Euler number and the Betti numbers / errors over dirty scratch memory, with
red zones around every buffer (tests/guarded_alloc.py), as tests/test_scratch_and_bounds_surface_gpu.py runs the surface distances:
three runs -- the outputs and the workspaces pre-filled with 0x00, 0xFF and seeded random bytes, the inputs copied into red-zoned
buffers -- must leave every red zone as it was, give the same bits, and equal the oracle (tests/betti_oracle.py), never another run
of the code under test.  The cases have rows with a tail, a degenerate axis, tiles that end inside a word and ragged last tiles.

Limit (the one tests/guarded_alloc.py documents, shared with the other mask operations): the wrappers normalise a mask with
``(a != 0).to(torch.uint8).contiguous()``, a copy made inside torch, so an over-read beside a mask would not reach the red zones of
the guarded input.  The workspaces, the tables and every output are guarded."""
import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import betti_oracle as bo
from test_betti_host import volume

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
NAMES = ("tail_3x4x130", "flat2_40x30x1", "noise30")


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return guard(torch.from_numpy(np.array(a)).cuda())          # (a writable copy: the shared volumes are read-only)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_label_and_table(A, name, connectivity):
    v = volume(name)
    lab, num, tab = three_fills(lambda: A.label(dev(v), connectivity, return_num=True, return_table=True), "label")
    want, n = bo.label(v, connectivity)
    assert num == n and np.array_equal(lab.cpu().numpy(), want)
    for g, w in zip((tab.size, tab.first, tab.box), bo.table(want, n)):
        assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("name", NAMES)
def test_remove_small_objects(A, name):
    v = volume(name)
    got = three_fills(lambda: A.remove_small_objects(dev(v), 2, 1), "remove small objects")
    assert np.array_equal(got.cpu().numpy(), bo.remove_small_objects(v, 2, 1))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("connectivity", [3, 1])
def test_euler_and_betti_numbers(A, name, connectivity):
    v = volume(name)
    got = three_fills(lambda: (A.euler_number(dev(v), connectivity), A.betti_numbers(dev(v), connectivity)), "betti numbers")
    assert got == (bo.euler_number(v, connectivity), bo.betti_numbers(v, connectivity))


@pytest.mark.parametrize("patch", [(16, 16, 24), (7, 5, 13)])
def test_betti_error(A, patch):
    a, b = bo.tile_volume("sparse"), bo.tile_volume("dense")
    got = three_fills(lambda: A.betti_error(dev(a), dev(b), patch, 3, whole=True), "betti error")
    tiles, tp, tl, err, total = bo.betti_error(a, b, patch, 3)
    assert got.tiles == tiles and np.array_equal(got.pred.cpu().numpy(), tp) and np.array_equal(got.label.cpu().numpy(), tl)
    assert np.array_equal(got.error, err) and got.total_error == total
    assert got.whole == (bo.betti_numbers(a, 3), bo.betti_numbers(b, 3))


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
