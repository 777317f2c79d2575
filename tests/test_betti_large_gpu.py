"""Labelling and the topological numbers at (1025, 1024, 2), density 0.3: more than 2^16 components at connectivity 1 (no cap on the
label count) and more than 2^20 packed words, where the scan's top level loops over chunks of 1024 block totals.  Against
tests/betti_oracle.py; scipy takes a tenth of a second per call."""
import numpy as np
import pytest
import torch

import betti_oracle as bo
from test_betti_host import volume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


@pytest.mark.parametrize("connectivity", [1, 3])
def test_label_and_table(A, connectivity):
    v = volume("large")
    want, num = bo.label(v, connectivity)
    assert (num > 65535) == (connectivity == 1)
    lab, n, tab = A.label(v, connectivity, return_num=True, return_table=True)
    assert n == num and np.array_equal(lab, want)
    size, first, box = bo.table(want, num)
    assert np.array_equal(tab.size, size) and np.array_equal(tab.first, first) and np.array_equal(tab.box, box)
    assert np.array_equal(A.remove_small_objects(v, 3, connectivity), bo.remove_small_objects(v, 3, connectivity))


@pytest.mark.parametrize("connectivity", [3, 1])
def test_euler_and_betti_numbers(A, connectivity):
    v = volume("large")
    assert A.euler_number(v, connectivity) == bo.euler_number(v, connectivity)
    assert A.betti_numbers(v, connectivity) == bo.betti_numbers(v, connectivity)


@pytest.mark.parametrize("connectivity", [3, 1])
def test_betti_numbers_over_tiles(A, connectivity):
    """More voxels than one visit of the grid-stride passes covers: their threads and waves meet several tiles in turn.  One mask as
    both arguments, so that the oracle's loop over the 121 crops runs once."""
    v = volume("large")
    patch = (100, 100, 2)
    want, tiles = bo.betti_tiles(v, patch, connectivity)
    got = A.betti_error(v, v, patch, connectivity)
    assert got.tiles == tiles == (11, 11, 1)
    assert np.array_equal(got.pred.cpu().numpy(), want) and np.array_equal(got.label.cpu().numpy(), want)
    assert got.error.tolist() == [0.0, 0.0, 0.0] and got.total_error == 0.0
