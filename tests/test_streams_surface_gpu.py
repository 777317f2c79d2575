"""The surface distances, the order statistics and the boundary metrics on a side stream, behind a producer that is still busy
when the operation is called (tests/side_stream.py), as tests/test_streams_edt_sampling_gpu.py runs the EDT: the inputs hold poison
(another valid input) until a delayed copy on a fresh non-blocking stream delivers the real data, and the operation is called under
that stream while the delay is pending.  A launch, memset or copy on stream 0, or a host read that waits for another stream, would
see the poison.  Results must equal the same call made beforehand on the default stream bit for bit, and the oracle."""
import numpy as np
import pytest
import torch

from guarded_alloc import same_bits
from side_stream import run_behind_delay, to_device

import surface_oracle as so
from test_surface_host import bits, case
from test_surface_gpu import TOLERANCES, check_metrics, wide_values

pytestmark = pytest.mark.gpu

NAME = "boxed_24x40x200"


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def both(real, poison, op, label, no_host_sync=False):
    """The side-stream result of ``op`` after asserting that it has the bits of the default-stream result (also the warm-up)."""
    want = op(*[to_device(v) for v in real])
    torch.cuda.synchronize()
    got = run_behind_delay(lambda: real, lambda: poison, op, no_host_sync=no_host_sync, label=label)
    same_bits(got, want, f"{label}: side stream against default stream")
    return got


def turned(a):
    """Poison for a volume: the same volume turned round along its three axes (another box, other counts)."""
    return np.ascontiguousarray(a[::-1, ::-1, ::-1])


def test_surface_distances(A):
    a, b, spacing, D, n_a, n_b, voxels = case(NAME)
    got, ga, gb, gv = both([a, b], [turned(b), turned(a)], lambda p, q: A.surface_distances(p, q, spacing, return_voxels=True),
                           "surface distances")
    assert (ga, gb) == (n_a, n_b) and np.array_equal(gv.cpu().numpy(), voxels) and np.array_equal(bits(got.cpu().numpy()), bits(D))


def test_surface_metrics(A):
    a, b, spacing, D, n_a, n_b, _ = case(NAME)
    got = both([a, b], [turned(b), turned(a)], lambda p, q: A.surface_metrics(p, q, spacing, tolerances=TOLERANCES), "surface metrics")
    check_metrics(got, so.metrics(D, n_a, n_b, 95.0, TOLERANCES), D, n_a, n_b)


def test_order_statistics_does_not_wait(A):
    n = 5000
    x = wide_values(n, 11)
    ranks, segs = [0, n // 2, n - 1, 100], [(0, n), (0, n), (0, n), (1000, 3000)]
    got = both([x], [np.ascontiguousarray(x[::-1] + 1.0)], lambda v: A.order_statistics(v, ranks, segs), "order statistics",
               no_host_sync=True)
    want = np.array([np.sort(x[b:e])[r] for (b, e), r in zip(segs, ranks)])
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
