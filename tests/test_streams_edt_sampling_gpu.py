"""The EDT with voxel spacing and the per-branch wall distance on a side stream, behind a producer that is still busy when the
operation is called (tests/side_stream.py), as tests/test_streams_gpu.py runs the other families: the inputs hold poison (another
valid input) until a delayed copy on a fresh non-blocking stream delivers the real data, and the operation is called under that
stream while the delay is pending.  A launch, memset or copy on stream 0, or a status read that waits for another stream, would
see the poison.  Results must equal the same call made beforehand on the default stream bit for bit, and the oracles."""
import numpy as np
import pytest
import torch

from guarded_alloc import same_bits
from side_stream import run_behind_delay, to_device

import edt_sampling_oracle as eo
import wall_distance_oracle as wo

pytestmark = pytest.mark.gpu

SPACING = (0.7, 0.8, 1.25)
NUM = 5


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def both(real, poison, op, label):
    """The side-stream result of ``op`` after asserting that it has the bits of the default-stream result (also the warm-up)."""
    want = op(*[to_device(v) for v in real])
    torch.cuda.synchronize()
    got = run_behind_delay(lambda: real, lambda: poison, op, label=label)
    same_bits(got, want, f"{label}: side stream against default stream")
    return got


def inputs():
    from test_scratch_and_bounds_edt_sampling_gpu import want
    parsing, skeleton, mask, dist, indices, tables = want((2, 3, 67))
    return parsing, skeleton, mask, dist, indices, tables


def turned(a):
    """Poison for a volume: the same volume turned round along its last three axes (still a valid input of that shape)."""
    return np.ascontiguousarray(a[..., ::-1, ::-1, ::-1])


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_distance_transform_with_sampling(A):
    _, _, mask, dist, indices, _ = inputs()
    got_dist, got_ind = both([mask], [turned(mask)], lambda t: A.distance_transform_edt(t, return_indices=True, sampling=SPACING),
                             "EDT with sampling")
    assert np.array_equal(got_ind.cpu().numpy(), indices) and np.array_equal(bits(got_dist.cpu().numpy()), bits(dist))


def test_no_zero_voxel_is_seen_on_the_side_stream(A):
    """The status word is read on the caller's stream: the poison has a zero voxel, the real volume has none."""
    real, poison = np.ones((2, 3, 67), np.uint8), np.zeros((2, 3, 67), np.uint8)
    with pytest.raises(ValueError):
        run_behind_delay(lambda: [real], lambda: [poison], lambda t: A.distance_transform_edt(t, sampling=SPACING), label="EDT status")


def test_branch_wall_distance(A):
    parsing, skeleton, _, _, indices, tables = inputs()
    real = [parsing, skeleton, indices]
    got = both(real, [turned(a) for a in real], lambda p, s, i: A.branch_wall_distance(p, s, SPACING, NUM, indices=i), "wall distance")
    wo.same_tables(got, tables)
    inside = both(real[:2], [turned(a) for a in real[:2]], lambda p, s: A.branch_wall_distance(p, s, SPACING, NUM), "wall distance, EDT inside")
    wo.same_tables(inside, tables)


def test_branch_morphometry_physical(A):
    parsing, skeleton, _, _, _, tables = inputs()
    real = [parsing, skeleton]
    got = both(real, [turned(a) for a in real], lambda p, s: A.branch_morphometry(p, s, SPACING, NUM, inscribed="physical"),
               "morphometry physical")
    wo.same_tables({k: getattr(got, k) for k in wo.TABLES}, tables)
    for k, v in wo.radii(tables, SPACING).items():
        assert np.array_equal(bits(getattr(got, k)), bits(v)), k
