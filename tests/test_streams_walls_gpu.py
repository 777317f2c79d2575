"""The airway walls on a side stream, behind a producer that is still busy when the operation is called (tests/side_stream.py), as
tests/test_streams_cross_section_gpu.py runs the cross-sections: the CT and the volumes hold poison (the same arrays turned round)
until a delayed copy on a fresh non-blocking stream delivers the real data, and the operation is called under that stream while the
delay is pending.  A launch or copy on stream 0 -- the upload of the sections' rows, the ray kernel, the copy back -- would see the
poison.  Results must equal the same call made beforehand on the default stream bit for bit, and the oracle.

The file is named so that it runs AFTER tests/test_streams_gpu.py, like the clDice stream tests (tests/test_topology_cldice_streams_gpu.py
says why): that file's first test is a positive control whose outcome depends on how many pool streams the process has used
before it, and with this file's five streams ahead of it the control saw the real data.  Run after it, this file leaves the
process as it was when the control draws its stream."""
import numpy as np
import pytest
import torch

from guarded_alloc import same_bits
from side_stream import run_behind_delay, to_device

import airway_wall_cases as wc
import airway_wall_oracle as wo
from test_airway_wall_gpu import given, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def both(real, poison, op, label):
    """The side-stream result of ``op`` after asserting that it has the bits of the default-stream result (also the warm-up)."""
    real = [np.array(v) for v in real]                         # (writable copies: the shared volumes are read-only)
    want = op(*[to_device(v) for v in real])
    torch.cuda.synchronize()
    got = run_behind_delay(lambda: real, lambda: poison, op, label=label)
    same_bits(got.to_dict(), want.to_dict(), f"{label}: side stream against default stream")
    return got


def turned(a):
    """Poison for a volume: the same volume turned round along its three axes (other points, other profiles)."""
    return np.ascontiguousarray(a[::-1, ::-1, ::-1])


@pytest.mark.parametrize("name", ["noise:", "blob:oblique"])
def test_sections_computed(A, name):
    c = wc.case(name)
    volumes = [c["ct"], c["parsing"], c["skeleton"]]
    got = both(volumes, [turned(v) for v in volumes], lambda ct, p, s: A.airway_walls(ct, p, s, c["spacing"], return_rays=True),
               "airway walls")
    same(got, wc.want(name))


@pytest.mark.parametrize("name", ["noise_f32:", "two_lumina:any"])
def test_sections_given(A, name):
    """The sections' rows are uploaded inside the call: that copy too must follow the stream."""
    c = wc.case(name)
    sections = given(A, wc.sections(name), c["spacing"], c["same_label"])
    volumes = [c["ct"], c["parsing"]]
    got = both(volumes, [turned(v) for v in volumes],
               lambda ct, p: A.airway_walls(ct, p, None, c["spacing"], sections=sections, return_rays=True), "airway walls, sections given")
    same(got, wc.want(name))


def test_branch_table(A):
    c = wc.case("noise:")
    volumes = [c["ct"], c["parsing"], c["skeleton"]]

    def op(ct, p, s):
        return A.branch_morphometry(p, s, c["spacing"], walls=A.airway_walls(ct, p, s, c["spacing"], min_rays=8))

    table = both(volumes, [turned(v) for v in volumes], op, "airway wall table")
    want = wc.want("noise:")
    rows = wo.per_branch(want["label"], wo.derived(want["mask"], want["sums"], 8), table.num)
    assert np.array_equal(table.wall_sections, rows["wall_sections"]) and table.wall_sections.sum() > 0
    for k in wo.BRANCH_COLUMNS:
        np.testing.assert_allclose(getattr(table, k), rows[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
