"""The airway cross-sections on a side stream, behind a producer that is still busy when the operation is called
(tests/side_stream.py), as tests/test_streams_betti_gpu.py runs the Betti numbers: the inputs hold poison (the volumes turned round,
another valid input with other points) until a delayed copy on a fresh non-blocking stream delivers the real data, and the
operation is called under that stream while the delay is pending.  A launch, memset or copy on stream 0, or a host read that waits
for another stream -- the read of the number of points, the copy back -- would see the poison.  Results must equal the same call
made beforehand on the default stream bit for bit, and the oracle."""
import numpy as np
import pytest
import torch

from guarded_alloc import same_bits
from side_stream import run_behind_delay, to_device

import cross_section_cases as cc
import cross_section_oracle as co
from test_cross_section_gpu import same

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
    """Poison for a volume: the same volume turned round along its three axes (other points, other sections)."""
    return np.ascontiguousarray(a[::-1, ::-1, ::-1])


@pytest.mark.parametrize("name", ["noise:", "cylinder:1,0.5"])
def test_cross_sections(A, name):
    parsing, skeleton, kw = cc.case(name)
    if name.startswith("cylinder"):                            # (a cylinder turned round is itself: cut one end off the skeleton)
        skeleton = np.array(skeleton)
        skeleton[:, :7] = 0
    got = both([parsing, skeleton], [turned(parsing), turned(skeleton)], lambda p, s: A.cross_sections(p, s, **kw), "cross sections")
    same(got, co.cross_sections(parsing, skeleton, **kw))


def test_branch_table(A):
    parsing, skeleton, kw = cc.case("noise:")
    table = both([parsing, skeleton], [turned(parsing), turned(skeleton)],
                 lambda p, s: A.branch_morphometry(p, s, cc.ANISO, cross_sections=True), "cross section table")
    want = co.cross_sections(parsing, skeleton, spacing=cc.ANISO)
    rows = co.per_branch(want["label"], co.derived(want["count"], want["moments"], want["rim"], want["step"]), table.num)
    assert np.array_equal(table.section_count, rows["section_count"])
    for k in co.BRANCH_COLUMNS:
        np.testing.assert_allclose(getattr(table, k), rows[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
