"""The re-check schedule of csrc/skeleton.hip on the volumes of tests/skeleton_cases.py, bitwise against
skeleton_oracle.skeletonize_memo, pass counts included: the grid-stride loop of skel_round_kernel (more than 8192 candidate
words), skel_finish_kernel with thousands of open words, multi-word rows and hundreds of rounds, and the carry of recheck_word
from one word of a row into the next.  What each case reaches, and which wrong re-check it tells from the right one, is asserted
on the CPU in tests/test_skeleton_host.py; a failure here prints what the oracle did with the first differing voxels, in which
(pass, direction) and in which round of skeleton_oracle.round_model.

All volumes are valid inputs far inside the limits of section 3d.  Wall time of one skeletonize_3d call with a synchronise
on one MI355X, after a warm-up on a small volume (information only, nothing asserts a time):
    many_words_short_chains (200, 200, 3)   2.3 ms      plate_noise (2, 80, 130)   6.4 ms
    slab_noise (110, 110, 3)                258 ms      tree2 (40, 48, 268)       30.6 ms
    sheet_noise (70, 70, 2)                19.8 ms      flat_axis0 (1, 90, 70)     2.4 ms
    plate (2, 80, 130)                     28.0 ms      flat_axis1 (90, 1, 70)     2.7 ms
"""
import numpy as np
import pytest
import torch

import skeleton_cases as sc
from guarded_alloc import guard, three_fills

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                              # a copy: the shared case arrays are read-only


def check(case, got, got_passes):
    g = got.cpu().numpy()
    assert g.dtype == np.uint8 and np.array_equal(g, case.skeleton), sc.describe_difference(case, g)
    assert got_passes == case.passes, f"{case.name}: {got_passes} passes, the oracle runs {case.passes}"


@pytest.mark.parametrize("name", sc.CASES)
def test_equals_the_oracle_bitwise(A, name):
    case = sc.solved(name)
    t = dev(case.volume)
    before = t.clone()
    got, got_passes = A.skeletonize_3d(t, return_passes=True)
    assert got.dtype == torch.uint8 and got.device == t.device and tuple(got.shape) == case.volume.shape
    assert torch.equal(t, before)                                            # the input is not modified
    check(case, got, got_passes)
    again, again_passes = A.skeletonize_3d(t, return_passes=True)            # a second call gives identical bits
    assert torch.equal(again, got) and again_passes == got_passes
    fixed, fixed_passes = A.skeletonize_3d(got, return_passes=True)          # a skeleton is its own skeleton, in one pass
    assert torch.equal(fixed, got), f"{name}: {int((fixed != got).sum())} voxels of the skeleton were thinned again"
    assert fixed_passes == 1


@pytest.mark.parametrize("name", sc.GUARDED)
def test_over_dirty_scratch_with_red_zones(A, name):
    """The word list and its tail, open_list and both undecided masks over 0x00, 0xFF and random scratch, every buffer between
    red zones: a read past the compacted list or of a word no launch wrote changes the bits, a write past a buffer a zone."""
    case = sc.solved(name)
    got, got_passes = three_fills(lambda: A.skeletonize_3d(guard(dev(case.volume)), return_passes=True), "skeleton rounds")
    check(case, got, got_passes)
