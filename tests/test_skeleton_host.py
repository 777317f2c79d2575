"""The thinning definition of DESIGN.md section 3d on the CPU: tests/skeleton_oracle.py reproduces the pinned voxel counts and
digests of the eight test volumes, keeps the topology, and is idempotent; the workspace query of the C ABI answers without a
GPU.  The oracle is the yardstick tests/test_skeleton_gpu.py compares the HIP kernels with.

Its memoised form skeletonize_memo equals it bit for bit, pass counts included; round_model counts the re-check rounds the way
csrc/skeleton.hip schedules them; and every volume of tests/skeleton_cases.py meets the conditions it was built for, among them
that it tells the wrong re-check models listed for it from the definition (tests/test_skeleton_rounds_gpu.py runs the kernels
on those volumes)."""
import numpy as np
import pytest

import skeleton_cases as sc
import skeleton_oracle as so


@pytest.mark.parametrize("name", so.CASES)
def test_oracle_reproduces_counts_and_digests(name):
    v, sk, passes = so.solved(name)
    n_in, n_out, dig, _ = so.EXPECTED[name]
    assert int(v.sum()) == n_in
    assert sk.dtype == np.uint8 and sk.shape == v.shape and set(np.unique(sk)) <= {0, 1}
    assert int(sk.sum()) == n_out
    assert so.digest(sk) == dig
    assert passes >= 1


@pytest.mark.parametrize("name", so.CASES)
def test_skeleton_is_a_subset_with_the_input_topology(name):
    v, sk, _ = so.solved(name)
    assert not np.any(sk.astype(bool) & ~v.astype(bool))
    triple = so.EXPECTED[name][3]
    assert so.topology(v) == triple
    assert so.topology(sk) == triple


@pytest.mark.parametrize("name", so.CASES)
def test_oracle_is_idempotent(name):
    _, sk, _ = so.solved(name)
    again, passes = so.skeletonize(sk)
    assert np.array_equal(again, sk)
    assert passes == 1


def test_the_recheck_and_its_order_matter():
    """The cases are only worth pinning if they tell the raster-order re-check from no re-check and from the reverse order."""
    for name in ("ring", "two"):
        v, sk, _ = so.solved(name)
        assert not np.array_equal(so.skeletonize(v, recheck="none")[0], sk), name
        assert not np.array_equal(so.skeletonize(v, recheck="reverse")[0], sk), name
    v, _, _ = so.solved("two")
    assert so.topology(so.skeletonize(v, recheck="none")[0])[0] != 2       # a component is lost without the re-check


# ---- the memoised statement of the definition, the round model and the cases built on them ---------------------------------
def _random_volume(seed):
    rng = np.random.default_rng(seed)
    shape = (int(rng.integers(1, 10)), int(rng.integers(1, 11)), int(rng.integers(1, 71)) if seed % 3 else int(rng.integers(64, 71)))
    return (rng.random(shape) < rng.uniform(0.5, 0.97)).astype(np.uint8)


@pytest.mark.parametrize("name", so.CASES)
def test_memo_equals_the_slow_oracle_on_the_pinned_cases(name):
    v, sk, passes = so.solved(name)
    got, got_passes = so.skeletonize_memo(v)
    assert got.dtype == sk.dtype and np.array_equal(got, sk) and got_passes == passes


@pytest.mark.parametrize("seed", range(24))
def test_memo_equals_the_slow_oracle_on_random_volumes(seed):
    v = _random_volume(seed)
    want, passes = so.skeletonize(v)
    got, got_passes = so.skeletonize_memo(v)
    assert np.array_equal(got, want) and got_passes == passes, v.shape


@pytest.mark.parametrize("name", ["plate", "sheet_noise"])
def test_memo_equals_the_slow_oracle_on_the_large_cases(name):
    case = sc.solved(name)
    want, passes = so.skeletonize(case.volume)
    assert np.array_equal(case.skeleton, want) and case.passes == passes


def test_memo_runs_the_wrong_rechecks_like_the_slow_oracle():
    for name in ("ring", "two"):
        v, _, _ = so.solved(name)
        for recheck in ("none", "reverse"):
            slow, fast = so.skeletonize(v, recheck=recheck), so.skeletonize_memo(v, recheck=recheck)
            assert np.array_equal(slow[0], fast[0]) and slow[1] == fast[1], (name, recheck)


def test_round_model_by_hand():
    """Rounds that can be counted by hand.  A solid (1, 3, 130) bar, direction 4 first: the candidates are the whole row j = 0
    (an edge or corner voxel of a 3 x 130 rectangle is simple, and none is an end point).  Nothing lies before that row, so word 0 is walked in round 1; the first voxel of word 1 waits for
    the last voxel of word 0 (round 2), and so does the first voxel of word 2 (round 3).  One row, three words."""
    subs = so.round_model(np.ones((1, 3, 130), dtype=np.uint8))
    first = subs[0]
    assert (first.pass_, first.direction, first.candidates, first.words, first.rounds, first.open_words) == (1, 4, 130, 3, 3, 0)
    # the (2, 72, 40) slab of test_long_chains_across_rows: one word per row, every row waits for the row before it
    assert max(s.rounds for s in so.round_model(np.ones((2, 72, 40), dtype=np.uint8))) == 72


def test_what_the_earlier_volumes_reach():
    """Why tests/skeleton_cases.py exists: no pinned volume and neither of the two extra volumes of test_skeleton_gpu.py has
    more candidate words than one grid of skel_round_kernel.  Apart from the slab, skel_finish_kernel only ever gets the two
    words that `tree` leaves for two rounds; the slab gives it 78 one-word rows for 40 rounds: never more words than one stride
    of its loops times five, never a row of several words."""
    dense = (np.random.default_rng(7).random((5, 6, 128)) < 0.7).astype(np.uint8)
    for v in [so.solved(name)[0] for name in so.CASES] + [dense]:
        subs = so.round_model(v)
        assert max(s.words for s in subs) <= 150
        assert max(s.rounds for s in subs) <= so.ROUND_LAUNCHES + 2 and max(s.open_words for s in subs) <= 2, v.shape
    subs = so.round_model(np.ones((2, 72, 40), dtype=np.uint8))
    assert (max(s.words for s in subs), max(s.rounds for s in subs), max(s.open_words for s in subs)) == (140, 72, 78)


def test_the_dense_two_word_volume_does_not_see_the_carry():
    """Recorded so that nobody relies on it: test_skeleton_gpu.py::test_word_aligned_rows_and_carries would pass with the carry
    from word 0 into word 1 dropped.  `plate` and `plate_noise` are the cases that pin the carry (test_case_conditions)."""
    v = (np.random.default_rng(7).random((5, 6, 128)) < 0.7).astype(np.uint8)
    right, wrong = so.skeletonize_memo(v), so.skeletonize_memo(v, recheck="no_carry")
    assert np.array_equal(right[0], wrong[0]) and right[1] == wrong[1]


@pytest.mark.parametrize("name", sc.CASES)
def test_case_conditions(name):
    """Every case still reaches what it was built to reach, and tells the wrong re-checks listed for it from the right one:
    replacing the oracle in tests/test_skeleton_rounds_gpu.py by one of those would make that case fail."""
    case, c = sc.solved(name), sc.CONDITIONS[name]
    figures = case.figures()
    assert case.volume.shape == c["shape"]
    assert case.volume.dtype == np.uint8 and not np.any(case.skeleton & ~case.volume)
    if "words_per_row" in c:
        assert -(-c["shape"][2] // so.WORD) == c["words_per_row"] and c["shape"][2] % so.WORD == c["tail"]
    if "min_words" in c:
        assert case.peak("words") > c["min_words"], figures
    if "min_open" in c:
        assert case.peak("open_words") > c["min_open"], figures
    if "max_open" in c:
        assert case.peak("open_words") <= c["max_open"], figures
    if "min_rounds" in c:
        assert case.peak("rounds") > c["min_rounds"], figures
    if "min_passes" in c:
        assert case.passes >= c["min_passes"], figures
    for recheck in c.get("differs", ()):
        wrong, _ = so.skeletonize_memo(case.volume, recheck=recheck)
        assert not np.array_equal(wrong, case.skeleton), f"{name} does not tell {recheck} from the definition"


def test_the_cases_named_in_the_gpu_file_exist():
    assert set(sc.GUARDED) <= set(sc.CASES)
    assert {r for c in sc.CONDITIONS.values() for r in c.get("differs", ())} == {"late_unchecked", "late_dropped", "no_carry"}


def test_a_difference_is_described_with_its_pass_direction_and_round():
    case = sc.solved("sheet_noise")
    assert sc.describe_difference(case, case.skeleton) == "sheet_noise: no voxel differs"
    wrong, _ = so.skeletonize_memo(case.volume, recheck="late_unchecked")
    text = sc.describe_difference(case, wrong)
    i, j, k = np.argwhere(wrong != case.skeleton)[0]
    t = case.trace
    assert text.startswith(f"sheet_noise: {int((wrong != case.skeleton).sum())} voxels differ")
    assert f"({i}, {j}, {k}) [word 0, bit {k}]: kernel {wrong[i, j, k]}, oracle {case.skeleton[i, j, k]}" in text
    assert f"pass {t.pass_[i, j, k]}, direction {t.direction[i, j, k]}, decided in round {t.round[i, j, k]}" in text
    assert "more, the last at" in text
    # a voxel the unchecked deletion removed was kept by the oracle's re-check, in a round the finish loop runs
    lost = (wrong == 0) & (case.skeleton == 1) & (t.kind == 1)
    assert lost.any() and (t.round[lost] > so.ROUND_LAUNCHES).any()


def test_workspace_query_is_pure_host():
    from seunet_amd import _lib
    lib = _lib.load()
    assert lib.seunet_skeleton_workspace_bytes(20, 24, 134) > 0
    assert lib.seunet_skeleton_workspace_bytes(1, 1, 70) > 0
    assert lib.seunet_skeleton_workspace_bytes(20, 0, 134) == 0
    assert "skeleton_workspace_bytes" in _lib.last_error()
    assert lib.seunet_skeleton_workspace_bytes(2048, 2048, 512) == 0         # 2^31 voxels
    assert "skeleton_workspace_bytes" in _lib.last_error()
