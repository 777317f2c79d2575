"""tests/pool_oracle.py against the reference's recorded behaviour (tests/golden/online_pool_known.npz, made by
scripts/make_golden_online_pool.py from the reference's own save_data_online / save_data_online3 / OnlineHMData statements on
distinct keys) -- exact equality of the surviving ids after every call and of every replay selection -- and against the
project's own rules where the reference is not well defined (ties, a key equal to the minimum, non-finite keys, several
samples of one call chasing one slot).  CPU only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pool_oracle import PoolOracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "online_pool_known.npz")


@pytest.fixture(scope="module")
def known():
    return np.load(GOLDEN)


def test_fixture_covers_every_branch(known):
    assert int(known["nrun"]) == 12
    configs = {tuple(int(v) for v in known[f"run{r}_config"]) for r in range(12)}
    assert configs == {(t, B, K) for t in (0, 1) for B in (3, 4) for K in (1, 7, 10)}
    rates = known["rates"].tolist()
    assert 1.0 in rates and any(int(r * 10) == 0 for r in rates)
    for r in range(12):
        keys = known[f"run{r}_keys"]
        assert keys.dtype == np.float32 and keys.shape[0] == 40 and len(set(keys.reshape(-1).tolist())) == keys.size      # distinct


@pytest.mark.parametrize("run", range(12))
def test_oracle_reproduces_the_reference(known, run):
    _, B, K = (int(v) for v in known[f"run{run}_config"])
    keys, survivors = known[f"run{run}_keys"], known[f"run{run}_survivors"]
    pool = PoolOracle(K)
    branches = set()
    for it in range(keys.shape[0]):
        full_before = pool.count == K
        slots = pool.add(keys[it].tolist(), payloads=list(range(it * B, (it + 1) * B)))
        assert len(slots) == B and len({s for s in slots if s >= 0}) == sum(s >= 0 for s in slots)
        want = [int(v) for v in survivors[it] if v >= 0]
        assert sorted(pool.stored()) == want, (it, sorted(pool.stored()), want)
        branches.add(("full" if full_before else "filling", "skip" if -1 in slots else "keep"))
        if pool.count == K and not full_before:
            branches.add("became full")
    assert {("full", "skip"), "became full"} <= branches and (K < B or ("filling", "keep") in branches)
    assert pool.count == K and pool.next >= K
    for k, rate in enumerate(known["rates"].tolist()):
        got = [pool.payload[j] for j in pool.replay_slots(rate)]
        assert got == known[f"run{run}_replay{k}"].tolist(), (rate, got)
    assert len(pool.replay_slots(0.05)) == K                                       # int(0.05 * K) == 0 selects everything


def filled(keys):
    pool = PoolOracle(len(keys))
    assert pool.add(keys) == list(range(len(keys)))
    return pool


def test_tie_evicts_the_oldest():
    pool = filled([2.0, 1.0, 1.0, 3.0])
    assert pool.add([5.0]) == [1] and pool.add([6.0]) == [2]
    pool = filled([1.0, 1.0, 1.0])
    assert pool.add([1.0, 1.0]) == [0, 1]                     # equal keys of one call are all kept: nothing is overwritten
    assert pool.add([1.0]) == [2] and pool.add([1.0]) == [0]  # the oldest is now the first of that call
    assert -0.0 == 0.0 and filled([0.0, -0.0]).add([0.0]) == [0]


def test_key_equal_to_the_minimum_is_accepted_and_a_smaller_one_is_not():
    pool = filled([5.0, 6.0])
    assert pool.add([5.0]) == [0] and pool.keys == [5.0, 6.0] and pool.seq == [2, 1]
    assert pool.add([math.nextafter(5.0, 0.0)]) == [-1] and pool.next == 3


def test_non_finite_keys_are_skipped():
    pool = PoolOracle(3)
    assert pool.add([float("nan"), 1.0, float("inf"), float("-inf"), 2.0]) == [-1, 0, -1, -1, 1]
    assert (pool.count, pool.next, pool.keys[:2], pool.seq[:2]) == (2, 2, [1.0, 2.0], [0, 1])
    pool.add([3.0])
    assert pool.add([float("nan"), float("inf")]) == [-1, -1] and pool.keys == [1.0, 2.0, 3.0]


def test_in_call_chain():
    pool = filled([5.0, 6.0])                                  # a = slot of 5, b = slot of 6
    a, b = 0, 1
    assert pool.add([7.0, 8.0, 9.0]) == [-1, b, a]            # 7 takes a, 8 takes b, 9 takes a back from 7
    assert pool.keys == [9.0, 8.0] and pool.seq == [4, 3] and pool.next == 5


def test_capacity_zero_and_clear():
    pool = PoolOracle(0)
    assert pool.add([1.0, float("nan"), 2.0]) == [-1, -1, -1] and (pool.count, pool.next) == (0, 0) and pool.replay_slots() == []
    pool = filled([1.0, 2.0])
    pool.clear()
    assert (pool.count, pool.next) == (0, 0) and pool.add([0.5]) == [0] and pool.replay_slots() == [0]


def test_replay_batches():
    pool = filled([3.0, 1.0, 2.0, 1.0, 5.0])
    assert pool.replay_slots() == [1, 3, 2, 0, 4]
    assert pool.replay_slots(0.5) == [0, 4] and pool.replay_slots(0.1) == [1, 3, 2, 0, 4] and pool.replay_slots(7.0) == [1, 3, 2, 0, 4]
    assert pool.replay_batches([4, 0, 2, 1, 3], batch_size=2) == [[4, 1], [2, 3]]
    assert pool.replay_batches([1, 0], batch_size=1, rate=0.5) == [[4], [0]]
