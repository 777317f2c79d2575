"""Host side of the stage-2/3 preparation (se-unet-airseg_amd/prep.py): CandidateSet against np.where on the fixture masks
(tests/golden/prep_known.npz, generated from the reference's own statements by scripts/make_golden_prep.py) and the samplers'
draws with a CandidateSet in place of the np.where triple.  No GPU needed."""
import os
import random

import numpy as np
import pytest


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "prep_known.npz"))


@pytest.fixture(scope="module")
def P():
    import seunet_amd
    return seunet_amd.prep


def _masks(g):
    out = []
    for c in range(int(g["ncase"])):
        p = f"case{c}_"
        out += [g[p + "loc_small"], g[p + "loc_skeleton"]]
        br = np.zeros(g[p + "label"].shape, bool)
        br[tuple(g[p + "loc_break"].astype(np.int64))] = True
        out.append(br)
    return out


def _same_as_where(P, mask):
    cs = P.CandidateSet.from_numpy(mask)
    ref = np.where(mask)
    assert len(cs) == len(cs[0]) == len(ref[0])
    got = np.array([cs.coords(k) for k in range(len(cs))], dtype=np.int64).reshape(-1, mask.ndim).T
    for ax in range(mask.ndim):
        assert np.array_equal(got[ax], ref[ax])
    for k in range(0, len(cs), max(1, len(cs) // 17)):
        assert tuple(int(cs[ax][k]) for ax in range(mask.ndim)) == tuple(int(r[k]) for r in ref)
    for a, b in zip(cs.to_numpy(), ref):
        assert np.array_equal(a, b)


def test_candidate_set_matches_np_where_on_fixture_masks(P, g):
    masks = _masks(g)
    assert any(m.all() for m in masks) and any(not m.any() for m in masks) and any(0 < m.sum() < m.size for m in masks)
    for m in masks:
        _same_as_where(P, m)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (2, 64, 9), (4, 33, 65)])
def test_candidate_set_empty_full_and_random(P, shape):
    rng = np.random.default_rng(sum(shape))
    for m in (np.zeros(shape, bool), np.ones(shape, bool), rng.random(shape) < 0.3, rng.random(shape) < 0.002):
        _same_as_where(P, m)
    cs = P.CandidateSet.from_numpy(np.ones(shape, bool))
    with pytest.raises(IndexError):
        cs.linear(int(np.prod(shape)))
    assert cs.coords(-1) == tuple(s - 1 for s in shape)


def test_samplers_draw_the_same_with_candidate_sets(P, g):
    import seunet_amd as A
    for c in range(int(g["ncase"]) - 1):
        p = f"case{c}_"
        masks = [g[p + "loc_skeleton"], g[p + "loc_small"]]
        br = np.zeros(g[p + "label"].shape, bool)
        br[tuple(g[p + "loc_break"].astype(np.int64))] = True
        masks.append(br)
        shape = (40, 48, 52)                       # any volume at least one cube wide: the draws only index the lists
        triples = [np.where(m) for m in masks]
        sets = [P.CandidateSet.from_numpy(m) for m in masks]
        for seed in (1, 2, 3):
            plans = []
            for locs in (triples, sets):
                random.seed(seed)
                np.random.seed(100 + seed)
                plans.append((A.draw_stage2_plan(shape, 6, locs[0], locs[1], cube=16, hard_ratio=0.9),
                              A.draw_stage3_plan(shape, 6, locs[0], locs[1], locs[2], cube=16, hard_ratio=0.9)))
            for a, b in zip(*plans):
                assert a["starts"] == b["starts"] and a["kinds"] == b["kinds"] and a["codes"] == b["codes"] and a["u"] == b["u"]


def test_lib_table_is_the_reference_arithmetic(P):
    t = P.lib_table()
    assert t.dtype == np.float32 and t.shape == (344,)
    k = np.arange(344, dtype=np.float32)
    conv = k / np.float32(343)                    # lib_weight.py:14-16
    conv[conv == 0] = 1
    assert np.array_equal(t.view(np.int32), (-np.log10(conv)).view(np.int32))
    assert np.signbit(t[0]) and np.signbit(t[343]) and t[0] == 0


def test_fixture_edt_indices_are_scipys(g):
    ndimage = pytest.importorskip("scipy.ndimage")
    for i in range(int(g["nedt"])):
        dist, ind = ndimage.distance_transform_edt(g[f"edt{i}_vol"], return_indices=True)
        assert np.array_equal(ind, g[f"edt{i}_ind"].astype(np.int32))
        assert np.array_equal(dist.view(np.int64), g[f"edt{i}_dist"].view(np.int64))
