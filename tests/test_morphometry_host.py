"""The branch morphometry without a GPU: the numpy oracle (tests/morphometry_oracle.py) against its own brute-force statement and
against known answers (straight lines, the L-corner, the corner diagonal), and the host half of seunet_amd.morphometry --
``branch_tree`` on hand-made adjacencies, the derived columns of ``BranchTable.from_stats`` from hand-made integer tables."""
import numpy as np
import pytest

import morphometry_oracle as mo

from seunet_amd import morphometry as M
import seunet_amd


def test_exports_and_link_classes():
    for name in ("branch_stats", "branch_tree", "branch_morphometry", "BranchTable"):
        assert getattr(seunet_amd, name) is getattr(M, name) and name in seunet_amd.__all__
    assert M.LINK_OFFSETS == mo.OFFSETS and len(mo.OFFSETS) == 13
    assert mo.OFFSETS[0] == (0, 0, 1) and mo.OFFSETS[1] == (0, 1, -1) and mo.OFFSETS[12] == (1, 1, 1)
    assert list(mo.OFFSETS) == sorted(mo.OFFSETS)
    assert [len(mo.intermediates(d)) for d in mo.OFFSETS] == [{1: 0, 2: 2, 3: 6}[sum(map(abs, d))] for d in mo.OFFSETS]


@pytest.mark.parametrize("seed", range(6))
def test_oracle_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    num = (1, 2, 3, 5, 7, 4)[seed]
    shape = (4, 5, 6)
    parsing = rng.integers(0, num + 1, shape).astype(np.int32)
    if seed == 5:                                            # labels outside 0..num: ignored, status 1
        parsing[1, 2, 3], parsing[0, 0, 0] = num + 1, -2
    skeleton = (rng.random(shape) < (0.25, 0.5, 0.8, 0.35, 1.0, 0.5)[seed]).astype(np.uint8)
    sqdist = rng.integers(0, 50, shape).astype(np.int32)
    for sq in (sqdist, None):
        fast, st_fast = mo.branch_stats(parsing, skeleton, num, sq)
        slow, st_slow = mo.branch_stats_brute(parsing, skeleton, num, sq)
        assert st_fast == st_slow == (1 if seed == 5 else 0)
        for k in mo.INT_TABLES:
            assert fast[k].dtype == slow[k].dtype and np.array_equal(fast[k], slow[k]), k
    assert fast["cross_links"].sum() % 2 == 0
    assert np.array_equal(fast["voxels"][1:], [(parsing == k).sum() for k in range(1, num + 1)])


@pytest.mark.parametrize("c", range(13))
def test_a_straight_line_has_m_minus_1_links_of_its_class(c):
    d = mo.OFFSETS[c]
    m = 5
    v = np.zeros((5, 5, 5), dtype=np.int32)
    start = [0 if d[a] >= 0 else m - 1 for a in range(3)]
    for t in range(m):
        v[tuple(start[a] + t * d[a] for a in range(3))] = 1
    t, status = mo.branch_stats(v, v, 1, None)
    want = np.zeros(13, dtype=np.int64)
    want[c] = m - 1
    assert status == 0 and np.array_equal(t["links"][1], want) and not t["cross_links"].any()
    assert t["skeleton_voxels"][1] == m == t["voxels"][1]


def test_l_corner_and_corner_diagonal():
    v = np.zeros((3, 3, 3), dtype=np.int32)
    v[1, 1, 0] = v[1, 1, 1] = v[1, 2, 1] = 1                 # an L: two face links, the edge diagonal across it is a shortcut
    t, _ = mo.branch_stats(v, v, 1)
    assert t["links"][1].sum() == 2 and t["links"][1, 0] == 1 and t["links"][1, 2] == 1
    v = np.zeros((3, 3, 3), dtype=np.int32)
    v[0, 0, 0] = v[1, 1, 1] = 1                              # a free corner diagonal counts ...
    t, _ = mo.branch_stats(v, v, 1)
    assert t["links"][1].sum() == 1 and t["links"][1, 12] == 1
    v[0, 1, 1] = 2                                           # ... until one of its six intermediate voxels is occupied, by any label
    t, _ = mo.branch_stats(v, v, 2)
    assert t["links"][1].sum() == 0
    assert t["cross_links"][1].sum() == 2 and t["cross_links"][2].sum() == 2     # (0,0,0)-(0,1,1) and (0,1,1)-(1,1,1)


def test_a_link_between_two_labels_is_credited_to_both():
    v = np.zeros((1, 1, 8), dtype=np.int32)
    v[0, 0, 1:4], v[0, 0, 4:7] = 1, 2
    sk = (v > 0).astype(np.uint8)
    sk[0, 0, 6] = 0                                          # a voxel off the skeleton has no links
    t, _ = mo.branch_stats(v, sk, 2)
    assert np.array_equal(t["links"][:, 0], [0, 2, 1]) and np.array_equal(t["cross_links"][:, 0], [0, 1, 1])
    assert mo.total_links(sk) == 4 == t["links"].sum() + t["cross_links"].sum() // 2


def test_branch_tree_chain_star_tie_unreachable_empty():
    def adj(num, pairs):
        a = np.zeros((num, num), dtype=np.uint8)
        for i, j in pairs:
            a[i - 1, j - 1] = a[j - 1, i - 1] = 1
        return a

    # a chain 1 - 2 - 3 - 4 rooted at its largest label, 2
    p, g, c = M.branch_tree([5, 9, 3, 2], adj(4, [(1, 2), (2, 3), (3, 4)]))
    assert p.dtype == g.dtype == c.dtype == np.int32
    assert p.tolist() == [2, 0, 2, 3] and g.tolist() == [1, 0, 1, 2] and c.tolist() == [0, 2, 1, 0]
    # a star around 3
    p, g, c = M.branch_tree([1, 1, 7, 1, 1], adj(5, [(3, 1), (3, 2), (3, 4), (3, 5)]))
    assert p.tolist() == [3, 3, 0, 3, 3] and g.tolist() == [1, 1, 0, 1, 1] and c.tolist() == [0, 0, 4, 0, 0]
    # a tie for the root goes to the lowest label; 4 touches both 2 and 3 of the same level: the first to reach it, 2, is its parent
    p, g, c = M.branch_tree([6, 2, 6, 1], adj(4, [(1, 2), (1, 3), (2, 4), (3, 4)]))
    assert p.tolist() == [0, 1, 1, 2] and g.tolist() == [0, 1, 1, 2] and c.tolist() == [2, 1, 0, 0]
    # label 4 touches nothing: unreachable; label 3 is empty, so it is no bridge to 5 either
    p, g, c = M.branch_tree([4, 3, 0, 2, 1], adj(5, [(1, 2), (2, 3), (3, 5)]))
    assert p.tolist() == [0, 1, -1, -1, -1] and g.tolist() == [0, 1, -1, -1, -1] and c.tolist() == [1, 0, 0, 0, 0]
    # no label at all, and only empty labels
    assert all(a.size == 0 for a in M.branch_tree([], np.zeros((0, 0))))
    p, g, c = M.branch_tree([0, 0], np.zeros((2, 2)))
    assert p.tolist() == [-1, -1] and g.tolist() == [-1, -1] and c.tolist() == [0, 0]
    for counts, a in (([5, 9, 3, 2], adj(4, [(1, 2), (2, 3), (3, 4)])), ([6, 2, 6, 1], adj(4, [(1, 2), (1, 3), (2, 4), (3, 4)]))):
        for got, want in zip(M.branch_tree(counts, a), mo.branch_tree(counts, a)):
            assert np.array_equal(got, want)


def _tables(num):
    t = mo.rows_from_one(mo._empty(num, (9, 9, 9)))
    return {k: v.copy() for k, v in t.items()}


def test_derived_columns_from_hand_made_tables():
    t = _tables(3)
    spacing = (2.0, 0.5, 1.0)
    # label 1: 10 voxels, 3 links along axis 2, 2 along (1, 1, 0), one cross link along axis 0; label 2 its partner; label 3 empty
    t["voxels"][:] = [10, 4, 0]
    t["coord_sum"][0], t["coord_sum"][1] = (30, 20, 45), (4, 8, 2)
    t["skeleton_voxels"][:] = [6, 1, 0]
    t["links"][0, 0], t["links"][0, 11] = 3, 2
    t["cross_links"][0, 8] = t["cross_links"][1, 8] = 1
    t["r2_sum"][:2], t["r2_min"][:2], t["r2_max"][:2] = (54, 4), (4, 4), (16, 4)
    ad = np.zeros((3, 3), dtype=np.uint8)
    ad[0, 1] = ad[1, 0] = 1
    b = M.BranchTable.from_stats(t, ad, spacing)
    diag = np.sqrt(2.0 ** 2 + 0.5 ** 2)
    assert b.num == 3 and b.spacing == spacing
    assert np.array_equal(b.volume, [10.0, 4.0, 0.0])
    assert np.array_equal(b.centroid[0], [6.0, 1.0, 4.5]) and np.array_equal(b.centroid[1], [2.0, 1.0, 0.5]) and np.isnan(b.centroid[2]).all()
    np.testing.assert_allclose(b.length, [3 * 1.0 + 2 * diag + 0.5 * 2.0, 0.5 * 2.0, 0.0], rtol=1e-15)
    np.testing.assert_allclose(b.radius_equivalent[:2], [np.sqrt(10.0 / (np.pi * b.length[0])), np.sqrt(4.0 / np.pi)], rtol=1e-15)
    assert np.isnan(b.radius_equivalent[2])
    assert np.array_equal(b.radius_inscribed_rms[:2], [3.0, 2.0]) and np.array_equal(b.radius_inscribed_min[:2], [2.0, 2.0])
    assert np.array_equal(b.radius_inscribed_max[:2], [4.0, 2.0])
    assert np.isnan([b.radius_inscribed_rms[2], b.radius_inscribed_min[2], b.radius_inscribed_max[2]]).all()
    assert b.parent.tolist() == [0, 1, -1] and b.generation.tolist() == [0, 1, -1] and b.n_children.tolist() == [1, 0, 0]
    assert b.is_leaf.tolist() == [False, True, False]
    assert (b.n_branches, b.n_leaves, b.max_generation) == (2, 1, 1) and b.branches_per_generation.tolist() == [1, 1]
    assert b.total_length == pytest.approx(b.length.sum(), rel=1e-15)
    d = b.to_dict()
    assert d["links"] is b.links and d["n_leaves"] == 1 and set(mo.INT_TABLES) | set(mo.FLOAT_COLUMNS) <= set(d)
    want = mo.derived(t, spacing)
    for k in mo.FLOAT_COLUMNS:
        np.testing.assert_allclose(getattr(b, k), want[k], rtol=1e-12, equal_nan=True)
    # without sqdist the radius columns of a label with skeleton voxels are nan too; an empty tree has no generation
    t["r2_sum"][:], t["r2_min"][:], t["r2_max"][:] = 0, mo.INT32_MAX, -1
    assert np.isnan(M.BranchTable.from_stats(t, ad).radius_inscribed_rms).all()
    e = M.BranchTable.from_stats(_tables(2), np.zeros((2, 2)))
    assert (e.n_branches, e.n_leaves, e.max_generation, e.total_length) == (0, 0, -1, 0.0) and e.branches_per_generation.size == 0
    with pytest.raises(ValueError):
        M.BranchTable.from_stats(t, ad, (1.0, 0.0, 1.0))


def test_link_lengths():
    s = (0.7, 0.8, 1.25)
    got = M.link_lengths(s)
    assert got.dtype == np.float64 and np.array_equal(got, mo.link_lengths(s))
    assert got[0] == 1.25 and got[2] == 0.8 and got[8] == 0.7 and got[12] == np.sqrt(0.7 ** 2 + 0.8 ** 2 + 1.25 ** 2)
