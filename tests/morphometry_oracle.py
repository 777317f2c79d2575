"""The definition of the branch morphometry (include/seunet_hip.h, seunet_branch_stats) in plain numpy: the
oracle csrc/morphometry.hip and seunet_amd.morphometry are tested against.  The reference has no such function, so this file is
the statement of what the numbers are.  ``branch_stats`` is vectorised (``bincount`` over shifted views); ``branch_stats_brute`` is
the same definition as a triple loop for tiny volumes, which tests/test_morphometry_host.py holds the vectorised one against.

Tables have one row per label 0..num (row 0 holds the empty values); ``rows_from_one`` drops row 0 as the package does."""
import itertools

import numpy as np

OFFSETS = tuple(d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0))     # ascending: class 0 = (0, 0, 1)
INT32_MAX = 2 ** 31 - 1
INT_TABLES = ("voxels", "coord_sum", "box_min", "box_max", "skeleton_voxels", "links", "cross_links", "r2_sum", "r2_min", "r2_max")
FLOAT_COLUMNS = ("volume", "centroid", "length", "radius_equivalent", "radius_inscribed_rms", "radius_inscribed_min",
                 "radius_inscribed_max")


def intermediates(d):
    """p + these offsets are the voxels that make the link (p, p + d) a shortcut: the proper non-empty parts of d."""
    axes = [a for a in range(3) if d[a]]
    out = []
    for r in range(1, len(axes)):
        for part in itertools.combinations(axes, r):
            out.append(tuple(d[a] if a in part else 0 for a in range(3)))
    return out


def _empty(num, shape):
    rows = num + 1
    t = {"voxels": np.zeros(rows, np.int64), "coord_sum": np.zeros((rows, 3), np.int64),
         "box_min": np.tile(np.asarray(shape, np.int32), (rows, 1)), "box_max": np.full((rows, 3), -1, np.int32),
         "skeleton_voxels": np.zeros(rows, np.int64), "links": np.zeros((rows, 13), np.int64),
         "cross_links": np.zeros((rows, 13), np.int64), "r2_sum": np.zeros(rows, np.int64),
         "r2_min": np.full(rows, INT32_MAX, np.int32), "r2_max": np.full(rows, -1, np.int32)}
    return t


def _shifted(a, d):
    """(a[p], a[p + d]) over every p with p + d inside the volume, as two views."""
    lo = tuple(slice(max(0, -d[k]), a.shape[k] - max(0, d[k])) for k in range(3))
    hi = tuple(slice(max(0, d[k]), a.shape[k] - max(0, -d[k])) for k in range(3))
    return a[lo], a[hi]


def branch_stats(parsing, skeleton, num, sqdist=None):
    """-> (tables, status).  A voxel whose label is outside 0..num is ignored everywhere and sets status to 1."""
    parsing = np.asarray(parsing).astype(np.int64)
    shape = parsing.shape
    bad = (parsing < 0) | (parsing > num)
    lab = np.where(bad, 0, parsing)
    t = _empty(num, shape)
    fg = lab > 0
    idx = np.nonzero(fg)
    ks = lab[idx]
    t["voxels"] = np.bincount(ks, minlength=num + 1).astype(np.int64)
    for a in range(3):
        np.add.at(t["coord_sum"][:, a], ks, idx[a].astype(np.int64))
        np.minimum.at(t["box_min"][:, a], ks, idx[a].astype(np.int32))
        np.maximum.at(t["box_max"][:, a], ks, idx[a].astype(np.int32))
    sk = np.where((np.asarray(skeleton) != 0) & fg, lab, 0)              # the label of a labelled skeleton voxel, else 0
    sidx = np.nonzero(sk)
    sks = sk[sidx]
    t["skeleton_voxels"] = np.bincount(sks, minlength=num + 1).astype(np.int64)
    if sqdist is not None:
        r2 = np.asarray(sqdist)[sidx].astype(np.int64)
        np.add.at(t["r2_sum"], sks, r2)
        np.minimum.at(t["r2_min"], sks, r2.astype(np.int32))
        np.maximum.at(t["r2_max"], sks, r2.astype(np.int32))
    pad = np.pad(sk, 1)                                                  # a ring of background: every neighbour exists
    core = tuple(slice(1, 1 + s) for s in shape)
    for c, d in enumerate(OFFSETS):
        there = pad[tuple(slice(1 + d[k], 1 + d[k] + shape[k]) for k in range(3))]
        link = (pad[core] > 0) & (there > 0)
        for m in intermediates(d):
            link &= pad[tuple(slice(1 + m[k], 1 + m[k] + shape[k]) for k in range(3))] == 0
        a, b = pad[core][link], there[link]
        t["links"][:, c] = np.bincount(a[a == b], minlength=num + 1)
        t["cross_links"][:, c] = np.bincount(a[a != b], minlength=num + 1) + np.bincount(b[a != b], minlength=num + 1)
    return t, int(bad.any())


def branch_stats_brute(parsing, skeleton, num, sqdist=None):
    """The same definition voxel by voxel (tiny volumes only)."""
    parsing = np.asarray(parsing)
    n0, n1, n2 = parsing.shape
    t = _empty(num, parsing.shape)
    status = 0

    def lsk(i, j, k):
        if not (0 <= i < n0 and 0 <= j < n1 and 0 <= k < n2) or skeleton[i, j, k] == 0:
            return 0
        v = int(parsing[i, j, k])
        return v if 1 <= v <= num else 0

    for i in range(n0):
        for j in range(n1):
            for k in range(n2):
                v = int(parsing[i, j, k])
                if v < 0 or v > num:
                    status = 1
                    continue
                if v == 0:
                    continue
                p = (i, j, k)
                t["voxels"][v] += 1
                for a in range(3):
                    t["coord_sum"][v, a] += p[a]
                    t["box_min"][v, a] = min(t["box_min"][v, a], p[a])
                    t["box_max"][v, a] = max(t["box_max"][v, a], p[a])
                if lsk(i, j, k) == 0:
                    continue
                t["skeleton_voxels"][v] += 1
                if sqdist is not None:
                    r2 = int(sqdist[i, j, k])
                    t["r2_sum"][v] += r2
                    t["r2_min"][v] = min(t["r2_min"][v], r2)
                    t["r2_max"][v] = max(t["r2_max"][v], r2)
                for c, d in enumerate(OFFSETS):
                    w = lsk(i + d[0], j + d[1], k + d[2])
                    if w == 0 or any(lsk(i + m[0], j + m[1], k + m[2]) for m in intermediates(d)):
                        continue
                    if w == v:
                        t["links"][v, c] += 1
                    else:
                        t["cross_links"][v, c] += 1
                        t["cross_links"][w, c] += 1
    return t, status


def rows_from_one(tables):
    return {k: v[1:] for k, v in tables.items()}


def total_links(skeleton_mask):
    """Counted links of a skeleton regardless of labels: what one label over the whole mask would give, summed over the classes."""
    sk = (np.asarray(skeleton_mask) != 0).astype(np.int64)
    t, _ = branch_stats(sk, sk, 1)
    return int(t["links"][1].sum())


def link_lengths(spacing):
    return np.array([np.sqrt(sum((d[a] * float(spacing[a])) ** 2 for a in range(3))) for d in OFFSETS], dtype=np.float64)


def derived(rows, spacing):
    """The float64 columns of seunet_amd.morphometry.BranchTable from integer rows 1..num, label by label in plain Python."""
    num = len(rows["voxels"])
    s = [float(v) for v in spacing]
    ell = link_lengths(spacing)
    out = {k: np.full((num, 3) if k == "centroid" else num, np.nan, dtype=np.float64) for k in FLOAT_COLUMNS}
    for k in range(num):
        n = int(rows["voxels"][k])
        out["volume"][k] = n * (s[0] * s[1] * s[2])
        if n:
            out["centroid"][k] = [int(rows["coord_sum"][k, a]) / n * s[a] for a in range(3)]
        length = 0.0
        for c in range(13):
            length += float(rows["links"][k, c]) * ell[c]
        half = 0.0
        for c in range(13):
            half += float(rows["cross_links"][k, c]) * ell[c]
        length += 0.5 * half
        out["length"][k] = length
        if length > 0:
            out["radius_equivalent"][k] = np.sqrt(out["volume"][k] / (np.pi * length))
        m = int(rows["skeleton_voxels"][k])
        if m and rows["r2_max"][k] >= 0:
            out["radius_inscribed_rms"][k] = np.sqrt(int(rows["r2_sum"][k]) / m)
            out["radius_inscribed_min"][k] = np.sqrt(float(rows["r2_min"][k]))
            out["radius_inscribed_max"][k] = np.sqrt(float(rows["r2_max"][k]))
    return out


def branch_tree(counts, adjacency):
    """Root = the most voxels (lowest label on a tie); breadth-first by levels, a level in ascending label order, the first label to
    reach another is its parent.  -> (parent, generation, n_children), label values, 0 root, -1 empty or unreachable."""
    num = len(counts)
    parent, gen, kids = [-1] * num, [-1] * num, [0] * num
    if num and max(counts) > 0:
        root = min(k for k in range(num) if counts[k] == max(counts))
        parent[root], gen[root] = 0, 0
        level = [root]
        while level:
            nxt = []
            for cur in sorted(level):
                for ch in range(num):
                    if (adjacency[cur][ch] or adjacency[ch][cur]) and gen[ch] < 0 and counts[ch] > 0:
                        parent[ch], gen[ch] = cur + 1, gen[cur] + 1
                        kids[cur] += 1
                        nxt.append(ch)
            level = nxt
    return np.array(parent, np.int32), np.array(gen, np.int32), np.array(kids, np.int32)


def adjacency(parsing, num):
    """(num, num) bool: labels i + 1 and j + 1 meet across a face."""
    parsing = np.asarray(parsing)
    ad = np.zeros((num + 1, num + 1), dtype=bool)
    for d in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
        a, b = _shifted(parsing, d)
        m = (a > 0) & (b > 0) & (a != b) & (a <= num) & (b <= num)
        ad[a[m], b[m]] = True
        ad[b[m], a[m]] = True
    return ad[1:, 1:]
