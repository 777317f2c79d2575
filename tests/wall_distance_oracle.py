"""The per-branch wall distance tables (include/seunet_hip.h, seunet_branch_wall_stats) in plain numpy: the
oracle csrc/morphometry.hip's wall pass and ``seunet_amd.branch_wall_distance`` are tested against.

Over the voxels with ``skeleton != 0``, a label k in 1..num and a feature (``indices[0] >= 0``):
``wall_count[k]`` their number; ``offset_sq_sum[k, a]`` the sum of ``(indices[a] - coordinate_a)**2``; ``wall_sq_min[k]`` /
``wall_sq_max[k]`` the minimum / maximum of ``(dt_0**2 + dt_1**2) + dt_2**2`` with ``dt_a = float64(indices[a] - coordinate_a) *
spacing[a]`` (none: +inf / 0.0).  Rows 1..num, as the package returns them.  A skeleton voxel whose label is outside 0..num is
ignored and sets the status."""
import numpy as np

TABLES = ("wall_count", "offset_sq_sum", "wall_sq_min", "wall_sq_max")


def wall_distance(parsing, skeleton, indices, spacing, num):
    """-> (tables with rows 1..num, status)."""
    parsing = np.asarray(parsing).astype(np.int64)
    skeleton = np.asarray(skeleton) != 0
    indices = np.asarray(indices).astype(np.int64)
    s = np.asarray(spacing, dtype=np.float64).reshape(3)
    bad = skeleton & ((parsing < 0) | (parsing > num))
    use = skeleton & (parsing >= 1) & (parsing <= num) & (indices[0] >= 0)
    off = indices - np.indices(parsing.shape)
    dt = off.astype(np.float64)
    for a in range(3):
        dt[a] = dt[a] * s[a]
    dt = dt * dt
    sq = (dt[0] + dt[1]) + dt[2]
    t = {"wall_count": np.zeros(num, np.int64), "offset_sq_sum": np.zeros((num, 3), np.int64),
         "wall_sq_min": np.full(num, np.inf, np.float64), "wall_sq_max": np.zeros(num, np.float64)}
    for k in range(1, num + 1):
        m = use & (parsing == k)
        if not m.any():
            continue
        t["wall_count"][k - 1] = int(m.sum())
        for a in range(3):
            t["offset_sq_sum"][k - 1, a] = int((off[a][m] ** 2).sum())
        t["wall_sq_min"][k - 1] = sq[m].min()
        t["wall_sq_max"][k - 1] = sq[m].max()
    return t, int(bad.any())


def hand_case():
    """A 3 x 3 x 4 case small enough to do by hand -> (parsing, skeleton, indices, spacing, num, tables written out by hand).
    spacing (2, 1, 0.5); `indices` is chosen freely, it need not be a distance transform of anything.
      label 1: (1, 1, 1) -> (0, 1, 1): offset (-1, 0, 0), squares (1, 0, 0), (2)^2 = 4.0
               (1, 1, 2) -> (1, 2, 3): offset (0, 1, 1), squares (0, 1, 1), (0 + 1) + 0.25 = 1.25
      label 2: (0, 0, 0) -> (2, 0, 2): offset (2, 0, 2), squares (4, 0, 4), (16 + 0) + 1 = 17.0
               (2, 2, 3) has no feature (-1): not measured
      label 3: one voxel, not on the skeleton; label 4: no voxel; (0, 2, 2): on the skeleton with parsing 0, ignored."""
    shape = (3, 3, 4)
    parsing = np.zeros(shape, np.int32)
    skeleton = np.zeros(shape, np.uint8)
    indices = np.indices(shape).astype(np.int32)
    parsing[1, 1, 1] = parsing[1, 1, 2] = 1
    parsing[0, 0, 0] = parsing[2, 2, 3] = 2
    parsing[1, 0, 0] = 3
    for p in ((1, 1, 1), (1, 1, 2), (0, 0, 0), (2, 2, 3), (0, 2, 2)):
        skeleton[p] = 1
    indices[:, 1, 1, 1] = (0, 1, 1)
    indices[:, 1, 1, 2] = (1, 2, 3)
    indices[:, 0, 0, 0] = (2, 0, 2)
    indices[:, 2, 2, 3] = -1
    indices[:, 0, 2, 2] = (2, 2, 2)
    tables = {"wall_count": np.array([2, 1, 0, 0], np.int64),
              "offset_sq_sum": np.array([[1, 1, 1], [4, 0, 4], [0, 0, 0], [0, 0, 0]], np.int64),
              "wall_sq_min": np.array([1.25, 17.0, np.inf, np.inf], np.float64),
              "wall_sq_max": np.array([4.0, 17.0, 0.0, 0.0], np.float64)}
    return parsing, skeleton, indices, (2.0, 1.0, 0.5), 4, tables


def radii(tables, spacing):
    """The three inscribed radii of ``BranchTable`` in physical mode, label by label in plain Python."""
    s = [float(v) for v in spacing]
    num = len(tables["wall_count"])
    out = {k: np.full(num, np.nan, dtype=np.float64) for k in ("radius_inscribed_rms", "radius_inscribed_min", "radius_inscribed_max")}
    for k in range(num):
        n = int(tables["wall_count"][k])
        if n == 0:
            continue
        q = [float(tables["offset_sq_sum"][k, a]) for a in range(3)]
        out["radius_inscribed_rms"][k] = np.sqrt((s[0] * s[0] * q[0] + s[1] * s[1] * q[1] + s[2] * s[2] * q[2]) / n)
        out["radius_inscribed_min"][k] = np.sqrt(float(tables["wall_sq_min"][k]))
        out["radius_inscribed_max"][k] = np.sqrt(float(tables["wall_sq_max"][k]))
    return out


def same_tables(got, want):
    """Bitwise equality of the four tables (float64 through their bit patterns)."""
    for k in TABLES:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(np.ascontiguousarray(g).view(np.int64), np.ascontiguousarray(w).view(np.int64)), (k, g, w)
