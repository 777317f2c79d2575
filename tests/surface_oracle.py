"""The surface distances and the boundary metrics built on them, stated in numpy: the oracle
csrc/surface.hip, ``seunet_amd.surface_distances``, ``order_statistics`` and ``surface_metrics`` are tested against.

Let ``A`` and ``B`` be masks of one shape (non-zero = 1) and ``s`` the voxel spacing.

* ``border(M) = M & ~binary_erosion(M)`` with the 6-neighbour cross, one iteration, outside the volume = 0 (scipy's default
  ``border_value``): a set voxel on a face of the volume is a border voxel.  MedPy's ``__surface_distances`` with
  ``connectivity=1``.  Stated with shifted slices below; nothing here imports scipy.
* ``d_AB = distance_transform_edt(~border(B), sampling=s)[border(A)]``: float64, in raster order of ``A``'s border voxels; the
  transform is tests/edt_sampling_oracle.py (scipy's, bit for bit).  ``d_BA`` is the mirror image.  ``D`` is ``d_AB`` followed by
  ``d_BA``.
* ``hd = max(D)``; ``hd_percentile = max(P(d_AB, q), P(d_BA, q))``; ``hd_percentile_pooled = P(D, q)`` (MedPy's ``hd95``);
  ``asd_ab = mean(d_AB)``, ``asd_ba = mean(d_BA)``, ``assd = sum(D) / (n_a + n_b)``; ``nsd[t] = #{D <= t} / (n_a + n_b)``.
* ``P`` is numpy's default (linear) percentile, restated in ``percentile`` as numpy 2.2 computes it.

Pure Python loops in the transform: meant for volumes of a few ten thousand voxels."""
import math

import numpy as np

import edt_sampling_oracle as eo


def border(mask):
    """bool: the set voxels with one of the six neighbours unset or outside the volume."""
    m = np.asarray(mask) != 0
    assert m.ndim == 3
    eroded = m.copy()
    for axis in range(3):
        lower = np.zeros_like(m)                               # the neighbour at index - 1 (outside: 0)
        upper = np.zeros_like(m)                               # the neighbour at index + 1
        dst, src = [slice(None)] * 3, [slice(None)] * 3
        dst[axis], src[axis] = slice(1, None), slice(None, -1)
        lower[tuple(dst)] = m[tuple(src)]
        upper[tuple(src)] = m[tuple(dst)]
        eroded &= lower & upper
    return m & ~eroded


def directed(a_border, b_border, spacing):
    """float64: the distance of every voxel of ``a_border``, in raster order, to the nearest voxel of ``b_border``."""
    dist, _ = eo.edt((~b_border).astype(np.uint8), spacing)
    return dist[a_border]


def surface_distances(a, b, spacing=(1.0, 1.0, 1.0)):
    """-> (D float64, n_a, n_b, voxels int32): ``d_AB`` then ``d_BA``; ``voxels``: the linear index of each border voxel."""
    ba, bb = border(a), border(b)
    assert ba.any() and bb.any(), "a mask without voxels has no surface distances"
    s = [float(v) for v in spacing]
    d_ab, d_ba = directed(ba, bb, s), directed(bb, ba, s)
    voxels = np.concatenate([np.flatnonzero(ba), np.flatnonzero(bb)]).astype(np.int32)
    return np.concatenate([d_ab, d_ba]), int(d_ab.size), int(d_ba.size), voxels


def percentile(values, q):
    """numpy's default percentile of a non-empty float64 vector, as numpy 2.2 computes it."""
    x = np.sort(np.asarray(values, dtype=np.float64))
    n = x.size
    vi = np.float64(n - 1) * (np.float64(q) / np.float64(100))
    lo = int(np.floor(vi))
    hi = min(lo + 1, n - 1)
    g = vi - np.float64(lo)
    a, b = x[lo], x[hi]
    diff = b - a
    return b - diff * (np.float64(1) - g) if g >= 0.5 else a + diff * g


def metrics(D, n_a, n_b, q=95.0, tolerances=(1.0,)):
    """dict of the metrics from the distance vector; the three means as exactly rounded sums (``math.fsum``), divided."""
    D = np.asarray(D, dtype=np.float64)
    d_ab, d_ba = D[:n_a], D[n_a:]
    assert d_ba.size == n_b
    return {
        "hd": float(D.max()),
        "hd_percentile": float(max(percentile(d_ab, q), percentile(d_ba, q))),
        "hd_percentile_pooled": float(percentile(D, q)),
        "asd_ab": math.fsum(d_ab) / n_a,
        "asd_ba": math.fsum(d_ba) / n_b,
        "assd": math.fsum(D) / (n_a + n_b),
        "nsd_counts": tuple(int((D <= t).sum()) for t in tolerances),
        "nsd": tuple(float(np.float64(int((D <= t).sum())) / np.float64(n_a + n_b)) for t in tolerances),
        "n_a": n_a, "n_b": n_b,
    }


def mean_bound(values):
    """The largest distance between ANY float64 summation order of the non-negative ``values`` and their exact sum, divided by
    their number: ``(n - 1) u sum / (1 - (n - 1) u) / n`` with ``u = 2^-53`` (Higham, Accuracy and Stability, section 4.2)."""
    n = len(values)
    gamma = (n - 1) * 2.0 ** -53
    return gamma * math.fsum(values) / (1.0 - gamma) / n
