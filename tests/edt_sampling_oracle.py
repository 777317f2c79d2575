"""The Euclidean distance transform with voxel spacing as scipy computes it, stated in plain Python: the
oracle csrc/edt_sampling.hip and ``seunet_amd.distance_transform_edt(..., sampling=...)`` are tested against.

``scipy.ndimage.distance_transform_edt(input, sampling=s, return_indices=True)`` runs a separable feature transform in float64
and computes the distances from the indices in numpy.  Python floats are IEEE doubles and every product and sum below is a
rounded operation of its own, in the order of the contract, so the results are scipy's bit for bit -- which
tests/test_edt_sampling_host.py checks against tests/golden/edt_sampling_known.npz (recorded from scipy) and, where it is
installed, against scipy itself.  Nothing here imports scipy.

Pure Python loops: meant for volumes of a few thousand voxels (a 3 x 130 x 70 volume takes about a second)."""
import itertools

import numpy as np


def _line(F, d, coor, s):
    """One line along axis ``d``.  ``F``: the features [f0, f1, f2] of the line's positions in order ([-1, -1, -1]: none);
    ``coor``: the line's coordinates (entry ``d`` is not used).  Returns the features after the pass."""
    others = [jj for jj in range(3) if jj != d]

    def off_line(site):                                       # uR / vR / wR of the contract
        r = 0.0
        for jj in others:
            tw = float(F[site][jj] - coor[jj]) * s[jj]
            r = r + tw * tw
        return r

    g = []                                                    # the stack: positions of sites
    for ii in range(len(F)):
        if F[ii][0] < 0:
            continue
        fd = float(F[ii][d])
        wR = off_line(ii)
        while len(g) >= 2:
            idx1, idx2 = g[-1], g[-2]
            a = (float(F[idx1][d]) - float(F[idx2][d])) * s[d]
            b = (fd - float(F[idx1][d])) * s[d]
            c = a + b
            uR, vR = off_line(idx2), off_line(idx1)
            if c * vR - b * uR - a * wR - a * b * c <= 0.0:   # left to right, a * b * c = (a * b) * c
                break
            g.pop()
        g.append(ii)
    if not g:
        return [list(f) for f in F]

    def delta(k, ii):
        r = 0.0
        for jj in range(3):
            t = float(F[g[k]][jj] - (ii if jj == d else coor[jj])) * s[jj]
            r = r + t * t
        return r

    out = []
    l = 0
    for ii in range(len(F)):
        d1 = delta(l, ii)
        while l < len(g) - 1:
            d2 = delta(l + 1, ii)
            if d1 <= d2:                                      # a tie keeps the earlier site
                break
            l += 1
            d1 = d2
        out.append(list(F[g[l]]))
    return out


def feature_transform(volume, sampling):
    """int32 (3, n0, n1, n2): for every voxel the coordinates of the nearest voxel with ``volume == 0`` under ``sampling``
    (three floats), ties as scipy resolves them; -1 everywhere when there is no such voxel."""
    vol = np.asarray(volume)
    assert vol.ndim == 3
    s = [float(v) for v in sampling]
    assert len(s) == 3
    shape = vol.shape
    f = np.full((3,) + shape, -1, dtype=np.int64)
    zero = vol == 0
    for a, idx in enumerate(np.indices(shape)):
        f[a][zero] = idx[zero]
    for d in range(3):
        others = [jj for jj in range(3) if jj != d]
        for fixed in itertools.product(*(range(shape[jj]) for jj in others)):
            coor = [0, 0, 0]
            sel = [slice(None)] * 4
            sel[1 + d] = slice(None)
            for jj, v in zip(others, fixed):
                coor[jj] = v
                sel[1 + jj] = v
            sel = tuple(sel)
            F = f[sel].T.tolist()                             # (len, 3)
            f[sel] = np.asarray(_line(F, d, coor, s), dtype=np.int64).reshape(len(F), 3).T
    return f.astype(np.int32)


def distances(indices, sampling):
    """float64 (n0, n1, n2) from the indices, as numpy computes them in scipy: dt_j = float64(index_j - coordinate_j) * s_j and
    dist = sqrt((dt_0^2 + dt_1^2) + dt_2^2)."""
    indices = np.asarray(indices)
    s = np.asarray(sampling, dtype=np.float64).reshape(3)
    dt = (indices.astype(np.int64) - np.indices(indices.shape[1:])).astype(np.float64)
    for j in range(3):
        dt[j] = dt[j] * s[j]
    dt = dt * dt
    return np.sqrt((dt[0] + dt[1]) + dt[2])


def edt(volume, sampling):
    """-> (dist float64, indices int32), scipy's ``distance_transform_edt(volume, sampling=sampling, return_indices=True)``."""
    ind = feature_transform(volume, sampling)
    return distances(ind, sampling), ind


def squared_distance_to_all_sites(volume, sampling):
    """float64 (n0, n1, n2): the minimum over all zero voxels of the contract's squared distance, by brute force (vectorised);
    the bound the long-line GPU tests hold the kernel's choice against."""
    vol = np.asarray(volume)
    s = np.asarray(sampling, dtype=np.float64).reshape(3)
    sites = np.argwhere(vol == 0)
    grid = np.indices(vol.shape).reshape(3, -1).T              # (n, 3)
    best = np.full(grid.shape[0], np.inf)
    for k in range(0, sites.shape[0], 64):
        dt = (sites[k:k + 64, None, :] - grid[None, :, :]).astype(np.float64) * s
        dt = dt * dt
        best = np.minimum(best, ((dt[..., 0] + dt[..., 1]) + dt[..., 2]).min(axis=0))
    return best.reshape(vol.shape)
