"""A plain numpy / scipy statement of what ``seunet_amd.components`` computes: the oracle of
tests/test_betti_host.py and tests/test_betti_*gpu.py.  Nothing here comes from the code under test except ``mean_abs_error``,
the one numpy expression the issue asks both sides to share.

* labels: ``scipy.ndimage.label`` with ``generate_binary_structure(3, connectivity)``;
* table: ``bincount`` / ``minimum.at`` / ``maximum.at`` over the labelled voxels;
* Euler number: the eight cell counts with shifted slices of the zero-padded mask -- OR over the voxels that share a lattice cell
  (connectivity 3, closed cubes) or AND over the voxels of a pair / square / cube (connectivity 1, voxels as vertices);
* b0 and b2: ``ndimage.label`` of the mask, and of the complement of the mask padded with one layer of background, minus one;
* tiles: a Python loop over crops."""
import functools

import numpy as np
from scipy import ndimage


def structure(connectivity):
    return ndimage.generate_binary_structure(3, connectivity)


def label(mask, connectivity=3):
    lab, num = ndimage.label(np.asarray(mask) != 0, structure(connectivity))
    return lab.astype(np.int32), int(num)


def table(lab, num):
    """(size int64 [N], first int64 [N], box int32 [N, 6] = min0, max0, min1, max1, min2, max2)."""
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    k = flat[idx].astype(np.int64) - 1
    size = np.bincount(flat, minlength=num + 1)[1:].astype(np.int64)
    first = np.full(num, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, k, idx.astype(np.int64))
    box = np.empty((num, 6), dtype=np.int32)
    for axis, coord in enumerate(np.unravel_index(idx, lab.shape)):
        lo = np.full(num, np.iinfo(np.int32).max, dtype=np.int32)
        hi = np.full(num, -1, dtype=np.int32)
        np.minimum.at(lo, k, coord.astype(np.int32))
        np.maximum.at(hi, k, coord.astype(np.int32))
        box[:, 2 * axis], box[:, 2 * axis + 1] = lo, hi
    return size, first, box


def remove_small_objects(mask, min_size, connectivity=3):
    lab, num = label(mask, connectivity)
    size = np.bincount(lab.ravel(), minlength=num + 1)
    keep = size >= min_size
    keep[0] = False
    return keep[lab].astype(np.uint8)


def cell_counts(mask, connectivity):
    """int64 [4]: the cell counts by the number of axes a cell spans two voxels along (0 .. 3)."""
    m = np.asarray(mask) != 0
    p = np.pad(m, 1)
    n = m.shape
    counts = np.zeros(4, dtype=np.int64)
    for S in range(8):
        axes = [(S >> k) & 1 for k in range(3)]
        acc = None
        for offs in np.ndindex(*[a + 1 for a in axes]):
            # axis k in S: positions 0 .. n_k, voxel (position - 1 + 1 - off) of the padded array; else the voxels themselves
            sl = tuple(slice(1 - o, 1 - o + n[k] + 1) if axes[k] else slice(1, n[k] + 1) for k, o in enumerate(offs))
            v = p[sl]
            acc = v if acc is None else ((acc & v) if connectivity == 1 else (acc | v))
        counts[sum(axes)] += int(np.count_nonzero(acc))
    return counts


def euler_number(mask, connectivity=3):
    c = cell_counts(mask, connectivity)
    if connectivity == 3:          # cubes, faces, edges, vertices: V - E + F - C
        return int(c[3] - c[2] + c[1] - c[0])
    if connectivity == 1:          # voxels, pairs, squares, cubes: V' - E' + F' - C'
        return int(c[0] - c[1] + c[2] - c[3])
    raise ValueError(connectivity)


def betti_numbers(mask, connectivity=3):
    if connectivity not in (1, 3):
        raise ValueError(connectivity)
    m = np.asarray(mask) != 0
    b0 = label(m, connectivity)[1]
    b2 = label(~np.pad(m, 1), 4 - connectivity)[1] - 1
    return b0, b0 + b2 - euler_number(m, connectivity), b2


def tile_slices(shape, patch):
    """The crops of the tiles in raster tile order, and the tiles per axis."""
    p = tuple(min(int(v), int(n)) for v, n in zip(patch, shape))
    tiles = tuple(-(-n // q) for n, q in zip(shape, p))
    out = []
    for a in range(tiles[0]):
        for b in range(tiles[1]):
            for c in range(tiles[2]):
                out.append((slice(a * p[0], (a + 1) * p[0]), slice(b * p[1], (b + 1) * p[1]), slice(c * p[2], (c + 1) * p[2])))
    return out, tiles


def betti_tiles(mask, patch, connectivity=3):
    """int32 [T, 3] and the tiles per axis."""
    m = np.asarray(mask) != 0
    slices, tiles = tile_slices(m.shape, patch if patch is not None else m.shape)
    return np.array([betti_numbers(m[s], connectivity) for s in slices], dtype=np.int32).reshape(-1, 3), tiles


def euler_tiles(mask, patch, connectivity=3):
    m = np.asarray(mask) != 0
    slices, _ = tile_slices(m.shape, patch)
    return np.array([euler_number(m[s], connectivity) for s in slices], dtype=np.int64)


def betti_error(pred, lab, patch=None, connectivity=3):
    """(tiles, pred table, label table, error float64 [3], total)."""
    from seunet_amd.components import mean_abs_error      # the shared numpy expression
    tp, tiles = betti_tiles(pred, patch, connectivity)
    tl, _ = betti_tiles(lab, patch, connectivity)
    err = mean_abs_error(tp, tl)
    return tiles, tp, tl, err, float(err.sum())


# ---- volumes the tests share ------------------------------------------------------------------------------------------------------
def noise(shape, density, seed):
    return (np.random.RandomState(seed).random_sample(shape) < density).astype(np.uint8)


def _grid(shape, centre):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) - c for n, c in zip(shape, centre)], indexing="ij")


def ball(shape, centre, r):
    x, y, z = _grid(shape, centre)
    return (x * x + y * y + z * z <= r * r).astype(np.uint8)


def shell(shape, centre, r_out, r_in):
    x, y, z = _grid(shape, centre)
    d2 = x * x + y * y + z * z
    return ((d2 <= r_out * r_out) & (d2 > r_in * r_in)).astype(np.uint8)


def torus(shape, centre, R, r):
    """A solid torus around axis 0."""
    x, y, z = _grid(shape, centre)
    return ((np.sqrt(y * y + z * z) - R) ** 2 + x * x <= r * r).astype(np.uint8)


KNOWN = {"ball": (1, 0, 0), "torus": (1, 1, 0), "shell": (1, 0, 1), "two_tori": (2, 2, 0), "shell_with_ball": (2, 0, 1),
         "empty": (0, 0, 0), "full": (1, 0, 0)}


@functools.lru_cache(maxsize=None)
def known(name, n=25):
    s, c = (n, n, n), (n // 2,) * 3
    if name == "ball":
        v = ball(s, c, 8)
    elif name == "torus":
        v = torus(s, c, 7, 2.5)
    elif name == "shell":
        v = shell(s, c, 9, 6)
    elif name == "two_tori":
        v = torus(s, (5, n // 2, n // 2), 7, 2.5) | torus(s, (18, n // 2, n // 2), 7, 2.5)
    elif name == "shell_with_ball":
        v = shell(s, c, 10, 7) | ball(s, c, 3)
    elif name == "empty":
        v = np.zeros(s, dtype=np.uint8)
    elif name == "full":
        v = np.ones(s, dtype=np.uint8)
    else:
        raise KeyError(name)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def serpentine(shape=(8, 16, 200)):
    """A one-voxel path: along axis 2 in every second row of every second plane, joined at alternating ends."""
    v = np.zeros(shape, dtype=np.uint8)
    at_end = False                                   # which end of axis 2 the path is at
    for x in range(0, shape[0], 2):
        ys = list(range(0, shape[1], 2))
        if (x // 2) % 2:
            ys.reverse()
        for k, y in enumerate(ys):
            v[x, y, :] = 1
            at_end = not at_end
            z = shape[2] - 1 if at_end else 0
            if k + 1 < len(ys):
                v[x, (y + ys[k + 1]) // 2, z] = 1
            elif x + 2 < shape[0]:
                v[x + 1, y, z] = 1
    v.setflags(write=False)
    return v


TILE_SHAPE = (40, 50, 150)
TILE_PATCHES = [(16, 16, 24), (32, 32, 32), (8, 8, 64), (7, 5, 13)]


@functools.lru_cache(maxsize=None)
def tile_volume(which):
    """The (40, 50, 150) volumes of the tile tests: noise at two densities, and a torus and a shell across tile corners."""
    if which == "sparse":
        v = noise(TILE_SHAPE, 0.08, 31)
    elif which == "dense":
        v = noise(TILE_SHAPE, 0.45, 32)
    elif which == "shapes":
        v = torus(TILE_SHAPE, (16, 16, 48), 9, 3) | shell(TILE_SHAPE, (32, 32, 96), 7, 4)
    else:
        raise KeyError(which)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def tile_tables(which, patch, connectivity):
    t, tiles = betti_tiles(tile_volume(which), patch, connectivity)
    t.setflags(write=False)
    return t, tiles
