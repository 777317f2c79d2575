"""The airway cross-sections in plain numpy: the definition of ``seunet_amd.cross_sections`` operation by
operation, float64, every product, sum, quotient and root a single numpy operation (numpy fuses nothing; no dot product, matmul or
einsum is used, which a BLAS might evaluate with fused multiply-adds).  The device equals every column bit for bit.

Points are the labelled skeleton voxels (``skeleton != 0``, ``1 <= parsing <= num``) in raster order.  Vectorised over points; the
sample planes are worked in chunks of points so that a chunk's arrays stay small."""
import numpy as np

HALF = 31                                                    # the sample plane is 63 x 63: columns i and rows j in -31 .. 31
SIDE = 2 * HALF + 1
POWER_STEPS = 6
CHUNK = 256
INT_COLUMNS = ("coord", "label", "support", "count", "moments", "rim")
FLOAT_COLUMNS = ("area", "diameter_major", "diameter_minor")
BRANCH_COLUMNS = ("area_mean", "area_min", "area_max", "area_median", "diameter_major_mean", "diameter_minor_mean")


def points(parsing, skeleton, num):
    """(coord int32[m, 3], label int32[m]) of the labelled skeleton voxels in raster order; status 1: a label outside 0 .. num."""
    parsing = np.asarray(parsing)
    status = int(((parsing < 0) | (parsing > num)).any())
    mask = (np.asarray(skeleton) != 0) & (parsing >= 1) & (parsing <= num)
    coord = np.argwhere(mask).astype(np.int32).reshape(-1, 3)
    return coord, parsing[mask].astype(np.int32), status


def _max_abs(a):
    return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


def tangents(parsing, skeleton, coord, label, spacing, window):
    """(support int32[m], tangent float64[m, 3], valid bool[m]): step 1 of the definition."""
    m = coord.shape[0]
    s = np.asarray(spacing, dtype=np.float64)
    W = int(window)
    marked = np.where(np.asarray(skeleton) != 0, np.asarray(parsing), 0).astype(np.int64)
    padded = np.pad(marked, W, constant_values=0)
    n = np.zeros(m, np.int64)
    sd = np.zeros((m, 3), np.int64)
    sdd = np.zeros((m, 3, 3), np.int64)
    c = coord.astype(np.int64) + W
    lab = label.astype(np.int64)
    for d0 in range(-W, W + 1):
        for d1 in range(-W, W + 1):
            for d2 in range(-W, W + 1):
                hit = (padded[c[:, 0] + d0, c[:, 1] + d1, c[:, 2] + d2] == lab).astype(np.int64)
                d = (d0, d1, d2)
                n += hit
                for a in range(3):
                    sd[:, a] += hit * d[a]
                    for b in range(a, 3):
                        sdd[:, a, b] += hit * (d[a] * d[b])
    A = np.zeros((m, 3, 3), np.float64)
    for a in range(3):
        for b in range(a, 3):
            scatter = n * sdd[:, a, b] - sd[:, a] * sd[:, b]
            A[:, a, b] = (scatter.astype(np.float64) * s[a]) * s[b]
            A[:, b, a] = A[:, a, b]
    tangent = np.zeros((m, 3), np.float64)
    valid = n >= 3
    if m:
        valid &= _max_abs(A) > 0.0
    idx = np.flatnonzero(valid)
    if idx.size:
        A = A[idx]
        A = A / _max_abs(A)[:, None, None]
        for _ in range(POWER_STEPS):
            B = np.empty_like(A)
            for a in range(3):
                for b in range(3):
                    B[:, a, b] = (A[:, a, 0] * A[:, 0, b] + A[:, a, 1] * A[:, 1, b]) + A[:, a, 2] * A[:, 2, b]
            A = B / _max_abs(B)[:, None, None]
        len2 = (A[:, 0, :] * A[:, 0, :] + A[:, 1, :] * A[:, 1, :]) + A[:, 2, :] * A[:, 2, :]      # [point, column]
        col = np.argmax(len2, axis=1)                        # the first of the maxima
        rows = np.arange(idx.size)
        t = A[rows, :, col] / np.sqrt(len2[rows, col])[:, None]
        lead = t[rows, np.argmax(np.abs(t), axis=1)]
        t = np.where((lead < 0.0)[:, None], -t, t)
        tangent[idx] = t
    return n.astype(np.int32), tangent, valid


def basis(t):
    """(u, v) float64[m, 3] of valid unit tangents t: step 2."""
    m = t.shape[0]
    rows = np.arange(m)
    a = np.argmin(np.abs(t), axis=1)                         # the first of the minima
    e = np.zeros((m, 3), np.float64)
    e[rows, a] = 1.0
    w = e - t[rows, a][:, None] * t
    u = w / np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])[:, None]
    v = np.stack([t[:, 1] * u[:, 2] - t[:, 2] * u[:, 1], t[:, 2] * u[:, 0] - t[:, 0] * u[:, 2], t[:, 0] * u[:, 1] - t[:, 1] * u[:, 0]],
                 axis=1)
    return u, v


def inside_planes(parsing, coord, label, u, v, spacing, step, same_label=True):
    """bool[m, 63, 63] indexed [point, row j + 31, column i + 31]: step 3."""
    parsing = np.asarray(parsing)
    s = np.asarray(spacing, dtype=np.float64)
    h = np.float64(step)
    k = np.arange(-HALF, HALF + 1).astype(np.float64)
    ih = (k * h)[None, None, :]                              # columns
    jh = (k * h)[None, :, None]                              # rows
    ok = np.ones((coord.shape[0], SIDE, SIDE), bool)
    vox = []
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            centre = (coord[:, a].astype(np.float64) * s[a])[:, None, None]
            x = (centre + ih * u[:, a][:, None, None]) + jh * v[:, a][:, None, None]
            f = np.floor(x / s[a] + 0.5)
            ok &= (f >= 0.0) & (f < float(parsing.shape[a]))
            vox.append(np.where(ok, f, 0.0).astype(np.int64))
    got = parsing[vox[0], vox[1], vox[2]]
    return ok & ((got == label[:, None, None]) if same_label else (got != 0))


def flood(inside):
    """The 4-connected part of each plane that contains the centre: step 4."""
    f = np.zeros_like(inside)
    f[:, HALF, HALF] = inside[:, HALF, HALF]
    while True:
        grown = f.copy()
        grown[:, 1:, :] |= f[:, :-1, :]
        grown[:, :-1, :] |= f[:, 1:, :]
        grown[:, :, 1:] |= f[:, :, :-1]
        grown[:, :, :-1] |= f[:, :, 1:]
        grown &= inside
        grown |= f
        if np.array_equal(grown, f):
            return f
        f = grown


def measure(f):
    """(count int32[m], moments int32[m, 5], rim int32[m]) of the planes f."""
    k = np.arange(-HALF, HALF + 1).astype(np.int64)
    i = k[None, None, :]
    j = k[None, :, None]
    g = f.astype(np.int64)
    count = g.sum(axis=(1, 2))
    moments = np.stack([(g * i).sum(axis=(1, 2)), (g * j).sum(axis=(1, 2)), (g * i * i).sum(axis=(1, 2)), (g * j * j).sum(axis=(1, 2)),
                        (g * i * j).sum(axis=(1, 2))], axis=1)
    edge = (np.abs(i) == HALF) | (np.abs(j) == HALF)
    rim = (g * edge).sum(axis=(1, 2))
    return count.astype(np.int32), moments.astype(np.int32), rim.astype(np.int32)


def cross_sections(parsing, skeleton, spacing=(1.0, 1.0, 1.0), step=None, window=4, same_label=True, num=None):
    """The integer columns and the tangents as a dict, plus ``status`` (1: a label outside 0 .. num) and ``step``."""
    parsing = np.asarray(parsing)
    s = np.asarray(spacing, dtype=np.float64).reshape(3)
    h = float(s.min() / 2.0) if step is None else float(step)
    if num is None:
        num = max(int(parsing.max()), 0) if parsing.size else 0
    coord, label, status = points(parsing, skeleton, num)
    m = coord.shape[0]
    support, tangent, valid = tangents(parsing, skeleton, coord, label, s, window)
    count = np.zeros(m, np.int32)
    moments = np.zeros((m, 5), np.int32)
    rim = np.zeros(m, np.int32)
    idx = np.flatnonzero(valid)
    for at in range(0, idx.size, CHUNK):
        part = idx[at:at + CHUNK]
        u, v = basis(tangent[part])
        f = flood(inside_planes(parsing, coord[part], label[part], u, v, s, h, same_label))
        count[part], moments[part], rim[part] = measure(f)
    return {"coord": coord, "label": label, "support": support, "tangent": tangent, "count": count, "moments": moments, "rim": rim,
            "status": status, "step": h}


def derived(count, moments, rim, step):
    """The host float64 columns from the integer ones: area, diameter_major, diameter_minor, valid."""
    h = float(step)
    c = np.asarray(count).astype(np.float64)
    mo = np.asarray(moments).astype(np.float64).reshape(-1, 5)
    with np.errstate(divide="ignore", invalid="ignore"):
        mi, mj = mo[:, 0] / c, mo[:, 1] / c
        a = mo[:, 2] / c - mi * mi + 1.0 / 12.0              # each sample stands for an h x h square
        b = mo[:, 3] / c - mj * mj + 1.0 / 12.0
        g = mo[:, 4] / c - mi * mj
        mid = 0.5 * (a + b)
        rad = np.sqrt(0.25 * (a - b) * (a - b) + g * g)
        major = 4.0 * h * np.sqrt(mid + rad)
        minor = 4.0 * h * np.sqrt(np.maximum(mid - rad, 0.0))
    empty = np.asarray(count) <= 0
    return {"area": c * (h * h), "diameter_major": np.where(empty, np.nan, major), "diameter_minor": np.where(empty, np.nan, minor),
            "valid": (np.asarray(count) > 0) & (np.asarray(rim) == 0)}


def per_branch(label, cols, num):
    """section_count int64[num] and the BRANCH_COLUMNS float64[num] over the valid rows of each label 1 .. num (nan: none)."""
    out = {"section_count": np.zeros(num, np.int64)}
    for k in BRANCH_COLUMNS:
        out[k] = np.full(num, np.nan)
    for lab in range(1, num + 1):
        rows = cols["valid"] & (np.asarray(label) == lab)
        n = int(rows.sum())
        out["section_count"][lab - 1] = n
        if n == 0:
            continue
        area = cols["area"][rows]
        out["area_mean"][lab - 1] = area.mean()
        out["area_min"][lab - 1] = area.min()
        out["area_max"][lab - 1] = area.max()
        out["area_median"][lab - 1] = np.median(area)
        out["diameter_major_mean"][lab - 1] = cols["diameter_major"][rows].mean()
        out["diameter_minor_mean"][lab - 1] = cols["diameter_minor"][rows].mean()
    return out
