"""The airway wall measurement in plain numpy: the definition of ``seunet_amd.airway_walls`` (include/seunet_hip.h, DESIGN.md section
3q) operation by operation; float64 where the definition says float64 and float32 where it says float32, every product, sum,
quotient and floor a single numpy operation (numpy fuses nothing).  The device equals ``mask``, ``codes``, ``edges`` and ``sums`` bit
for bit.  The direction table is an argument (``seunet_airway_wall_directions``, or scripts/gen_wall_table.py's), so that no cos or
sin shows in a result.

Vectorised over points, rays and samples; the points are worked in chunks so that a chunk's arrays stay small."""
import numpy as np

import cross_section_oracle as co

RAYS = 64
SAMPLES = 64
CHUNK = 128
FLOAT_COLUMNS = ("inner_radius", "outer_radius", "wall_thickness", "inner_area", "outer_area", "wall_area", "wall_area_percent",
                 "inner_perimeter", "peak")
BRANCH_COLUMNS = ("wall_thickness_mean", "wall_thickness_median", "wall_area_percent_mean", "wall_area_percent_median")


def n_search(ray_step, max_wall):
    """The smallest integer n with n * ray_step >= max_wall."""
    n = int(np.ceil(max_wall / ray_step))
    while n > 0 and (n - 1) * ray_step >= max_wall:
        n -= 1
    while n * ray_step < max_wall:
        n += 1
    return n


def table_of(sections):
    """int32[m, 12]: the rows of seunet_cross_section_emit from the dict of cross_section_oracle.cross_sections."""
    m = len(sections["label"])
    t = np.zeros((m, 12), np.int32)
    t[:, 0:3] = sections["coord"]
    t[:, 3] = sections["label"]
    t[:, 4] = sections["support"]
    t[:, 5] = sections["count"]
    t[:, 6:11] = sections["moments"]
    t[:, 11] = sections["rim"]
    return t


def take(a, k):
    return np.take_along_axis(a, np.clip(k, 0, SAMPLES - 1)[..., None], axis=-1)[..., 0]


def butterfly(x):
    """T_{l+1}[r] = T_l[r] + T_l[r ^ (1 << l)], l = 0 .. 5, along axis 1 (64 long): T_6[0]."""
    for _ in range(6):
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def rays(ct, parsing, table, tangent, directions, spacing, step, ray_step, n, min_contrast, same_label):
    """One chunk of measured points (count != 0, rim <= 0): dict of [point, ray] arrays."""
    ct, parsing = np.asarray(ct), np.asarray(parsing)
    s = np.asarray(spacing, dtype=np.float64)
    h, dr, c = np.float64(step), np.float64(ray_step), np.float32(min_contrast)
    d = np.asarray(directions, dtype=np.float64).reshape(RAYS, 2)
    K = np.arange(SAMPLES)
    u, v = co.basis(tangent)
    count = table[:, 5].astype(np.float64)
    cih = (table[:, 6].astype(np.float64) / count) * h
    cjh = (table[:, 7].astype(np.float64) / count) * h
    rho = K.astype(np.float64) * dr
    usable = np.ones((table.shape[0], RAYS, SAMPLES), bool)
    f, w, near = [], [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            o = (table[:, a].astype(np.float64) * s[a] + cih * u[:, a]) + cjh * v[:, a]
            e = d[None, :, 0] * u[:, a][:, None] + d[None, :, 1] * v[:, a][:, None]
            x = o[:, None, None] + rho[None, None, :] * e[:, :, None]
            g = x / s[a]
            fa = np.floor(g)
            usable &= (fa >= 0.0) & (fa <= float(ct.shape[a] - 2))
            f.append(fa)
            w.append((g - fa).astype(np.float32))
            near.append(np.floor(g + 0.5))
    L = np.where(usable.all(axis=-1), SAMPLES, np.argmin(usable, axis=-1))
    fi = [np.where(usable, fa, 0.0).astype(np.int64) for fa in f]
    one = usable.astype(np.int64)

    def corner(b0, b1, b2):
        return ct[fi[0] + b0 * one, fi[1] + b1 * one, fi[2] + b2 * one].astype(np.float32)

    def lerp(a, b, wa):
        return a + wa * (b - a)

    with np.errstate(over="ignore", invalid="ignore"):
        c00, c01 = lerp(corner(0, 0, 0), corner(0, 0, 1), w[2]), lerp(corner(0, 1, 0), corner(0, 1, 1), w[2])
        c10, c11 = lerp(corner(1, 0, 0), corner(1, 0, 1), w[2]), lerp(corner(1, 1, 0), corner(1, 1, 1), w[2])
        P = lerp(lerp(c00, c01, w[1]), lerp(c10, c11, w[1]), w[0])
    assert P.dtype == np.float32
    ni = [np.where(usable, na, 0.0).astype(np.int64) for na in near]
    got = parsing[ni[0], ni[1], ni[2]]
    nonzero = usable & (got != 0)
    inside = usable & ((got == table[:, 3][:, None, None]) if same_label else (got != 0))

    Lk = L[..., None]
    outside = ~inside & (K < Lk) & (K >= 1)
    bounded = (L > 0) & inside[..., 0] & outside.any(axis=-1)
    kb = np.argmax(outside, axis=-1)
    lo, hi = np.maximum(kb - 1, 0), np.minimum(kb + n, L - 1)
    window = (K >= lo[..., None]) & (K <= hi[..., None])
    Pw = np.where(window, P, -np.inf)
    kp = np.argmax(Pw, axis=-1)                               # the first of the maxima
    Pp = take(P, kp)
    tie = (Pw == Pp[..., None]).sum(axis=-1) > 1
    fail2 = (kp + 1 >= L) | ((kp == hi) & (take(P, kp + 1) >= Pp))
    Pl = np.where(K <= kp[..., None], P, np.inf).min(axis=-1).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        fail3 = (Pp - Pl) < c
    stop = np.minimum(kp + n, L - 1)
    falls = np.zeros(P.shape, bool)
    falls[..., :-1] = P[..., 1:] <= P[..., :-1]
    stays = (K >= kp[..., None]) & ~((K < stop[..., None]) & falls)
    ko = np.argmax(stays, axis=-1)
    Po = take(P, ko)
    fail4 = (nonzero & (K >= kb[..., None]) & (K <= ko[..., None])).any(axis=-1)
    with np.errstate(invalid="ignore", over="ignore"):
        fail5 = (Pp - Po) < c
    code = np.select([~bounded, fail2, fail3, fail4, fail5], [1, 2, 3, 4, 5], 0).astype(np.uint8)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Hin = np.float32(0.5) * (Pl + Pp)
        cand = (K < kp[..., None]) & (P <= Hin[..., None])
        ki = SAMPLES - 1 - np.argmax(cand[..., ::-1], axis=-1)
        a = take(P, ki).astype(np.float64)
        rin = (ki.astype(np.float64) + (Hin.astype(np.float64) - a) / (take(P, ki + 1).astype(np.float64) - a)) * dr
        Hout = np.float32(0.5) * (Pp + Po)
        below = np.zeros(P.shape, bool)
        below[..., :-1] = P[..., 1:] <= Hout[..., None]
        ke = np.argmax((K >= kp[..., None]) & (K <= ko[..., None] - 1) & below, axis=-1)
        a = take(P, ke).astype(np.float64)
        rout = (ke.astype(np.float64) + (a - Hout.astype(np.float64)) / (a - take(P, ke + 1).astype(np.float64))) * dr
    ok = code == 0
    return {"code": code, "rho_in": np.where(ok, rin, 0.0), "rho_out": np.where(ok, rout, 0.0),
            "peak": np.where(ok, Pp.astype(np.float64), 0.0), "L": L, "kb": np.where(bounded, kb, -1), "kp": np.where(code != 1, kp, -1),
            "hi": hi, "tie": tie & (code != 1)}


def airway_walls(ct, parsing, sections, directions, spacing=(1.0, 1.0, 1.0), ray_step=None, max_wall=None, min_contrast=100.0,
                 same_label=True):
    """``sections``: the dict of cross_section_oracle.cross_sections for the same volume, spacing and ``same_label``.  ->
    ``mask`` uint64[m], ``sums`` float64[m, 6], ``codes`` uint8[m, 64], ``edges`` float64[m, 64, 2], and for the tests that ask what
    a case reaches ``L``, ``kb``, ``kp``, ``hi`` int64[m, 64] (-1: none) and ``tie`` bool[m, 64]."""
    s = np.asarray(spacing, dtype=np.float64).reshape(3)
    step = float(sections["step"])
    dr = step if ray_step is None else float(ray_step)
    reach = 5.0 * float(s.min()) if max_wall is None else float(max_wall)
    n = n_search(dr, reach)
    assert 1 <= n <= 31, n
    table, tangent = table_of(sections), np.asarray(sections["tangent"], dtype=np.float64)
    m = table.shape[0]
    out = {"codes": np.full((m, RAYS), 6, np.uint8), "edges": np.zeros((m, RAYS, 2), np.float64), "peaks": np.zeros((m, RAYS), np.float64),
           "L": np.full((m, RAYS), -1, np.int64), "kb": np.full((m, RAYS), -1, np.int64), "kp": np.full((m, RAYS), -1, np.int64),
           "hi": np.full((m, RAYS), -1, np.int64), "tie": np.zeros((m, RAYS), bool)}
    idx = np.flatnonzero((table[:, 5] != 0) & (table[:, 11] <= 0))
    for at in range(0, idx.size, CHUNK):
        part = idx[at:at + CHUNK]
        r = rays(ct, parsing, table[part], tangent[part], directions, s, step, dr, n, min_contrast, same_label)
        out["codes"][part] = r["code"]
        out["edges"][part, :, 0], out["edges"][part, :, 1], out["peaks"][part] = r["rho_in"], r["rho_out"], r["peak"]
        for k in ("L", "kb", "kp", "hi", "tie"):
            out[k][part] = r[k]
    rin, rout = out["edges"][:, :, 0], out["edges"][:, :, 1]
    out["sums"] = np.stack([butterfly(x) for x in (rin, rout, rin * rin, rout * rout, rout - rin, out["peaks"])], axis=1).reshape(m, 6)
    bits = (out["codes"] == 0).astype(np.uint64) << np.arange(RAYS, dtype=np.uint64)[None, :]
    out["mask"] = np.bitwise_or.reduce(bits, axis=1).astype(np.uint64).reshape(m)
    out.update(label=np.asarray(sections["label"], np.int32), ray_step=dr, n_search=n, step=step)
    return out


def derived(mask, sums, min_rays=32):
    """The host float64 columns from the device's mask and sums; nan where fewer than ``min_rays`` rays are measured."""
    n = np.array([bin(int(v)).count("1") for v in np.asarray(mask).reshape(-1)], dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 6)
    valid = n >= min_rays
    with np.errstate(divide="ignore", invalid="ignore"):
        c = n.astype(np.float64)
        cols = {"inner_radius": sums[:, 0] / c, "outer_radius": sums[:, 1] / c, "wall_thickness": sums[:, 4] / c,
                "inner_area": np.pi * sums[:, 2] / c, "outer_area": np.pi * sums[:, 3] / c, "peak": sums[:, 5] / c}
        cols["wall_area"] = cols["outer_area"] - cols["inner_area"]
        cols["wall_area_percent"] = 100.0 * cols["wall_area"] / cols["outer_area"]
        cols["inner_perimeter"] = 2.0 * np.pi * cols["inner_radius"]
    cols = {k: np.where(valid, v, np.nan) for k, v in cols.items()}
    cols.update(rays_valid=n, valid=valid)
    return cols


def per_branch(label, cols, num):
    """wall_count int64[num] and the BRANCH_COLUMNS float64[num] over the valid rows of each label 1 .. num (nan: none)."""
    out = {"wall_sections": np.zeros(num, np.int64)}
    for k in BRANCH_COLUMNS + ("wall_area_median", "inner_perimeter_median"):
        out[k] = np.full(num, np.nan)
    for lab in range(1, num + 1):
        rows = cols["valid"] & (np.asarray(label) == lab)
        n = int(rows.sum())
        out["wall_sections"][lab - 1] = n
        if n == 0:
            continue
        out["wall_thickness_mean"][lab - 1] = cols["wall_thickness"][rows].mean()
        out["wall_thickness_median"][lab - 1] = np.median(cols["wall_thickness"][rows])
        out["wall_area_percent_mean"][lab - 1] = cols["wall_area_percent"][rows].mean()
        out["wall_area_percent_median"][lab - 1] = np.median(cols["wall_area_percent"][rows])
        out["wall_area_median"][lab - 1] = np.median(cols["wall_area"][rows])
        out["inner_perimeter_median"][lab - 1] = np.median(cols["inner_perimeter"][rows])
    return out
