"""Synthetic inputs of the airway-wall tests (tests/test_airway_wall_host.py checks the oracle on them against known answers,
tests/test_airway_wall_gpu.py the device against the oracle): ``case(name)`` is a dict with ``ct`` int16, ``parsing`` int32,
``skeleton`` uint8, ``spacing``, ``same_label`` and ``kw``, the keywords of ``airway_walls``.  Built once per name and shared
read-only, like the oracle's sections (``sections(name)``) and results (``want(name)``).

The phantoms are partial-volume tubes: lumen / wall / parenchyma at -1000 / 50 / -850 HU, every voxel the mean of 4 x 4 x 4
sub-voxel samples, lumen radius R = 4.0 and wall thickness T = 2.0 in the units of the spacing (1.25, 0.7, 0.7)."""
import ctypes as C

import numpy as np

import airway_wall_oracle as wo
import cross_section_cases as cc
import cross_section_oracle as co

ANISO = cc.ANISO
LUMEN, WALL, PARENCHYMA = -1000.0, 50.0, -850.0
R, T = 4.0, 2.0
SUB = 4
LENGTH = 12.0                                                # of a tube, in the units of the spacing
MARGIN = 4.5                                                 # parenchyma around the outer wall: past max_wall = 3.5
OBLIQUE = (3.0, 2.0, 1.0)
_CACHE, _SECTIONS, _WANT = {}, {}, {}
_DIRECTIONS = []


def directions():
    """float64[64, 2]: the committed table, from the library (host only: no GPU is needed)."""
    if not _DIRECTIONS:
        import seunet_amd
        out = (C.c_double * 128)()
        assert seunet_amd._lib.load().seunet_airway_wall_directions(out) == 0
        _DIRECTIONS.append(cc.frozen(np.array(out, dtype=np.float64).reshape(64, 2))[0])
    return _DIRECTIONS[0]


def axis_distance(x, centre, direction):
    """Distance of the points x[..., 3] from the line through ``centre`` along ``direction``."""
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.sqrt((d * d).sum())
    rel = x - np.asarray(centre, dtype=np.float64)
    along = (rel * d).sum(axis=-1)
    off = rel - along[..., None] * d
    return np.sqrt((off * off).sum(axis=-1))


def physical(shape, spacing, offset=(0.0, 0.0, 0.0)):
    """x[..., 3]: the physical position of every voxel centre, moved by ``offset`` voxels."""
    g = np.meshgrid(*[(np.arange(n) + o) * s for n, o, s in zip(shape, offset, spacing)], indexing="ij")
    return np.stack(g, axis=-1)


def paint(shape, spacing, value):
    """int16 volume: the mean of ``value(x)`` over SUB^3 samples per voxel."""
    offs = (np.arange(SUB) + 0.5) / SUB - 0.5
    acc = np.zeros(shape, np.float64)
    for o0 in offs:
        for o1 in offs:
            for o2 in offs:
                acc += value(physical(shape, spacing, (o0, o1, o2)))
    return np.rint(acc / SUB ** 3).astype(np.int16)


def line_skeleton(shape, spacing, centre, direction, length):
    """The voxels nearest to points every quarter of the smallest spacing along the axis, away from the ends of the volume."""
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.sqrt((d * d).sum())
    t = np.arange(-length / 2.0, length / 2.0, min(spacing) / 4.0)
    pts = np.floor((np.asarray(centre)[None, :] + t[:, None] * d[None, :]) / np.asarray(spacing)[None, :] + 0.5).astype(np.int64)
    keep = np.all((pts >= 0) & (pts < np.asarray(shape)[None, :]), axis=1)
    skeleton = np.zeros(shape, np.uint8)
    skeleton[tuple(pts[keep].T)] = 1
    return skeleton


def tube(direction, wall=T, blob=False, flat=False, cut=None, spacing=ANISO):
    """A tube through the middle of the volume along ``direction``.  ``blob``: a sphere of wall density against the outer wall
    on one side (an abutting vessel).  ``flat``: the CT is constant.  ``cut``: the volume ends this far past the axis on the high
    side of axis 2."""
    d = np.abs(np.asarray(direction, dtype=np.float64))
    d = d / np.sqrt((d * d).sum())
    reach = R + wall + MARGIN
    half = [int(np.ceil((LENGTH / 2.0 * da + reach * np.sqrt(max(1.0 - da * da, 0.0))) / s)) + 1 for da, s in zip(d, spacing)]
    shape = [2 * h + 1 for h in half]
    centre = [h * s for h, s in zip(half, spacing)]
    if cut is not None:
        shape[2] = half[2] + int(np.ceil(cut / spacing[2])) + 1
    shape = tuple(shape)
    other = np.cross(d, (1.0, 0.0, 0.0) if d[0] < 0.9 else (0.0, 1.0, 0.0))
    other = other / np.sqrt((other * other).sum())
    blob_at = np.asarray(centre) + (R + wall + 1.5) * other

    def value(x):
        r = axis_distance(x, centre, direction)
        v = np.where(r < R, LUMEN, np.where(r < R + wall, WALL, PARENCHYMA))
        if blob:
            rel = x - blob_at
            v = np.where((rel * rel).sum(axis=-1) < 2.0 * 2.0, WALL, v)
        return v

    parsing = (axis_distance(physical(shape, spacing), centre, direction) <= R).astype(np.int32)
    ct = np.full(shape, 37, np.int16) if flat else paint(shape, spacing, value)
    return ct, parsing, line_skeleton(shape, spacing, centre, direction, LENGTH)


def two_lumina(spacing=ANISO):
    """Two tubes along axis 0 with labels 1 and 2, their axes 2 R + T apart along axis 2: one wall between them."""
    reach = R + T + MARGIN
    half = [5, int(np.ceil(reach / spacing[1])) + 1, int(np.ceil((reach + R + T / 2.0) / spacing[2])) + 1]
    shape = tuple(2 * h + 1 for h in half)
    mid = [h * s for h, s in zip(half, spacing)]
    a = [mid[0], mid[1], mid[2] - (R + T / 2.0)]
    b = [mid[0], mid[1], mid[2] + (R + T / 2.0)]

    def value(x):
        ra, rb = axis_distance(x, a, (1, 0, 0)), axis_distance(x, b, (1, 0, 0))
        r = np.minimum(ra, rb)
        return np.where(r < R, LUMEN, np.where(r < R + T, WALL, PARENCHYMA))

    x = physical(shape, spacing)
    parsing = np.where(axis_distance(x, a, (1, 0, 0)) <= R, 1, np.where(axis_distance(x, b, (1, 0, 0)) <= R, 2, 0)).astype(np.int32)
    skeleton = line_skeleton(shape, spacing, a, (1, 0, 0), 2.0 * mid[0]) | line_skeleton(shape, spacing, b, (1, 0, 0), 2.0 * mid[0])
    return paint(shape, spacing, value), parsing, skeleton


def crescent(spacing=ANISO):
    """A lumen that is two thirds of a ring (radii 4 and 6 about an axis along axis 0): its centroid lies in the hole."""
    half = [5, int(np.ceil(10.0 / spacing[1])) + 1, int(np.ceil(10.0 / spacing[2])) + 1]
    shape = tuple(2 * h + 1 for h in half)
    mid = [h * s for h, s in zip(half, spacing)]

    def lumen(x):
        y, z = x[..., 1] - mid[1], x[..., 2] - mid[2]
        r = np.sqrt(y * y + z * z)
        return (r >= 4.0) & (r <= 6.0) & (np.abs(np.arctan2(z, y)) <= 2.0 * np.pi / 3.0)

    def value(x):
        y, z = x[..., 1] - mid[1], x[..., 2] - mid[2]
        r = np.sqrt(y * y + z * z)
        return np.where(lumen(x), LUMEN, np.where(r < 8.0, WALL, PARENCHYMA))

    parsing = lumen(physical(shape, spacing)).astype(np.int32)
    skeleton = line_skeleton(shape, spacing, [mid[0], mid[1] + 5.0, mid[2]], (1, 0, 0), 2.0 * mid[0])
    skeleton &= parsing.astype(np.uint8)
    return paint(shape, spacing, value), parsing, skeleton


def noise_ct(shape, seed=3):
    return np.random.default_rng(seed).integers(-1000, 400, shape).astype(np.int16)


def build(name):
    kind, _, arg = name.partition(":")
    kw, same_label, spacing = {}, True, ANISO
    if kind == "tube":                                       # tube:0, tube:1, tube:2, tube:oblique
        ct, parsing, skeleton = tube(OBLIQUE if arg == "oblique" else np.eye(3)[int(arg)])
    elif kind == "blob":
        ct, parsing, skeleton = tube(OBLIQUE if arg == "oblique" else np.eye(3)[int(arg)], blob=True)
    elif kind == "two_lumina":
        ct, parsing, skeleton = two_lumina()
        same_label = arg != "any"
    elif kind == "border":
        ct, parsing, skeleton = tube((1, 0, 0), cut=5.0)
    elif kind == "crescent":
        ct, parsing, skeleton = crescent()
    elif kind == "thick":                                    # a wall thicker than max_wall = 5 min(spacing) = 3.5
        ct, parsing, skeleton = tube((1, 0, 0), wall=6.0)
    elif kind == "flat":
        ct, parsing, skeleton = tube((1, 0, 0), flat=True)
    elif kind == "noise":                                    # noise:, noise:any
        parsing, skeleton, _ = cc.case("noise:")
        ct = noise_ct(parsing.shape)
        same_label = arg != "any"
    elif kind == "noise_f32":                                # values that are no integers
        parsing, skeleton, _ = cc.case("noise:")
        ct = (noise_ct(parsing.shape).astype(np.float32) * np.float32(1.0009765625) + np.float32(0.3)).astype(np.float32)
    else:
        raise KeyError(name)
    ct, parsing, skeleton = cc.frozen(np.ascontiguousarray(ct), np.ascontiguousarray(parsing), np.ascontiguousarray(skeleton))
    return {"ct": ct, "parsing": parsing, "skeleton": skeleton, "spacing": spacing, "same_label": same_label, "kw": kw}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = build(name)
    return _CACHE[name]


def sections(name):
    """The oracle's cross-sections of a case (a dict), computed once."""
    if name not in _SECTIONS:
        c = case(name)
        _SECTIONS[name] = co.cross_sections(c["parsing"], c["skeleton"], spacing=c["spacing"], same_label=c["same_label"])
    return _SECTIONS[name]


def want(name, **over):
    """The oracle's walls of a case, computed once per set of keywords."""
    key = (name, tuple(sorted(over.items())))
    if key not in _WANT:
        c = case(name)
        _WANT[key] = wo.airway_walls(c["ct"], c["parsing"], sections(name), directions(), spacing=c["spacing"],
                                     same_label=c["same_label"], **dict(c["kw"], **over))
    return _WANT[key]


TUBES = ("tube:0", "tube:1", "tube:2", "tube:oblique")
NAMED = (TUBES + ("blob:0", "blob:1", "blob:2", "blob:oblique", "two_lumina:", "two_lumina:any", "border:", "crescent:", "thick:",
                  "flat:", "noise:", "noise:any", "noise_f32:"))
