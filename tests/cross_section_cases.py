"""Synthetic inputs of the cross-section tests (tests/test_cross_section_host.py checks the oracle on them against known answers,
tests/test_cross_section_gpu.py the device against the oracle): ``(parsing int32, skeleton uint8, kwargs of cross_sections)``.
Built once per name and shared read-only."""
import numpy as np

ANISO = (1.25, 0.7, 0.7)
RADIUS = 5.0                                                 # of the cylinders, in the units of the spacing
CYLINDER_STEPS = (0.35, 0.5, 0.7)
LINE_STEP = 0.3                                              # of the straight lines: no sample falls on a voxel boundary
DIRECTIONS = ((1, 1, 0), (3, 2, 1), (1, 1, 1), (1, 2, 5))
PLANE = 63                                                   # samples per side of the section grid
_CACHE = {}


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def line(axis, spacing=ANISO):
    """A straight skeleton along ``axis`` through the middle of a 9-voxel-wide tube of label 1."""
    shape = [9, 9, 9]
    shape[axis] = 12
    parsing = np.ones(shape, np.int32)
    skeleton = np.zeros(shape, np.uint8)
    at = [4, 4, 4]
    at[axis] = slice(None)
    skeleton[tuple(at)] = 1
    return frozen(parsing, skeleton) + (dict(spacing=spacing, step=LINE_STEP),)


def cylinder(axis, step, spacing=ANISO):
    """The voxels within RADIUS (physical) of a line along ``axis`` through a voxel centre; the skeleton is that line."""
    half = [int(np.ceil(RADIUS / s)) + 2 for s in spacing]
    shape = [2 * h + 1 for h in half]
    shape[axis] = 20
    grid = np.meshgrid(*[(np.arange(n) - h) * s for n, h, s in zip(shape, half, spacing)], indexing="ij")
    r2 = sum(g * g for a, g in enumerate(grid) if a != axis)
    parsing = (r2 <= RADIUS * RADIUS).astype(np.int32)
    skeleton = np.zeros(shape, np.uint8)
    at = list(half)
    at[axis] = slice(None)
    skeleton[tuple(at)] = 1
    return frozen(parsing, skeleton) + (dict(spacing=spacing, step=step),)


def digital_line(direction, length=24):
    """The voxels round(k d / max|d|), k = 0 .. length - 1, as skeleton and as the only voxels of label 1."""
    d = np.asarray(direction, dtype=np.float64)
    pts = np.floor(np.arange(length)[:, None] * (d / np.abs(d).max())[None, :] + 0.5).astype(np.int64)
    pts -= pts.min(axis=0)
    shape = tuple(int(v) + 1 for v in pts.max(axis=0))
    skeleton = np.zeros(shape, np.uint8)
    skeleton[pts[:, 0], pts[:, 1], pts[:, 2]] = 1
    return frozen(skeleton.astype(np.int32), skeleton)


# ---- flood-fill patterns: a straight skeleton along axis 0 and a step equal to the in-plane spacing make the samples of a point
# the voxels of its slice: column i = axis 1, row j = axis 2, so the pattern drawn in every slice of `parsing` is the plane
def spiral():
    """A corridor one sample wide that winds outwards from the centre, walls one sample wide: 0/1 (PLANE, PLANE)."""
    p = np.zeros((PLANE, PLANE), np.int32)
    c = PLANE // 2
    x, y, dx, dy, run = c, c, 1, 0, 2
    p[x, y] = 1
    while True:
        for _ in range(2):
            for _ in range(run):
                x, y = x + dx, y + dy
                if not (1 <= x < PLANE - 1 and 1 <= y < PLANE - 1):
                    return p
                p[x, y] = 1
            dx, dy = -dy, dx
        run += 2


def disc(radius, centre=(0, 0), n=PLANE):
    k = np.arange(n) - n // 2
    return ((k[:, None] - centre[0]) ** 2 + (k[None, :] - centre[1]) ** 2 <= radius * radius).astype(np.int32)


def pattern(name):
    if name == "spiral":
        return spiral()
    if name == "two_discs":
        return disc(6) | disc(5, (14, -9))
    if name == "full":                                       # reaches every edge of the grid: truncated
        return np.ones((PLANE, PLANE), np.int32)
    if name == "labels":                                     # label 1 inside, a ring of label 2 around it
        return disc(6) + 2 * (disc(11) - disc(6))
    raise KeyError(name)


def plane_case(name, h=0.7):
    """``pattern(name)`` in every slice of a (5, PLANE + 4, PLANE + 4) volume, the skeleton along axis 0 through its centre."""
    n = PLANE + 4
    parsing = np.zeros((5, n, n), np.int32)
    parsing[:, 2:-2, 2:-2] = pattern(name)[None]
    skeleton = np.zeros(parsing.shape, np.uint8)
    skeleton[:, n // 2, n // 2] = 1
    return frozen(parsing, skeleton) + (dict(spacing=(1.25, h, h), step=h),)


def corner_case(h=0.7):
    """The skeleton along axis 0 at (., 0, 0), a 5 x 5 block of label 1 around it: most samples fall outside the volume."""
    parsing = np.zeros((5, 9, 9), np.int32)
    parsing[:, :5, :5] = 1
    skeleton = np.zeros(parsing.shape, np.uint8)
    skeleton[:, 0, 0] = 1
    return frozen(parsing, skeleton) + (dict(spacing=(1.25, h, h), step=h),)


def noise(shape=(12, 13, 14), labels=3, seed=7, density=0.5):
    """Label noise with a random skeleton: degenerate windows and tiny sections."""
    rng = np.random.default_rng(seed)
    parsing = rng.integers(0, labels + 1, shape).astype(np.int32)
    skeleton = (rng.random(shape) < density).astype(np.uint8)
    return frozen(parsing, skeleton) + (dict(spacing=ANISO),)


def y_tree(n=40):
    """A Y of three tubes as a 0/1 mask: a trunk along axis 0 that splits into two oblique arms."""
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).astype(np.float64)
    mask = np.zeros((n, n, n), bool)
    c = n / 2.0

    def tube(a, b, r):
        a, b = np.asarray(a, float), np.asarray(b, float)
        ab = b - a
        t = np.clip(((g - a) * ab).sum(-1) / (ab * ab).sum(), 0.0, 1.0)
        d = g - (a + t[..., None] * ab)
        return (d * d).sum(-1) <= r * r

    mask |= tube((3, c, c), (n * 0.5, c, c), 4.0)
    mask |= tube((n * 0.5, c, c), (n - 5, c - 10, c + 4), 3.0)
    mask |= tube((n * 0.5, c, c), (n - 5, c + 10, c - 4), 3.0)
    return frozen(mask.astype(np.uint8))[0]


def case(name):
    """(parsing, skeleton, kwargs) by name, built once."""
    if name not in _CACHE:
        kind, _, arg = name.partition(":")
        if kind == "line":
            _CACHE[name] = line(int(arg))
        elif kind == "cylinder":
            axis, step = arg.split(",")
            _CACHE[name] = cylinder(int(axis), float(step))
        elif kind == "oblique":
            p, s = digital_line(DIRECTIONS[int(arg)])
            _CACHE[name] = (p, s, {})
        elif kind == "plane":
            _CACHE[name] = plane_case(arg)
        elif kind == "plane_any":                            # the label pattern with same_label=False
            p, s, kw = plane_case(arg)
            _CACHE[name] = (p, s, dict(kw, same_label=False))
        elif kind == "corner":
            _CACHE[name] = corner_case()
        elif kind == "noise":
            _CACHE[name] = noise()
        else:
            raise KeyError(name)
    return _CACHE[name]


SYNTHETIC = (("line:0", "line:1", "line:2") + tuple(f"cylinder:{a},{h}" for a in range(3) for h in CYLINDER_STEPS)
             + tuple(f"oblique:{k}" for k in range(len(DIRECTIONS)))
             + ("plane:spiral", "plane:two_discs", "plane:full", "plane:labels", "plane_any:labels", "corner:", "noise:"))
