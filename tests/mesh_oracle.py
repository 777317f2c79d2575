"""Plain numpy statement of the surface meshing of DESIGN.md section 3h: the triangle table derived from the rule's text, the
extraction, the vertex adjacency, the Jacobi smoothing and the binary-STL records.  No GPU, nothing imported from the package
or from scripts/gen_mesh_table.py: the table is built here from the vectors of the rule (g x n), the generator builds it from
corner walks, and tests/test_mesh_host.py compares the two.

Numbering: corner bit 4*d0 + 2*d1 + d2; cube edge id 4*axis + 2*du + dv with (du, dv) the offsets on the other two axes, lower
axis first; vertices in raster order of their voxel, then by axis; faces in raster order of the cells, then in table order."""
import itertools

import numpy as np

CORNERS = [np.array(d) for d in itertools.product((0, 1), repeat=3)]       # CORNERS[bit] has offsets (d0, d1, d2)


def _edge_ends(e):
    axis, du, dv = e >> 2, (e >> 1) & 1, e & 1
    lo = np.zeros(3, int)
    lo[[a for a in range(3) if a != axis]] = (du, dv)
    hi = lo.copy()
    hi[axis] = 1
    return lo, hi


EDGE_ENDS = [_edge_ends(e) for e in range(12)]
EDGE_MID = [(lo + hi) / 2.0 for lo, hi in EDGE_ENDS]


def _in_face(p, f, side):
    return p[f] == side


def _fg(config, corner):
    return (config >> (4 * corner[0] + 2 * corner[1] + corner[2])) & 1


def _face_segments(config, f, side):
    """Directed segments (from edge, to edge) on one face, oriented along g x n."""
    n = np.zeros(3)
    n[f] = 1.0 if side else -1.0
    corners = [c for c in CORNERS if _in_face(c, f, side)]
    edges = [e for e in range(12) if _in_face(EDGE_ENDS[e][0], f, side) and _in_face(EDGE_ENDS[e][1], f, side)]
    cross = [e for e in edges if _fg(config, EDGE_ENDS[e][0]) != _fg(config, EDGE_ENDS[e][1])]
    centre = np.mean(corners, axis=0)

    def directed(a, b, g):
        d = np.cross(g, n)
        s = float(np.dot(EDGE_MID[b] - EDGE_MID[a], d))
        assert abs(s) > 1e-9
        return (a, b) if s > 0 else (b, a)

    if len(cross) == 2:
        fg = [c for c in corners if _fg(config, c)]
        bg = [c for c in corners if not _fg(config, c)]
        return [directed(cross[0], cross[1], np.mean(bg, axis=0) - np.mean(fg, axis=0))]
    if len(cross) == 4:                                     # ambiguous: every foreground corner is cut off on its own
        out = []
        for c in corners:
            if _fg(config, c):
                a, b = [e for e in cross if any(np.array_equal(c, end) for end in EDGE_ENDS[e])]
                out.append(directed(a, b, centre - c))
        return out
    assert not cross
    return []


def _share_face(a, b):
    for f in range(3):
        for side in (0, 1):
            if all(_in_face(end, f, side) for e in (a, b) for end in EDGE_ENDS[e]):
                return True
    return False


def _config_triangles(config):
    follow = {}
    for f in range(3):
        for side in (0, 1):
            for a, b in _face_segments(config, f, side):
                assert a not in follow
                follow[a] = b
    tris, todo = [], sorted(follow)
    while todo:
        loop, e = [], todo[0]                               # the loop with the smallest edge id, starting there
        while e in todo:
            todo.remove(e)
            loop.append(e)
            e = follow[e]
        assert e == loop[0]
        for r in range(len(loop)):
            p = loop[r:] + loop[:r]
            diagonals = [(p[0], p[k]) for k in range(2, len(p) - 1)]
            if not any(_share_face(a, b) for a, b in diagonals):
                break
        else:
            raise AssertionError(f"configuration {config}: no apex for loop {loop}")
        tris += [(p[0], p[k], p[k + 1]) for k in range(1, len(p) - 1)]
    return tris


TABLE = [_config_triangles(c) for c in range(256)]
TRI_COUNT = np.array([len(t) for t in TABLE], np.int64)
TRI_EDGES = np.full((256, 5, 3), 255, np.int64)
for _c, _t in enumerate(TABLE):
    if _t:
        TRI_EDGES[_c, :len(_t)] = _t


# ---- extraction ----------------------------------------------------------------------------------------------------------------

def offsets(level):
    """(t for a low end of 0, t for a low end of 1): formed in float64, rounded once to float32."""
    return np.float32(np.float64(level)), np.float32(1.0 - np.float64(level))


def marching_cubes(volume, level=0.95):
    """(verts float32 (V, 3), faces int32 (F, 3)) of a 3-D volume (non-zero = 1)."""
    v = (np.asarray(volume) != 0)
    assert v.ndim == 3
    n = v.shape
    if min(n) < 2:                                          # no cells: an empty mesh, vertices included
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    t0, t1 = offsets(level)
    own = np.zeros(n + (3,), bool)
    own[:-1, :, :, 0] = v[:-1] != v[1:]
    own[:, :-1, :, 1] = v[:, :-1] != v[:, 1:]
    own[:, :, :-1, 2] = v[:, :, :-1] != v[:, :, 1:]
    vid = (np.cumsum(own.reshape(-1)) - 1).reshape(own.shape)
    i0, i1, i2, ax = np.nonzero(own)
    verts = np.stack([i0, i1, i2], axis=1).astype(np.float32)
    t = np.where(v[i0, i1, i2], t1, t0).astype(np.float32)
    rows = np.arange(len(ax))
    verts[rows, ax] = verts[rows, ax] + t                   # float32 + float32
    config =np.zeros((n[0] - 1, n[1] - 1, n[2] - 1), np.int64)
    for bit, d in enumerate(CORNERS):
        config |= v[d[0]:d[0] + n[0] - 1, d[1]:d[1] + n[1] - 1, d[2]:d[2] + n[2] - 1].astype(np.int64) << bit
    ntri = TRI_COUNT[config].reshape(-1)
    cells = np.flatnonzero(ntri)
    reps = np.repeat(cells, ntri[cells])
    first = np.repeat(np.cumsum(ntri[cells]) - ntri[cells], ntri[cells])
    which = np.arange(len(reps)) - first
    c0, c1, c2 = np.unravel_index(reps, config.shape)
    edges = TRI_EDGES[config.reshape(-1)[reps], which]       # (F, 3)
    faces = np.zeros((len(reps), 3), np.int32)
    lo = np.array([EDGE_ENDS[e][0] for e in range(12)])
    for k in range(3):
        e = edges[:, k]
        o = lo[e]
        idx = vid[c0 + o[:, 0], c1 + o[:, 1], c2 + o[:, 2], e >> 2]
        assert own[c0 + o[:, 0], c1 + o[:, 1], c2 + o[:, 2], e >> 2].all()
        faces[:, k] = idx
    return verts.reshape(-1, 3), faces


# ---- adjacency -----------------------------------------------------------------------------------------------------------------

def directed_edges(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)


def adjacency(faces, n_verts):
    """(indptr int32 (V+1), indices int32, boundary uint8 (V)): the neighbours of every vertex ascending and without repeats;
    boundary = the vertex is an end of a directed edge whose reverse no face has."""
    V = int(n_verts)
    d = directed_edges(faces)
    key = d[:, 0] * max(V, 1) + d[:, 1]
    rev = d[:, 1] * max(V, 1) + d[:, 0]
    both = np.unique(np.concatenate([key, rev]))
    src, dst = both // max(V, 1), both % max(V, 1)
    indptr = np.zeros(V + 1, np.int64)
    np.add.at(indptr, src + 1, 1)
    indptr = np.cumsum(indptr)
    lone = d[~np.isin(key, rev)]
    boundary = np.zeros(V, np.uint8)
    boundary[lone.reshape(-1)] = 1
    return indptr.astype(np.int32), dst.astype(np.int32), boundary


def smooth(verts, faces, n_iter=20, relaxation_factor=0.2):
    """``n_iter`` Jacobi sweeps x' = x + l * (m - x) in float32; m = (0 + the neighbours in ascending order) / degree, one
    rounding per operation.  Boundary vertices and vertices without neighbours stay."""
    x = np.array(verts, np.float32).reshape(-1, 3)
    V = len(x)
    indptr, indices, boundary = adjacency(faces, V)
    deg = np.diff(indptr).astype(np.int64)
    lam = np.float32(relaxation_factor)
    move = (deg > 0) & (boundary == 0)
    width = int(deg.max()) if V else 0
    for _ in range(int(n_iter)):
        acc = np.zeros_like(x)
        for k in range(width):
            has = deg > k
            nb = indices[np.minimum(indptr[:-1].astype(np.int64) + k, len(indices) - 1)]
            acc = np.where(has[:, None], acc + x[nb], acc)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = acc / deg.astype(np.float32)[:, None]
        new = x + lam * (m - x)
        x = np.where(move[:, None], new, x).astype(np.float32)
    return x


# ---- affine step and STL ------------------------------------------------------------------------------------------------------

def affine(verts, centre, scale):
    return ((np.asarray(verts, np.float32) - np.asarray(centre, np.float32)) * np.asarray(scale, np.float32)).astype(np.float32)


STL_DTYPE = np.dtype([("normal", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")])
assert STL_DTYPE.itemsize == 50


def stl_records(verts, faces, centre=(0, 0, 0), scale=(1, 1, 1)):
    """uint8 (F, 50): normal, three vertices, a zero attribute word.  The normal is (b - a) x (c - a) over its length, every
    operation rounded to float32 (the squares summed x, y, z); a zero-area triangle gets 0, 0, 0."""
    p = affine(verts, centre, scale)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    u, w = b - a, c - a
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    length = np.sqrt((nx * nx + ny * ny) + nz * nz)
    rec = np.zeros(len(f), STL_DTYPE)
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.stack([nx, ny, nz], axis=1) / length[:, None]
    rec["normal"] = np.where(length[:, None] > 0, nrm, np.float32(0))
    rec["v"][:, 0], rec["v"][:, 1], rec["v"][:, 2] = a, b, c
    return rec.view(np.uint8).reshape(len(f), 50)


# ---- mesh properties the host tests use ---------------------------------------------------------------------------------------

def signed_volume(verts, faces):
    p = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def mesh_components(n_verts, faces):
    """Number of connected components among the vertices that a face uses."""
    parent = np.arange(n_verts)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for a, b in directed_edges(faces):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    used = np.unique(np.asarray(faces).reshape(-1))
    return len({find(i) for i in used})


def random_closed_volume(seed, n=14):
    """Noise or blobs with the foreground off the border."""
    rng = np.random.default_rng(seed)
    v = np.zeros((n, n, n), np.uint8)
    if seed % 2:
        v[1:-1, 1:-1, 1:-1] = rng.random((n - 2,) * 3) < 0.4
    else:
        g = np.indices((n, n, n)).astype(np.float64)
        for _ in range(6):
            c = rng.uniform(3, n - 4, 3)
            r = rng.uniform(1.2, 2.8)
            v |= (((g - c[:, None, None, None]) ** 2).sum(0) < r * r).astype(np.uint8)
        v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1] = 0, 0, 0, 0, 0, 0
    return v
