"""Volumes of more than 2^20 packed words, and meshes of more than 2^20 vertices and 2^22 items: the sizes at which the exclusive
scan of csrc/bitvol.hip (``run_scan``) leaves its first chunk.  ``scan_block_kernel`` scans blocks of
``SCAN_BLOCK`` elements; ``scan_top_kernel``, one workgroup of ``TOP_THREADS`` threads, scans the block totals in chunks of
``TOP_THREADS`` and hands a 64-bit carry from chunk to chunk.  A chunk therefore covers ``CHUNK`` = 2^20 scanned elements, and
every case below is the smallest that reaches what its line names.  The last axis is 2, so a row is one word (2 valid bits) and
the words are the rows: word = i0 * n1 + i1, and a block of the scan is 1024 rows.

The builders run each numpy oracle once per process and keep the result (``mesh``, ``adjacency``, ``smoothed``, ``labels``,
``surface``), as ``case()`` does in tests/test_mesh_gpu.py and tests/test_surface_host.py.  tests/test_volume_large_host.py
proves without a GPU that every case reaches the mechanism it names; tests/test_volume_large_gpu.py runs them."""
import numpy as np

import mesh_label_oracle as lo
import mesh_oracle as mo
import surface_oracle as so

SCAN_BLOCK = 1024                 # kScanBlock (csrc/bitvol.h)
TOP_THREADS = 1024                # threads of scan_top_kernel = its chunk step (csrc/bitvol.hip)
SORT_BLOCK = 1024                 # kSortBlock (csrc/volume.h)
CHUNK = SCAN_BLOCK * TOP_THREADS  # scanned elements per chunk of the top scan: 2^20

LEVEL = 0.95
SPACING = (1.25, 0.7, 0.7)
LABEL_NUM = 300

# name -> (shape, zeroed planes or None, words, block totals, chunks of the top scan)
CASES = {
    "exact": ((1024, 1024, 2), None, 1048576, 1024, 1),        # one full chunk, no second: thread 1023's carry write, the total
    "one_more": ((1025, 1024, 2), None, 1049600, 1025, 2),     # a second chunk of one full block
    "ragged": ((1027, 1023, 2), None, 1050621, 1026, 2),       # a second chunk whose last block holds 1021 elements
    "three": ((2049, 1024, 2), None, 2098176, 2049, 3),        # a third chunk: the carry is handed on twice
    # noise in planes 0..63 and 961..1024 only: 897 zero block totals in a row inside the first chunk, then the second chunk
    "ends": ((1025, 1024, 2), (64, 961), 1049600, 1025, 2),
    # noise in planes 0..63 and 1036..1099 only: zero counts on both sides of the chunk border (plane 1024); the offsets of the
    # second chunk's first twelve blocks are the carry and nothing else
    "gap": ((1100, 1024, 2), (64, 1036), 1126400, 1100, 2),
}
MESH_CASES = ["exact", "one_more", "ragged", "three", "ends", "gap"]
SURFACE_CASES = ["one_more", "ragged", "ends", "gap"]

_CACHE = {}


def noise(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def volume(name, seed):
    """``noise(shape, 0.5, seed)`` of the case, its zeroed planes cleared."""
    shape, zero = CASES[name][:2]
    v = noise(shape, 0.5, seed)
    if zero is not None:
        v[zero[0]:zero[1]] = 0
    return v


def word_count(shape):
    return shape[0] * shape[1] * ((shape[2] + 63) // 64)


def block_totals(n):
    return (n + SCAN_BLOCK - 1) // SCAN_BLOCK


def chunks(n):
    """Trips of scan_top_kernel's loop over the block totals of ``n`` scanned elements."""
    return (block_totals(n) + TOP_THREADS - 1) // TOP_THREADS


def chunk_borders(n):
    """The scanned-element indices at which a later chunk of the top scan begins."""
    return [c * CHUNK for c in range(1, chunks(n))]


def sort_bins(n):
    """Elements of the histogram scan of one radix pass over ``n`` items."""
    return 256 * ((n + SORT_BLOCK - 1) // SORT_BLOCK)


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- marching_cubes, adjacency, smoothing -----------------------------------------------------------------------------------------
def mesh(name):
    """(volume, oracle verts, oracle faces) at level 0.95."""
    def make():
        v = volume(name, 11)
        return (v,) + mo.marching_cubes(v, LEVEL)
    return _once(("mesh", name), make)


def adjacency():
    """``mesh_oracle.adjacency`` of the mesh of ``one_more``."""
    def make():
        _, verts, faces = mesh("one_more")
        return mo.adjacency(faces, len(verts))
    return _once("adjacency", make)


def smoothed():
    """One sweep of ``mesh_oracle.smooth`` over the mesh of ``one_more``, relaxation factor 0.2."""
    def make():
        _, verts, faces = mesh("one_more")
        return mo.smooth(verts, faces, 1, 0.2)
    return _once("smoothed", make)


# ---- label_meshes -----------------------------------------------------------------------------------------------------------------
def labels():
    """(L int32 with the labels 1 and 300, ``mesh_label_oracle.label_meshes(L)``) on the shape of ``one_more``."""
    def make():
        L = lo.random_labels(CASES["one_more"][0], 2, 0.9, 2)
        L[L == 2] = LABEL_NUM
        return L, lo.label_meshes(L)
    return _once("labels", make)


def relabel_result(res, top):
    """The oracle's result for the volume whose largest label ``LABEL_NUM`` is renamed to ``top`` (> 1), from its result ``res``
    for the labels 1 and ``LABEL_NUM``: the result is the concatenation of the labels' meshes in label order, so vertices and faces
    stay and only the pointer arrays change their length (tests/test_volume_large_host.py checks this against the oracle on a
    small volume)."""
    verts, faces, vert_ptr, face_ptr = res
    vp, fp = np.full(top + 1, vert_ptr[1], np.int64), np.full(top + 1, face_ptr[1], np.int64)
    vp[0] = fp[0] = 0
    vp[top], fp[top] = vert_ptr[-1], face_ptr[-1]
    return verts, faces, vp, fp


# The radix passes write their histogram digit-major: digit d of ceil(n / SORT_BLOCK) blocks fills the bins [d * blocks, (d + 1) *
# blocks).  With n a little over 2^22 items the bins past CHUNK belong to the digits from 207 on, and the labels 1 and 300 have the
# digits 1, 44 (low) and 0, 1 (high): every item's bin lies in the first chunk of the histogram scan, and the second chunk scans
# zeros that no item reads.  So the sorts get labellings of their own, the same voxels with the larger label renamed:
#   65535: digits 1, 255 (low) and 0, 255 (high): items on both sides of the chunk border in both passes;
#   255:   digits 1, 255 in the one pass of num < 256.
LABEL_TOPS = {"two_passes": 65535, "one_pass": 255}


def labels_renamed(which):
    """(L with ``LABEL_NUM`` renamed to ``LABEL_TOPS[which]``, the oracle's result for it)."""
    def make():
        L, res = labels()
        top = LABEL_TOPS[which]
        return np.where(L == LABEL_NUM, top, L).astype(np.int32), relabel_result(res, top)
    return _once(("labels", which), make)


def labels_first_only():
    """(L with ``LABEL_NUM`` cleared, the oracle's result for it with num = 1): label 1's slice of ``labels()``."""
    def make():
        L, (verts, faces, vert_ptr, face_ptr) = labels()
        return (np.where(L == LABEL_NUM, 0, L).astype(np.int32),
                (verts[:vert_ptr[1]], faces[:face_ptr[1]], vert_ptr[:2].copy(), face_ptr[:2].copy()))
    return _once(("labels", "first"), make)


def digit_bins(n, labels, shift):
    """The bin ranges [first, last) of a radix pass over ``n`` items that the digits of ``labels`` fill."""
    blocks = (n + SORT_BLOCK - 1) // SORT_BLOCK
    return sorted({((k >> shift) & 255) * blocks: ((k >> shift) & 255) * blocks + blocks for k in labels}.items())


# ---- surface distances ------------------------------------------------------------------------------------------------------------
def surface_masks(name):
    """(a, b, border of a, border of b): the masks ``noise(shape, 0.5, 3 / 4)`` and ``surface_oracle.border`` of each."""
    def make():
        a, b = volume(name, 3), volume(name, 4)
        return a, b, so.border(a), so.border(b)
    return _once(("masks", name), make)


def surface(name):
    """(a, b, spacing, D, n_a, n_b, voxels) as ``case()`` of tests/test_surface_host.py gives them.  Counts and voxel indices come
    from ``surface_oracle.border``; the distances from scipy's transform, which ``surface_oracle`` states bit for bit in Python
    loops that would take a minute here (tests/test_volume_large_host.py compares the two on a small mask).  ``D`` is None where
    scipy is not installed."""
    def make():
        a, b, ba, bb = surface_masks(name)
        voxels = np.concatenate([np.flatnonzero(ba), np.flatnonzero(bb)]).astype(np.int32)
        try:
            from scipy import ndimage
        except ImportError:
            D = None
        else:
            s = [float(v) for v in SPACING]
            D = np.concatenate([ndimage.distance_transform_edt(~bb, sampling=s)[ba], ndimage.distance_transform_edt(~ba, sampling=s)[bb]])
        return a, b, SPACING, D, int(ba.sum()), int(bb.sum()), voxels
    return _once(("surface", name), make)


def metrics(name, tolerances):
    """``surface_oracle.metrics`` of the case's distances at the 95th percentile (None without scipy)."""
    def make():
        _, _, _, D, n_a, n_b, _ = surface(name)
        return None if D is None else so.metrics(D, n_a, n_b, 95.0, tolerances)
    return _once(("metrics", name, tuple(tolerances)), make)
