"""Plain numpy statement of the labelled surface meshing of DESIGN.md section 3i, built on tests/mesh_oracle.py alone: the mesh of
label k of an integer volume L is ``mesh_oracle.marching_cubes(L == k, level)``, and the result is the concatenation of these
meshes for k = 1 .. num in label order, the faces shifted by the vertices before them.  ``branch_meshes`` composes that with
``mesh_oracle.affine`` and ``mesh_oracle.smooth`` per label.  No GPU, nothing imported from the package."""
import numpy as np

import mesh_oracle as mo


def label_meshes(L, num=None, level=0.95):
    """(verts float32 (V, 3), faces int32 (F, 3), vert_ptr int64 (num + 1), face_ptr int64 (num + 1))."""
    L = np.asarray(L)
    assert L.ndim == 3
    if num is None:
        num = max(int(L.max()), 0) if L.size else 0
    verts, faces = [np.zeros((0, 3), np.float32)], [np.zeros((0, 3), np.int32)]
    vert_ptr, face_ptr = np.zeros(num + 1, np.int64), np.zeros(num + 1, np.int64)
    present = set(np.unique(L).tolist())
    for k in range(1, num + 1):
        vert_ptr[k], face_ptr[k] = vert_ptr[k - 1], face_ptr[k - 1]
        if k not in present:                                # the reference skips such labels; their slices are empty
            continue
        v, f = mo.marching_cubes(L == k, level)
        verts.append(v)
        faces.append((f.astype(np.int64) + vert_ptr[k - 1]).astype(np.int32))
        vert_ptr[k] += len(v)
        face_ptr[k] += len(f)
    return np.concatenate(verts), np.concatenate(faces), vert_ptr, face_ptr


def mesh(result, k):
    """Label k's own (verts, faces) out of a result of ``label_meshes``."""
    verts, faces, vert_ptr, face_ptr = result
    return verts[vert_ptr[k - 1]:vert_ptr[k]], faces[face_ptr[k - 1]:face_ptr[k]] - np.int32(vert_ptr[k - 1])


def branch_meshes(L, spacing=None, centre=None, num=None, level=0.95, smooth=True, n_iter=20, relaxation_factor=0.15):
    """Per label: extraction, ``affine(verts, centre, spacing)`` when either is given, ``smooth``; then the concatenation."""
    res = label_meshes(L, num, level)
    verts = res[0].copy()
    for k in range(1, len(res[2])):
        v, f = mesh(res, k)
        if not len(v):
            continue
        if centre is not None or spacing is not None:
            v = mo.affine(v, (0, 0, 0) if centre is None else centre, (1, 1, 1) if spacing is None else spacing)
        if smooth:
            v = mo.smooth(v, f, n_iter, relaxation_factor)
        verts[res[2][k - 1]:res[2][k]] = v
    return (verts,) + res[1:]


def random_labels(shape, labels, density, seed):
    """Seeded volume with values 0 .. labels: a voxel is non-zero with probability ``density``, its label uniform."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, labels + 1, shape) * (rng.random(shape) < density)).astype(np.int32)


def set_partitions(n):
    """Every partition of range(n) as a list of block numbers per element (restricted growth strings)."""
    def grow(prefix, blocks):
        if len(prefix) == n:
            yield list(prefix)
            return
        for b in range(blocks + 1):
            yield from grow(prefix + [b], max(blocks, b + 1))
    yield from grow([], 0)
