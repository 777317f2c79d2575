"""Surface meshing on the GPU: the last step of the reference's deployment path (prediction.py:121-149) -- mask to smoothed,
centred, scaled triangle mesh and a binary STL file (csrc/mesh.hip).

The reference calls ``skimage.measure.marching_cubes_lewiner(result, 0.95)``, centres the vertices on the mean skeleton
coordinate, scales them by ``spacing / 10``, copies every face into a numpy-stl mesh in a Python loop and smooths the saved file
with ``pyvista``'s ``smooth(relaxation_factor=0.2)``.  Here the extraction follows the rule written out in DESIGN.md 3h (one
vertex per sign-changing grid edge at the position Lewiner's rule gives it, ambiguous faces always separating the foreground
corners as Lewiner's face test does on a 0/1 volume at level 0.95; the cut of a cell's polygon into triangles and Lewiner's rare
interior cases differ) and the smoothing is ``n_iter`` Jacobi sweeps with fixed boundary vertices (VTK's update order and
boundary handling are not reproduced).  Equality with skimage or VTK is not claimed; every result equals tests/mesh_oracle.py bit
for bit and is deterministic.

``label_meshes`` / ``branch_meshes`` (csrc/mesh_label.hip) make the meshes of all the labels of a ``parsing``
volume in one extraction -- the per-branch models of the reference's tree tools (ours_skel_parse.py:1101-1152) -- each label's
mesh bit for bit ``marching_cubes(parsing == k)``; tests/mesh_label_oracle.py states the concatenation.

CUDA tensors in -> CUDA tensors out, numpy arrays in -> numpy arrays out; there is no CPU path."""
from __future__ import annotations

import ctypes as C
import struct
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._volume import mask_in, out as _out, read_status, workspace
from .prep import _labels_in, _vol, skeletonize_3d

_PREFIX = "seunet mesh"


def _mask_in(a, name):
    return mask_in(a, name, _PREFIX, _vol)


def _level(level) -> float:
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"{_PREFIX}: level must lie strictly between 0 and 1, got {level}")
    return level


def _mesh_in(verts, faces):
    """(verts float32 (V, 3) CUDA, faces int32 (F, 3) CUDA, came-as-numpy)."""
    as_numpy = isinstance(verts, np.ndarray)
    if as_numpy != isinstance(faces, np.ndarray):
        raise TypeError(f"{_PREFIX}: `verts` and `faces` must both be numpy arrays or both CUDA tensors")
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{_PREFIX}: needs a GPU (there is no CPU path)")
        verts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).cuda()
        faces = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).cuda()
    for t, name in ((verts, "verts"), (faces, "faces")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{_PREFIX}: `{name}` must be a CUDA tensor resident on the GPU (there is no CPU path)")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{_PREFIX}: `{name}` must be (n, 3), got {tuple(t.shape)}")
    if verts.dtype != torch.float32:
        raise TypeError(f"{_PREFIX}: `verts` has dtype {verts.dtype}; expected float32")
    if faces.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{_PREFIX}: `faces` has dtype {faces.dtype}; expected int32")
    if faces.device != verts.device:
        raise ValueError(f"{_PREFIX}: `faces` is on {faces.device}, `verts` on {verts.device}")
    return verts.contiguous(), faces.to(torch.int32).contiguous(), as_numpy


def _float3(v, name) -> Optional[C.Array]:
    """Three values -> a host float32[3]; each is rounded once from float64."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size != 3:
        raise ValueError(f"{_PREFIX}: `{name}` must hold 3 values, got {a.size}")
    return (C.c_float * 3)(*[float(np.float32(x)) for x in a])


def _index_status(status, what):
    if read_status(status) != 0:
        raise ValueError(f"{_PREFIX}: {what}: `faces` holds an index outside 0 .. V - 1")


# ---- extraction -----------------------------------------------------------------------------------------------------------------

def marching_cubes(volume, level: float = 0.95):
    """Triangle mesh of the 0/1 ``volume`` (uint8 / bool CUDA tensor or numpy array of any dtype, non-zero = 1, shape (n0, n1,
    n2)) -> ``(verts float32 (V, 3), faces int32 (F, 3))`` in voxel coordinates, no padding (a foreground voxel on the border
    leaves the surface open there).  ``level`` places a vertex at ``level`` from the background end of its grid edge.  The right-
    hand normals point out of the mask.  An empty result is a pair of (0, 3) arrays; a volume with an extent of 1 has no cells and
    gives one.  Reading the two output sizes synchronises once."""
    level = _level(level)
    vol, as_numpy = _mask_in(volume, "volume")
    n0, n1, n2 = (int(v) for v in vol.shape)
    dev = vol.device
    nv, nf = C.c_longlong(0), C.c_longlong(0)
    lib = _lib.load()
    with torch.cuda.device(dev):
        if vol.numel():
            ws = workspace(lib.seunet_mesh_workspace_bytes, n0, n1, n2, device=dev, what=f"{_PREFIX}: marching_cubes")
            _lib.check(lib.seunet_mesh_count(vol.data_ptr(), n0, n1, n2, C.byref(nv), C.byref(nf), ws.data_ptr(), ws.numel(),
                                             _lib.stream_ptr()), "mesh_count")
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf.value, 3), dtype=torch.int32, device=dev)
        if nv.value or nf.value:
            _lib.check(lib.seunet_mesh_emit(n0, n1, n2, level, nv.value, nf.value, verts.data_ptr(), faces.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _lib.stream_ptr()), "mesh_emit")
    return _out(verts, as_numpy), _out(faces, as_numpy)


# ---- every label's mesh of a parsing volume ----------------------------------------------------------------------------------------

MAX_LABELS = 65535
_INT32_MAX = 2 ** 31 - 1


class LabelMeshes(NamedTuple):
    """The meshes of the labels 1 .. num, concatenated in label order: label k owns ``verts[vert_ptr[k-1]:vert_ptr[k]]`` and
    ``faces[face_ptr[k-1]:face_ptr[k]]``; ``faces`` index the concatenated ``verts``.  ``vert_ptr`` / ``face_ptr``: host numpy
    int64 of length num + 1."""
    verts: object
    faces: object
    vert_ptr: np.ndarray
    face_ptr: np.ndarray

    @property
    def num(self) -> int:
        return len(self.vert_ptr) - 1

    def mesh(self, k: int):
        """``(verts_k, faces_k)`` of label k (1 .. num), the faces indexing ``verts_k``: what ``marching_cubes(parsing == k)``
        gives.  Slices, no copy of the vertices."""
        k = int(k)
        if not 1 <= k <= self.num:
            raise IndexError(f"{_PREFIX}: label {k} outside 1 .. {self.num}")
        v0, v1 = int(self.vert_ptr[k - 1]), int(self.vert_ptr[k])
        f0, f1 = int(self.face_ptr[k - 1]), int(self.face_ptr[k])
        faces = self.faces[f0:f1]
        return self.verts[v0:v1], (faces - np.int32(v0) if isinstance(faces, np.ndarray) else faces - v0)


def label_meshes(parsing, num: Optional[int] = None, level: float = 0.95) -> LabelMeshes:
    """The mesh of every label of an integer label volume (CUDA tensor int32 / int64 / int16 / uint8 or numpy array of any integer
    dtype, shape (n0, n1, n2), values 0 .. num, 0 = background; non-contiguous is fine) in one extraction: label k's mesh is
    bit for bit ``marching_cubes(parsing == k, level)``, and the result is their concatenation for k = 1 .. ``num`` (see
    ``LabelMeshes``).  ``num=None``: the largest label present, found on the device.  A grid edge between two different non-zero
    labels carries one vertex for each of them.  A label without voxels, a volume with an extent of 1 and a volume without labels
    give empty slices.  ValueError: a negative label, a label above an explicit ``num``, more than 65535 labels, ``V`` or ``3 F``
    beyond int32.  The sizes and the two pointer arrays are read after the call's one synchronise."""
    level = _level(level)
    if num is not None:
        num = int(num)
        if not 0 <= num <= MAX_LABELS:
            raise ValueError(f"{_PREFIX}: label_meshes: num must lie in 0 .. {MAX_LABELS}, got {num}")
    lab, as_numpy = _labels_in(parsing, "parsing")
    n0, n1, n2 = (int(v) for v in lab.shape)
    dev = lab.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        if lab.numel() == 0:
            n = num or 0
            empty = LabelMeshes(torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
                                np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64))
            return empty._replace(verts=_out(empty.verts, as_numpy), faces=_out(empty.faces, as_numpy))
        cap = MAX_LABELS + 1 if num is None else num + 1
        ptrs = torch.empty((2, cap), dtype=torch.int64, device=dev)
        ws = workspace(lib.seunet_mesh_label_workspace_bytes, n0, n1, n2, device=dev, what=f"{_PREFIX}: label_meshes")
        nv, nf, used, status = C.c_longlong(0), C.c_longlong(0), C.c_int(0), C.c_int(0)
        _lib.check(lib.seunet_mesh_label_count(lab.data_ptr(), n0, n1, n2, -1 if num is None else num, C.byref(nv), C.byref(nf),
                                               C.byref(used), C.byref(status), ptrs[0].data_ptr(), ptrs[1].data_ptr(), cap,
                                               ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "mesh_label_count")
        if status.value & 1:
            raise ValueError(f"{_PREFIX}: label_meshes: `parsing` holds a negative label")
        if status.value & 2:
            raise ValueError(f"{_PREFIX}: label_meshes: `parsing` holds a label above " +
                             (f"{MAX_LABELS}, the most labels one call takes" if num is None else f"num = {num}"))
        V, F, n = nv.value, nf.value, used.value
        if V > _INT32_MAX or 3 * F > _INT32_MAX:
            raise ValueError(f"{_PREFIX}: label_meshes: {V} vertices / {F} faces: V or 3 F exceeds the int32 index range")
        host_ptrs = ptrs[:, :n + 1].cpu().numpy()              # the stream is idle after the count call's synchronise
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        if V or F:
            sort_ws = workspace(lib.seunet_mesh_label_sort_bytes, V, F, device=dev, what=f"{_PREFIX}: label_meshes")
            _lib.check(lib.seunet_mesh_label_emit(lab.data_ptr(), n0, n1, n2, n, level, V, F, verts.data_ptr(), faces.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), sort_ws.data_ptr(), sort_ws.numel(), _lib.stream_ptr()),
                       "mesh_label_emit")
    return LabelMeshes(_out(verts, as_numpy), _out(faces, as_numpy), np.ascontiguousarray(host_ptrs[0]),
                       np.ascontiguousarray(host_ptrs[1]))


def branch_meshes(parsing, spacing=None, centre=None, num: Optional[int] = None, level: float = 0.95, smooth: bool = True,
                  n_iter: int = 20, relaxation_factor: float = 0.15) -> LabelMeshes:
    """The per-branch models of the reference's tree tool (ours_skel_parse.py:1110-1119, ``sub_model``) for all branches at once,
    in its order of steps: ``label_meshes(parsing, num, level)``, ``transform_mesh(verts, centre, spacing)`` (``(v - centre) *
    spacing``; the reference uses one centre ``o`` for the whole tree -- ``mean_coordinate`` gives it -- and both None is the
    ATM'22 tool's variant without centring, tree_parsing.py:167-176), then ``smooth_mesh`` with the reference's relaxation factor
    0.15.  The labels' meshes share no vertex, so the one smoothing call equals smoothing every label's mesh on its own bit for
    bit.  ``write_stl(path, *meshes.mesh(k))`` writes one branch."""
    m = label_meshes(parsing, num, level)
    verts = m.verts
    if centre is not None or spacing is not None:
        verts = transform_mesh(verts, centre, spacing)
    if smooth:
        verts = smooth_mesh(verts, m.faces, n_iter, relaxation_factor)
    return m._replace(verts=verts)


# ---- adjacency and smoothing ----------------------------------------------------------------------------------------------------

def _adjacency(faces, n_verts):
    dev = faces.device
    F = int(faces.shape[0])
    lib = _lib.load()
    with torch.cuda.device(dev):
        indptr = torch.empty(n_verts + 1, dtype=torch.int32, device=dev)
        room = torch.empty(6 * F, dtype=torch.int32, device=dev)
        boundary = torch.empty(n_verts, dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ws = workspace(lib.seunet_mesh_adjacency_workspace_bytes, n_verts, F, device=dev, what=f"{_PREFIX}: mesh_adjacency")
        _lib.check(lib.seunet_mesh_adjacency(faces.data_ptr(), F, n_verts, indptr.data_ptr(), room.data_ptr(), 6 * F,
                                             boundary.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                   "mesh_adjacency")
        _index_status(status, "mesh_adjacency")
    return indptr, room, boundary


def mesh_adjacency(faces, n_verts: int):
    """Vertex neighbour lists of a triangle mesh in CSR form -> ``(indptr int32 (V + 1), indices int32, boundary uint8 (V))``:
    the neighbours of vertex v are ``indices[indptr[v]:indptr[v + 1]]``, ascending and without repeats; ``boundary[v]`` is 1
    where v is an end of a directed face edge whose reverse no face has.  Independent of the device's scheduling."""
    as_numpy = isinstance(faces, np.ndarray)
    _, f, _ = _mesh_in(np.zeros((0, 3), np.float32) if as_numpy else torch.empty((0, 3), dtype=torch.float32, device=faces.device),
                       faces)
    n_verts = int(n_verts)
    if n_verts < 0:
        raise ValueError(f"{_PREFIX}: n_verts must not be negative")
    indptr, room, boundary = _adjacency(f, n_verts)
    indices = room[:int(indptr[-1].item())].clone()
    return _out(indptr, as_numpy), _out(indices, as_numpy), _out(boundary, as_numpy)


def smooth_mesh(verts, faces, n_iter: int = 20, relaxation_factor: float = 0.2):
    """``n_iter`` Jacobi sweeps ``x' = x + relaxation_factor * (m - x)`` with m the mean of the neighbouring vertices (summed in
    ascending index order, float32, one rounding per operation); boundary vertices and vertices no face uses stay where they
    are.  The defaults are pyvista's ``n_iter`` with the reference's relaxation factor (prediction.py:147); VTK's own update
    order and boundary handling are not reproduced.  Returns the new ``verts``; the input is not modified."""
    v, f, as_numpy = _mesh_in(verts, faces)
    n_iter = int(n_iter)
    if n_iter < 0:
        raise ValueError(f"{_PREFIX}: n_iter must not be negative")
    V = int(v.shape[0])
    dev = v.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = torch.empty((V, 3), dtype=torch.float32, device=dev)
        if n_iter == 0 or V == 0:
            out.copy_(v)
            return _out(out, as_numpy)
        indptr, indices, boundary = _adjacency(f, V)
        tmp = torch.empty((V, 3), dtype=torch.float32, device=dev) if n_iter > 1 else None
        _lib.check(lib.seunet_mesh_smooth(v.data_ptr(), V, indptr.data_ptr(), indices.data_ptr(), boundary.data_ptr(), n_iter,
                                          float(relaxation_factor), out.data_ptr(), _lib.ptr(tmp), _lib.stream_ptr()), "mesh_smooth")
    return _out(out, as_numpy)


# ---- affine step, STL -----------------------------------------------------------------------------------------------------------

def transform_mesh(verts, centre=None, scale=None):
    """``(verts - centre) * scale`` per axis in float32 (``centre`` / ``scale``: 3 values each, rounded once to float32; None: 0 /
    1).  Returns new ``verts``."""
    as_numpy = isinstance(verts, np.ndarray)
    v, _, _ = _mesh_in(verts, np.zeros((0, 3), np.int32) if as_numpy else torch.empty((0, 3), dtype=torch.int32, device=verts.device))
    c, s = _float3(centre, "centre"), _float3(scale, "scale")
    with torch.cuda.device(v.device):
        out = torch.empty_like(v)
        _lib.check(_lib.load().seunet_mesh_affine(v.data_ptr(), int(v.shape[0]), c, s, out.data_ptr(), _lib.stream_ptr()), "mesh_affine")
    return _out(out, as_numpy)


def stl_records(verts, faces, centre=None, scale=None):
    """The binary-STL records of a mesh -> uint8 ``(F, 50)``: unit normal of ``(b - a) x (c - a)`` (zeros for a zero-area
    triangle), the three vertices, a zero attribute word; ``centre`` / ``scale`` apply ``transform_mesh`` on the way."""
    v, f, as_numpy = _mesh_in(verts, faces)
    c, s = _float3(centre, "centre"), _float3(scale, "scale")
    F = int(f.shape[0])
    dev = v.device
    with torch.cuda.device(dev):
        rec = torch.empty((F, 50), dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().seunet_mesh_stl_records(v.data_ptr(), int(v.shape[0]), f.data_ptr(), F, c, s, rec.data_ptr(),
                                                       status.data_ptr(), _lib.stream_ptr()), "mesh_stl_records")
        _index_status(status, "stl_records")
    return _out(rec, as_numpy)


def write_stl(path_or_file, verts, faces, header: bytes = b"") -> int:
    """Write the mesh as a binary STL: an 80-byte header (``header`` padded with zeros), the uint32 face count and the records
    of ``stl_records`` -- one copy from the device.  ``path_or_file``: a path or a binary file object.  Returns the bytes
    written (84 + 50 F)."""
    header = bytes(header)
    if len(header) > 80:
        raise ValueError(f"{_PREFIX}: the STL header holds at most 80 bytes, got {len(header)}")
    rec = stl_records(verts, faces)
    rec = rec if isinstance(rec, np.ndarray) else rec.cpu().numpy()
    data = header.ljust(80, b"\0") + struct.pack("<I", rec.shape[0]) + rec.tobytes()
    if hasattr(path_or_file, "write"):
        path_or_file.write(data)
    else:
        with open(path_or_file, "wb") as f:
            f.write(data)
    return len(data)


# ---- the reference's mesh step ----------------------------------------------------------------------------------------------------

def coordinate_sums(mask) -> Tuple[int, int, int, int]:
    """(count, sum of i0, sum of i1, sum of i2) over the non-zero voxels of ``mask`` as exact Python ints (synchronises)."""
    vol, _ = _mask_in(mask, "mask")
    n0, n1, n2 = (int(v) for v in vol.shape)
    if vol.numel() == 0:
        return 0, 0, 0, 0
    with torch.cuda.device(vol.device):
        sums = torch.empty(4, dtype=torch.int64, device=vol.device)
        _lib.check(_lib.load().seunet_mesh_coord_sums(vol.data_ptr(), n0, n1, n2, sums.data_ptr(), _lib.stream_ptr()), "mesh_coord_sums")
    return tuple(int(v) for v in sums.cpu().tolist())


def mean_coordinate(mask) -> np.ndarray:
    """Mean coordinate of the non-zero voxels -> float32 (3,): the exact integer sums divided in float64 and rounded once.  (The
    reference takes ``np.mean`` of float32 columns, a pairwise float32 sum that can differ in the last bits.)"""
    count, s0, s1, s2 = coordinate_sums(mask)
    if count == 0:
        raise ValueError(f"{_PREFIX}: mean_coordinate: the mask is empty")
    return (np.array([s0, s1, s2], dtype=np.float64) / np.float64(count)).astype(np.float32)


def prediction_mesh(mask, spacing: Sequence[float], flip: bool = False, level: float = 0.95, smooth: bool = True, skeleton=None):
    """prediction.py:121-149 in order: flip of axis 0 (what the per-``y`` ``np.flipud`` does), ``marching_cubes(mask, level)``,
    centring on the mean coordinate of the skeleton (``skeletonize_3d`` of the flipped mask when ``skeleton`` is None; a passed
    ``skeleton`` belongs to the mask as given and is flipped with it), scaling by ``spacing / 10`` and ``smooth_mesh`` with its
    defaults.  Returns ``(verts, faces)``; ``write_stl`` makes the file."""
    spacing = np.asarray(spacing, dtype=np.float64).reshape(-1)
    if spacing.size != 3:
        raise ValueError(f"{_PREFIX}: `spacing` must hold 3 values, got {spacing.size}")
    level = _level(level)
    vol, as_numpy = _mask_in(mask, "mask")
    skel = None if skeleton is None else _mask_in(skeleton, "skeleton")[0]
    if skel is not None and skel.shape != vol.shape:
        raise ValueError(f"{_PREFIX}: `skeleton` shape {tuple(skel.shape)} differs from `mask`'s {tuple(vol.shape)}")
    if flip:
        vol = vol.flip(0).contiguous()
        skel = None if skel is None else skel.flip(0).contiguous()
    verts, faces = marching_cubes(vol, level)
    if skel is None:
        skel = skeletonize_3d(vol)
    verts = transform_mesh(verts, mean_coordinate(skel), spacing / 10.0)
    if smooth:
        verts = smooth_mesh(verts, faces)
    return _out(verts, as_numpy), _out(faces, as_numpy)
