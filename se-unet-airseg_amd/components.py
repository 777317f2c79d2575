"""Connected components and the topological numbers of a binary volume on the GPU (csrc/betti.hip).

``label`` is ``scipy.ndimage.label`` bit for bit (components numbered ``1..N`` in raster order of their first voxels) with an optional
component table; ``remove_small_objects`` filters by size without leaving the device; ``euler_number``, ``betti_numbers`` and
``betti_error`` are the Euler characteristic, the Betti numbers (pieces, loops, cavities) and the Betti error of two masks, whole or
averaged over non-overlapping patches.  Masks are numpy arrays or CUDA tensors of any dtype (non-zero = foreground), C-contiguous
``(n0, n1, n2)`` with fewer than 2^31 voxels.  ``connectivity`` 1, 2, 3 = 6, 18, 26 neighbours, scipy's
``generate_binary_structure(3, connectivity)``.  Integer work only: every result is exact and the same on every run.  There is no
CPU path."""
import dataclasses
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._volume import out as _out, upload_mask, workspace


@dataclasses.dataclass(frozen=True)
class ComponentTable:
    """Per component ``k + 1`` of a ``label`` call: ``size[k]`` voxels (int64), ``first[k]`` the linear index of its first voxel
    in raster order (int64), ``box[k]`` = ``(min0, max0, min1, max1, min2, max2)`` of its voxels' coordinates, maxima inclusive
    (int32).  numpy arrays for a numpy mask, CUDA tensors for a tensor."""
    size: object
    first: object
    box: object


@dataclasses.dataclass(frozen=True)
class BettiError:
    """What ``betti_error`` returns.  ``tiles``: tiles per axis.  ``pred`` / ``label``: int32 ``[T, 3]`` device tables of
    ``(b0, b1, b2)`` per tile in raster tile order.  ``error``: float64 ``[3]``, the mean over the tiles of ``|pred - label|``;
    ``total_error``: its sum.  ``whole``: ``(pred triple, label triple)`` of the whole volume, or None."""
    tiles: Tuple[int, int, int]
    pred: torch.Tensor
    label: torch.Tensor
    error: np.ndarray
    total_error: float
    whole: Optional[Tuple[Tuple[int, int, int], Tuple[int, int, int]]]


def mean_abs_error(pred_table: np.ndarray, label_table: np.ndarray) -> np.ndarray:
    """float64 ``[3]``: the mean over the tiles of ``|pred - label|`` of two integer ``[T, 3]`` tables (tests/betti_oracle.py forms its
    expectation with this same expression)."""
    return np.abs(pred_table.astype(np.int64) - label_table.astype(np.int64)).mean(axis=0, dtype=np.float64)


def _mask(a, what):
    """(uint8 CUDA tensor of a 3-D mask, came-as-numpy)."""
    if isinstance(a, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError(f"seunet {what}: needs a GPU (no CPU path)")
        t, as_numpy = upload_mask(a), True
    elif isinstance(a, torch.Tensor) and a.is_cuda:
        t, as_numpy = (a != 0).to(torch.uint8).contiguous(), False
    else:
        raise RuntimeError(f"seunet {what}: needs a CUDA tensor or a numpy array (no CPU path)")
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"seunet {what}: expects a non-empty 3-D volume, got shape {tuple(t.shape)}")
    return t, as_numpy


def _connectivity(connectivity, what, allowed):
    c = int(connectivity)
    if c != connectivity or c not in allowed:
        raise ValueError(f"seunet {what}: `connectivity` must be one of {allowed}, got {connectivity!r}")
    return c


def _patch(patch, shape, what):
    """None, an int or a 3-tuple -> three ints clamped to the extents."""
    if patch is None:
        return tuple(int(v) for v in shape)
    p = (patch,) * 3 if isinstance(patch, (int, np.integer)) else tuple(patch)
    if len(p) != 3 or any(int(v) != v or int(v) < 1 for v in p):
        raise ValueError(f"seunet {what}: `patch` must be None, a positive int or three positive ints, got {patch!r}")
    return tuple(min(int(v), int(n)) for v, n in zip(p, shape))


def _tiles(shape, patch):
    return tuple(-(-int(n) // p) for n, p in zip(shape, patch))


def label(mask, connectivity: int = 3, return_num=False, return_table: bool = False):
    """``scipy.ndimage.label(mask, generate_binary_structure(3, connectivity))`` bit for bit: an int32 volume with 0 on the
    background and the components numbered ``1..N`` in raster order of each component's first voxel.  numpy in -> numpy out, CUDA
    tensor in -> CUDA tensor out.

    ``return_num``: also ``N`` -- a 0-d int32 device tensor that no one has waited for (tensor in), or a Python int (numpy in, or
    ``return_num="int"``).  ``return_table``: also a ``ComponentTable``, for any ``N``; the host reads ``N`` once to size it.
    Returns ``labels``, then ``N`` and the table where asked for, as a tuple."""
    c = _connectivity(connectivity, "label", (1, 2, 3))
    t, as_numpy = _mask(mask, "label")
    lib = _lib.load()
    n0, n1, n2 = (int(v) for v in t.shape)
    dev = t.device
    with torch.cuda.device(dev):
        ws = workspace(lib.seunet_label_workspace_bytes, n0, n1, n2, device=dev, what="seunet label")
        labels = torch.empty((n0, n1, n2), dtype=torch.int32, device=dev)
        num = torch.empty((), dtype=torch.int32, device=dev)
        _lib.check(lib.seunet_label(t.data_ptr(), n0, n1, n2, c, labels.data_ptr(), num.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _lib.stream_ptr()), "label")
        res = [_out(labels, as_numpy)]
        want_int = as_numpy or return_num == "int" or return_table
        n = int(num.item()) if (return_num or return_table) and want_int else None
        if return_num:
            res.append(n if want_int else num)
        if return_table:
            size = torch.empty(n, dtype=torch.int64, device=dev)
            first = torch.empty(n, dtype=torch.int64, device=dev)
            box = torch.empty((n, 6), dtype=torch.int32, device=dev)
            if n > 0:
                _lib.check(lib.seunet_component_table(labels.data_ptr(), n0, n1, n2, n, size.data_ptr(), first.data_ptr(), box.data_ptr(),
                                                      ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "component_table")
            res.append(ComponentTable(_out(size, as_numpy), _out(first, as_numpy), _out(box, as_numpy)))
    return res[0] if len(res) == 1 else tuple(res)


def remove_small_objects(mask, min_size: int, connectivity: int = 3):
    """The uint8 mask of the components of ``mask`` with at least ``min_size`` voxels (``skimage.morphology.remove_small_objects``
    on a binary volume).  Labelling, counting and filtering run back to back on the device; the call does not wait for it.
    numpy in -> numpy out, CUDA tensor in -> CUDA tensor out."""
    c = _connectivity(connectivity, "remove_small_objects", (1, 2, 3))
    if int(min_size) != min_size:
        raise ValueError(f"seunet remove_small_objects: `min_size` must be an integer, got {min_size!r}")
    t, as_numpy = _mask(mask, "remove_small_objects")
    lib = _lib.load()
    n0, n1, n2 = (int(v) for v in t.shape)
    with torch.cuda.device(t.device):
        ws = workspace(lib.seunet_cc_workspace_bytes, n0, n1, n2, device=t.device, what="seunet remove_small_objects")
        out = torch.empty((n0, n1, n2), dtype=torch.uint8, device=t.device)
        _lib.check(lib.seunet_remove_small_objects(t.data_ptr(), n0, n1, n2, int(min_size), c, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   _lib.stream_ptr()), "remove_small_objects")
        return _out(out, as_numpy)


def _euler_tiles(t, patch, c):
    """int64 device vector: chi per tile."""
    lib = _lib.load()
    n0, n1, n2 = (int(v) for v in t.shape)
    ws = workspace(lib.seunet_euler_workspace_bytes, n0, n1, n2, *patch, device=t.device, what="seunet euler_number")
    tiles = _tiles(t.shape, patch)
    chi = torch.empty(tiles[0] * tiles[1] * tiles[2], dtype=torch.int64, device=t.device)
    _lib.check(lib.seunet_euler(t.data_ptr(), n0, n1, n2, *patch, c, chi.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "euler")
    return chi


def _betti_tiles(t, patch, c):
    """int32 device table [T, 3]: (b0, b1, b2) per tile."""
    lib = _lib.load()
    n0, n1, n2 = (int(v) for v in t.shape)
    ws = workspace(lib.seunet_betti_workspace_bytes, n0, n1, n2, *patch, device=t.device, what="seunet betti_numbers")
    tiles = _tiles(t.shape, patch)
    table = torch.empty((tiles[0] * tiles[1] * tiles[2], 3), dtype=torch.int32, device=t.device)
    _lib.check(lib.seunet_betti(t.data_ptr(), n0, n1, n2, *patch, c, table.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "betti")
    return table


def euler_number(mask, connectivity: int = 3) -> int:
    """The Euler characteristic of the foreground as a Python int.  ``connectivity=3``: of the union of the closed unit cubes of
    the voxels (vertices - edges + faces - cubes of the lattice cells a voxel touches); ``connectivity=1``: of the complex whose
    vertices are the voxels (voxels - face-adjacent pairs + 2x2 squares - 2x2x2 cubes, all foreground).  A ball gives 1, a
    solid torus 0, a hollow shell 2.  The call waits for the current stream only."""
    c = _connectivity(connectivity, "euler_number", (1, 3))
    t, _ = _mask(mask, "euler_number")
    with torch.cuda.device(t.device):
        return int(_euler_tiles(t, _patch(None, t.shape, "euler_number"), c).item())


def betti_numbers(mask, connectivity: int = 3) -> Tuple[int, int, int]:
    """``(b0, b1, b2)`` as Python ints: the connected components at ``connectivity`` (3 or 1), the loops, and the cavities -- the
    components of the complement at the dual connectivity (3 <-> 1) that do not reach the border of the volume;
    ``b1 = b0 + b2 - euler_number``.  An intact airway tree is (1, 0, 0).  The call waits for the current stream only."""
    c = _connectivity(connectivity, "betti_numbers", (1, 3))
    t, _ = _mask(mask, "betti_numbers")
    with torch.cuda.device(t.device):
        b = _betti_tiles(t, _patch(None, t.shape, "betti_numbers"), c).cpu().numpy()
    return int(b[0, 0]), int(b[0, 1]), int(b[0, 2])


def betti_error(pred, label, patch=None, connectivity: int = 3, whole: bool = False) -> BettiError:
    """The Betti error of a prediction against a label: ``|b(pred) - b(label)|`` per Betti number, averaged over the tiles of
    ``patch`` -- ``None`` (the whole volume), an int or three ints; non-overlapping tiles from the origin, the last one of an axis
    ragged.  A tile's numbers are exactly ``betti_numbers(mask[tile])``.  All tiles of a mask are done by one fixed set of launches;
    the host waits once, for the two integer tables.  ``whole``: also the whole-volume triples of both masks."""
    c = _connectivity(connectivity, "betti_error", (1, 3))
    tp, _ = _mask(pred, "betti_error")
    tl, _ = _mask(label, "betti_error")
    if tp.shape != tl.shape or tp.device != tl.device:
        raise ValueError(f"seunet betti_error: the two masks must have one shape and device, got {tuple(tp.shape)} and {tuple(tl.shape)}")
    p = _patch(patch, tp.shape, "betti_error")
    with torch.cuda.device(tp.device):
        tabs = [_betti_tiles(tp, p, c), _betti_tiles(tl, p, c)]
        if whole:
            full = _patch(None, tp.shape, "betti_error")
            tabs += [_betti_tiles(tp, full, c), _betti_tiles(tl, full, c)]
        host = torch.cat(tabs).cpu().numpy()
    T = tabs[0].shape[0]
    error = mean_abs_error(host[:T], host[T:2 * T])
    both = (tuple(int(v) for v in host[2 * T]), tuple(int(v) for v in host[2 * T + 1])) if whole else None
    return BettiError(_tiles(tp.shape, p), tabs[0], tabs[1], error, float(error.sum()), both)
