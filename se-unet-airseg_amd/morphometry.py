"""Branch morphometry: the table of numbers per branch that a labelled airway tree is made for.

``branch_stats`` (csrc/morphometry.hip) reduces a ``parsing`` volume, its ``skeleton`` and the integer squared EDT to integer tables
per label in two streaming passes on the GPU, with no launch, pass or synchronise per label; ``branch_tree`` turns the face
adjacency of ``label_adjacency`` into parent / generation on the host; ``branch_morphometry`` joins them into a ``BranchTable`` with
lengths, volumes and radii in float64.  The reference has no such function: the definition is the docstrings here and
include/seunet_hip.h, restated in plain numpy by tests/morphometry_oracle.py, and the integer tables equal that oracle bit for bit.

``branch_wall_distance`` reduces the feature transform of the EDT with voxel spacing over the skeleton in one
more streaming pass: the distance from the centreline to the wall per branch as a length, which ``branch_morphometry(...,
inscribed="physical")`` puts into the table; its tables equal tests/wall_distance_oracle.py bit for bit.

``cross_sections`` (csrc/cross_section.hip) measures the lumen section perpendicular to the centreline at every
labelled skeleton voxel, one wave per point: its sample count, five integer moments and the samples on the grid's rim, from which
area and major / minor diameter follow on the host; ``branch_morphometry(..., cross_sections=True)`` reduces them per branch.  Its
integer columns and its float64 tangents equal tests/cross_section_oracle.py bit for bit."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, prep

_PREFIX = "seunet morphometry"

# the 13 link classes: the offsets of {-1, 0, 1}^3 lexicographically above (0, 0, 0), ascending
LINK_OFFSETS = tuple((d0, d1, d2) for d0 in (-1, 0, 1) for d1 in (-1, 0, 1) for d2 in (-1, 0, 1) if (d0, d1, d2) > (0, 0, 0))

# the integer tables of seunet_branch_stats: name -> (dtype, columns); device layout: all int64 tables, then all int32 tables
_TABLES = (("voxels", np.int64, 1), ("coord_sum", np.int64, 3), ("skeleton_voxels", np.int64, 1), ("links", np.int64, 13),
           ("cross_links", np.int64, 13), ("r2_sum", np.int64, 1), ("box_min", np.int32, 3), ("box_max", np.int32, 3),
           ("r2_min", np.int32, 1), ("r2_max", np.int32, 1))
_ARG_ORDER = ("voxels", "coord_sum", "box_min", "box_max", "skeleton_voxels", "links", "cross_links", "r2_sum", "r2_min", "r2_max")
INT32_MAX = int(np.iinfo(np.int32).max)


def _sqdist_in(a, name):
    if isinstance(a, np.ndarray):
        if a.ndim != 3:
            raise ValueError(f"{_PREFIX}: `{name}` must be (n0, n1, n2), got {tuple(a.shape)}")
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    if not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise RuntimeError(f"{_PREFIX}: `{name}` must be a CUDA tensor resident on the GPU (there is no CPU path)")
    if a.dim() != 3:
        raise ValueError(f"{_PREFIX}: `{name}` must be (n0, n1, n2), got {tuple(a.shape)}")
    if a.dtype != torch.int32:
        raise TypeError(f"{_PREFIX}: `{name}` has dtype {a.dtype}; expected the int32 squared distance "
                        "(distance_transform_edt(..., return_sqdist=True))")
    return a.contiguous()


def _empty_tables(num: int, shape) -> Dict[str, np.ndarray]:
    out = {}
    for name, dtype, cols in _TABLES:
        out[name] = np.zeros((num, cols) if cols > 1 else (num,), dtype=dtype)
    out["box_min"][:] = np.asarray(shape, dtype=np.int32)
    out["box_max"][:] = -1
    out["r2_min"][:] = INT32_MAX
    out["r2_max"][:] = -1
    return out


def _branch_stats(vol, skel, sq, num: int) -> Dict[str, np.ndarray]:
    """The tables of ``branch_stats`` for device inputs that are already checked, rows 1..num."""
    lib = _lib.load()
    cap = int(lib.seunet_label_stats_max_num())
    if not 0 <= num <= cap:
        raise ValueError(f"{_PREFIX}: labels up to {cap} are supported, got num = {num}")
    shape = tuple(int(v) for v in vol.shape)
    if vol.numel() == 0:
        return _empty_tables(num, shape)
    rows = num + 1
    dev = vol.device
    with torch.cuda.device(dev):
        # one buffer of 8-byte words: the int64 tables, the int32 tables (two values per word), the status word
        at, words = {}, 0
        for name, dtype, cols in _TABLES:
            at[name] = words
            words += (rows * cols * np.dtype(dtype).itemsize + 7) // 8
        buf = torch.empty(words + 1, dtype=torch.int64, device=dev)
        base = buf.data_ptr()
        _lib.check(lib.seunet_branch_stats(vol.data_ptr(), skel.data_ptr(), _lib.ptr(sq), *shape, num,
                                           *(base + 8 * at[name] for name in _ARG_ORDER), base + 8 * words, _lib.stream_ptr()),
                   "branch_stats")
        host = buf.cpu().numpy()                             # the one copy back; it carries the status
    if int(host[words:].view(np.int32)[0]) != 0:
        raise ValueError(f"{_PREFIX}: the volume holds a label outside 0..{num}")
    out = {}
    for name, dtype, cols in _TABLES:
        t = host[at[name]:].view(dtype)[:rows * cols]
        out[name] = (t.reshape(rows, cols) if cols > 1 else t)[1:].copy()
    return out


def _inputs(parsing, skeleton, sqdist):
    vol, as_numpy = prep._labels_in(parsing, "parsing")
    skel = None
    if skeleton is not None:
        skel, _ = prep._mask_in(skeleton, "skeleton")
        prep._same(vol, skel, "parsing", "skeleton")
    sq = None
    if sqdist is not None:
        sq = _sqdist_in(sqdist, "sqdist")
        prep._same(vol, sq, "parsing", "sqdist")
    return vol, skel, sq, as_numpy


def branch_stats(parsing, skeleton, num: Optional[int] = None, sqdist=None) -> Dict[str, np.ndarray]:
    """The integer tables of ``seunet_branch_stats`` as a dict of numpy arrays with one row per label 1..num (row k - 1 = label k):

    ``voxels`` int64[num]; ``coord_sum`` int64[num, 3], the sums of i0, i1, i2; ``box_min`` / ``box_max`` int32[num, 3], the inclusive
    bounding box (a label without voxels: the volume's shape / -1); ``skeleton_voxels`` int64[num], the voxels with ``skeleton != 0``
    and that label; ``links`` int64[num, 13], links between two skeleton voxels of the label by offset class (``LINK_OFFSETS``);
    ``cross_links`` int64[num, 13], links to a skeleton voxel of another label >= 1, counted in both labels' rows; ``r2_sum`` int64[num],
    ``r2_min`` / ``r2_max`` int32[num], sum, minimum and maximum of ``sqdist`` over the label's skeleton voxels (none, or
    ``sqdist=None``: 0, INT32_MAX, -1).

    A link joins two skeleton voxels with labels in 1..num whose offset d is one of the 13 classes, unless a voxel p + (a proper
    non-empty part of d's non-zero components) is such a skeleton voxel too: the diagonal across an L-shaped corner is not counted.

    ``parsing``: integer labels 0..num; ``skeleton``: 0/1 mask; ``sqdist``: int32, ``distance_transform_edt(..., return_sqdist=True)``.
    CUDA tensors or numpy arrays; the inputs are not modified.  ``num=None`` takes ``int(parsing.max())``, which reads the device
    once more; otherwise the call ends in one copy back that carries the status, with no synchronise before it.  ValueError: a label
    outside 0..num, ``num`` above 4095, mismatched shapes."""
    vol, skel, sq, _ = _inputs(parsing, skeleton, sqdist)
    if skel is None:
        raise ValueError(f"{_PREFIX}: branch_stats needs the skeleton")
    if num is None:
        num = max(int(vol.max()), 0) if vol.numel() else 0
    return _branch_stats(vol, skel, sq, int(num))


WALL_TABLES = ("wall_count", "offset_sq_sum", "wall_sq_min", "wall_sq_max")


def _indices_in(a, vol, name="indices"):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(vol.device)
    if not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise RuntimeError(f"{_PREFIX}: `{name}` must be a CUDA tensor resident on the GPU (there is no CPU path)")
    if a.dtype != torch.int32:
        raise TypeError(f"{_PREFIX}: `{name}` has dtype {a.dtype}; expected the int32 indices of "
                        "distance_transform_edt(..., return_indices=True, sampling=spacing)")
    if tuple(a.shape) != (3,) + tuple(vol.shape):
        raise ValueError(f"{_PREFIX}: `{name}` shape {tuple(a.shape)} is not (3,) + `parsing`'s {tuple(vol.shape)}")
    if a.device != vol.device:
        raise ValueError(f"{_PREFIX}: `{name}` is on {a.device}, `parsing` on {vol.device}")
    return a.contiguous()


def _empty_wall(num: int) -> Dict[str, np.ndarray]:
    return {"wall_count": np.zeros(num, np.int64), "offset_sq_sum": np.zeros((num, 3), np.int64),
            "wall_sq_min": np.full(num, np.inf, np.float64), "wall_sq_max": np.zeros(num, np.float64)}


def _branch_wall(vol, skel, ind, s, num: int) -> Dict[str, np.ndarray]:
    """The tables of ``branch_wall_distance`` for device inputs that are already checked, rows 1..num."""
    lib = _lib.load()
    cap = int(lib.seunet_label_stats_max_num())
    if not 0 <= num <= cap:
        raise ValueError(f"{_PREFIX}: labels up to {cap} are supported, got num = {num}")
    if vol.numel() == 0:
        return _empty_wall(num)
    rows = num + 1
    dev = vol.device
    with torch.cuda.device(dev):
        # one buffer of 8-byte words: wall_count, offset_sq_sum (3 per row), wall_sq_min, wall_sq_max, the status word
        buf = torch.empty(6 * rows + 1, dtype=torch.int64, device=dev)
        base = buf.data_ptr()
        _lib.check(lib.seunet_branch_wall_stats(vol.data_ptr(), skel.data_ptr(), ind.data_ptr(), *(int(v) for v in vol.shape), num,
                                                s[0], s[1], s[2], base, base + 8 * rows, base + 8 * 4 * rows, base + 8 * 5 * rows,
                                                base + 8 * 6 * rows, _lib.stream_ptr()), "branch_wall_stats")
        host = buf.cpu().numpy()                             # the one copy back; it carries the status
    if int(host[6 * rows:].view(np.int32)[0]) != 0:
        raise ValueError(f"{_PREFIX}: the volume holds a label outside 0..{num}")
    return {"wall_count": host[1:rows].copy(), "offset_sq_sum": host[rows:4 * rows].reshape(rows, 3)[1:].copy(),
            "wall_sq_min": host[4 * rows:5 * rows].view(np.float64)[1:].copy(),
            "wall_sq_max": host[5 * rows:6 * rows].view(np.float64)[1:].copy()}


def branch_wall_distance(parsing, skeleton, spacing, num: Optional[int] = None, indices=None) -> Dict[str, np.ndarray]:
    """The distance from the centreline to the wall per branch under the voxel ``spacing`` (a positive number or three of them), as a
    dict of numpy arrays with one row per label 1..num, over the label's skeleton voxels that have a feature in ``indices``:

    ``wall_count`` int64[num], their number; ``offset_sq_sum`` int64[num, 3], the exact sums of ``(index_a - coordinate_a)**2`` per
    axis; ``wall_sq_min`` / ``wall_sq_max`` float64[num], minimum and maximum of ``(dt_0**2 + dt_1**2) + dt_2**2`` with
    ``dt_a = float64(index_a - coordinate_a) * spacing[a]``, which is the square of ``distance_transform_edt(..., sampling=spacing)``
    there before the root (none: +inf and 0.0).  All four are deterministic and equal tests/wall_distance_oracle.py bit for bit.

    ``indices``: int32 (3, n0, n1, n2), ``distance_transform_edt(mask, return_indices=True, sampling=spacing)``; None computes it
    for ``parsing != 0`` (a volume without a background voxel has none: ValueError).  One streaming pass over ``skeleton``
    (``seunet_branch_wall_stats``) and one copy back that carries the status; ``parsing`` is read at skeleton voxels only, so a
    label outside 0..num is a ValueError when a skeleton voxel carries it.  ``num=None``: ``int(parsing.max())``.  CUDA tensors or
    numpy arrays; the inputs are not modified."""
    s = prep.normalize_sampling(spacing, "spacing")
    vol, skel, _, _ = _inputs(parsing, skeleton, None)
    if skel is None:
        raise ValueError(f"{_PREFIX}: branch_wall_distance needs the skeleton")
    if num is None:
        num = max(int(vol.max()), 0) if vol.numel() else 0
    num = int(num)
    if indices is not None:
        ind = _indices_in(indices, vol)
    elif vol.numel():
        _, ind, _ = prep._edt_sampling((vol != 0).to(torch.uint8), s, False, True)
    else:
        ind = None
    return _branch_wall(vol, skel, ind, s, num)


SECTION_HALF = 31                                            # the sample plane is 63 x 63: columns and rows -31 .. 31
SECTION_COLUMNS = ("section_count", "area_mean", "area_min", "area_max", "area_median", "diameter_major_mean", "diameter_minor_mean")


@dataclasses.dataclass
class CrossSections:
    """One row per labelled skeleton voxel (``skeleton != 0``, ``1 <= parsing <= num``) in raster order.  Integer columns, from the
    device: ``coord`` int32[m, 3]; ``label`` int32[m]; ``support`` int32[m], the same-label skeleton voxels in the tangent window;
    ``count`` int32[m], the samples in the section; ``moments`` int32[m, 5], the sums of i, j, i^2, j^2 and ij over the section's
    samples (column i, row j in -31 .. 31); ``rim`` int32[m], the section's samples on the outermost ring of the grid (> 0: the
    section is cut off by the grid).  ``tangent`` float64[m, 3]: the unit tangent, zeros where it is invalid (then ``count`` is 0).
    float64 columns derived on the host: ``area = count * step^2``; ``diameter_major`` / ``diameter_minor = 4 step sqrt(lambda)``
    with lambda the larger / smaller eigenvalue of the samples' 2 x 2 covariance, 1/12 added on its diagonal so that a sample
    stands for a step x step square (the diameters of the ellipse with those second moments; nan where ``count`` is 0);
    ``valid = (count > 0) & (rim == 0)``.  Lengths are in the units of ``spacing``."""
    num: int
    spacing: Tuple[float, float, float]
    step: float
    window: int
    same_label: bool
    coord: np.ndarray
    label: np.ndarray
    support: np.ndarray
    tangent: np.ndarray
    count: np.ndarray
    moments: np.ndarray
    rim: np.ndarray
    area: np.ndarray
    diameter_major: np.ndarray
    diameter_minor: np.ndarray
    valid: np.ndarray

    def __len__(self) -> int:
        return int(self.label.shape[0])

    def to_dict(self) -> dict:
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self)}

    @classmethod
    def from_columns(cls, coord, label, support, tangent, count, moments, rim, step: float, num: Optional[int] = None,
                     spacing: Sequence[float] = (1.0, 1.0, 1.0), window: int = 4, same_label: bool = True) -> "CrossSections":
        """The derived columns from the integer ones; host only."""
        step = float(step)
        if not (np.isfinite(step) and step > 0):
            raise ValueError(f"{_PREFIX}: step must be positive and finite, got {step}")
        label = np.asarray(label, dtype=np.int32).reshape(-1)
        m = label.size
        count = np.asarray(count, dtype=np.int32).reshape(m)
        moments = np.asarray(moments, dtype=np.int32).reshape(m, 5)
        rim = np.asarray(rim, dtype=np.int32).reshape(m)
        c = count.astype(np.float64)
        mo = moments.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean_i, mean_j = mo[:, 0] / c, mo[:, 1] / c
            var_i = mo[:, 2] / c - mean_i * mean_i + 1.0 / 12.0
            var_j = mo[:, 3] / c - mean_j * mean_j + 1.0 / 12.0
            cov = mo[:, 4] / c - mean_i * mean_j
            mid = 0.5 * (var_i + var_j)
            rad = np.sqrt(0.25 * (var_i - var_j) * (var_i - var_j) + cov * cov)
            major = 4.0 * step * np.sqrt(mid + rad)
            minor = 4.0 * step * np.sqrt(np.maximum(mid - rad, 0.0))
        empty = count <= 0
        return cls(num=int(label.max()) if num is None and m else int(num or 0), spacing=tuple(float(v) for v in spacing), step=step,
                   window=int(window), same_label=bool(same_label), coord=np.asarray(coord, dtype=np.int32).reshape(m, 3), label=label,
                   support=np.asarray(support, dtype=np.int32).reshape(m), tangent=np.asarray(tangent, dtype=np.float64).reshape(m, 3),
                   count=count, moments=moments, rim=rim, area=c * (step * step), diameter_major=np.where(empty, np.nan, major),
                   diameter_minor=np.where(empty, np.nan, minor), valid=(count > 0) & (rim == 0))

    def per_branch(self, num: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Per label 1..num (row k - 1 = label k) over its ``valid`` rows: ``section_count`` int64[num]; ``area_mean``, ``area_min``,
        ``area_max``, ``area_median``, ``diameter_major_mean``, ``diameter_minor_mean`` float64[num], nan for a label without one."""
        num = self.num if num is None else int(num)
        out = {"section_count": np.zeros(num, np.int64)}
        for k in SECTION_COLUMNS[1:]:
            out[k] = np.full(num, np.nan, np.float64)
        rows = np.flatnonzero(self.valid & (self.label >= 1) & (self.label <= num))
        if rows.size == 0:
            return out
        rows = rows[np.lexsort((self.area[rows], self.label[rows]))]       # by label, a label's rows by area
        labels, start, n = np.unique(self.label[rows], return_index=True, return_counts=True)
        at = labels - 1
        area = self.area[rows]
        out["section_count"][at] = n
        out["area_mean"][at] = np.add.reduceat(area, start) / n
        out["area_min"][at] = area[start]
        out["area_max"][at] = area[start + n - 1]
        out["area_median"][at] = 0.5 * (area[start + (n - 1) // 2] + area[start + n // 2])
        out["diameter_major_mean"][at] = np.add.reduceat(self.diameter_major[rows], start) / n
        out["diameter_minor_mean"][at] = np.add.reduceat(self.diameter_minor[rows], start) / n
        return out


def _cross_sections(vol, skel, s, step: float, window: int, same_label: bool, num: int) -> CrossSections:
    """``cross_sections`` for device inputs and parameters that are already checked."""
    lib = _lib.load()
    cap = int(lib.seunet_label_stats_max_num())
    if not 0 <= num <= cap:
        raise ValueError(f"{_PREFIX}: labels up to {cap} are supported, got num = {num}")
    shape = tuple(int(v) for v in vol.shape)
    m, host = 0, None
    if vol.numel():
        dev = vol.device
        with torch.cuda.device(dev):
            ws_bytes = int(lib.seunet_cross_section_workspace_bytes(*shape))
            if ws_bytes == 0:
                raise ValueError(f"{_PREFIX}: {_lib.last_error()}")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            n_points, status = C.c_longlong(0), C.c_int(0)
            _lib.check(lib.seunet_cross_section_count(vol.data_ptr(), skel.data_ptr(), *shape, num, C.byref(n_points), C.byref(status),
                                                      ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "cross_section_count")
            if status.value != 0:
                raise ValueError(f"{_PREFIX}: the volume holds a label outside 0..{num}")
            m = int(n_points.value)                           # the one host read that sizes the outputs
            if m:
                # one buffer of 8-byte words: tangent (3 per point), table (12 int32 per point), lin (one int32 per point)
                buf = torch.empty(3 * m + 6 * m + (m + 1) // 2, dtype=torch.int64, device=dev)
                base = buf.data_ptr()
                _lib.check(lib.seunet_cross_section_emit(vol.data_ptr(), skel.data_ptr(), *shape, s[0], s[1], s[2], step, window,
                                                         int(same_label), m, base + 8 * 9 * m, base, base + 8 * 3 * m, ws.data_ptr(),
                                                         ws_bytes, _lib.stream_ptr()), "cross_section_emit")
                host = buf.cpu().numpy()                         # the one copy back
    if m == 0:
        tangent, table = np.zeros((0, 3), np.float64), np.zeros((0, 12), np.int32)
    else:
        tangent = host[:3 * m].view(np.float64).reshape(m, 3).copy()
        table = host[3 * m:9 * m].view(np.int32).reshape(m, 12)
    return CrossSections.from_columns(table[:, 0:3].copy(), table[:, 3].copy(), table[:, 4].copy(), tangent, table[:, 5].copy(),
                                      table[:, 6:11].copy(), table[:, 11].copy(), step, num, s, window, same_label)


def _section_args(spacing, step, window):
    s = prep.normalize_sampling(spacing, "spacing")
    step = min(s) / 2.0 if step is None else float(step)
    if not (np.isfinite(step) and step > 0):
        raise ValueError(f"{_PREFIX}: step must be positive and finite, got {step}")
    if int(window) != window or not 1 <= int(window) <= 7:
        raise ValueError(f"{_PREFIX}: window must be an integer in 1..7, got {window!r}")
    return s, step, int(window)


def cross_sections(parsing, skeleton, spacing: Sequence[float] = (1.0, 1.0, 1.0), step: Optional[float] = None, window: int = 4,
                   same_label: bool = True, num: Optional[int] = None) -> CrossSections:
    """The lumen cross-section perpendicular to the centreline at every labelled skeleton voxel: ``CrossSections``, one row per point.

    At a point p of label k the tangent is the dominant direction of the physical scatter of the label's skeleton voxels within
    ``window`` voxels (Chebyshev) of p; a plane of 63 x 63 samples of pitch ``step`` (``None``: ``min(spacing) / 2``; in the units
    of ``spacing``) through p perpendicular to it is sampled by nearest voxel; a sample is inside when its voxel carries label k
    (``same_label=False``: any label); the section is the 4-connected set of inside samples that contains p.  A section that
    reaches the outermost ring of the grid is cut off (``rim > 0``, ``valid`` False): choose a larger ``step``.  A point with fewer
    than 3 same-label skeleton voxels in its window has no tangent (``tangent`` 0, ``count`` 0).  The exact definition, operation by
    operation, is include/seunet_hip.h and tests/cross_section_oracle.py.

    ``parsing``: integer labels 0..num; ``skeleton``: 0/1 mask; ``spacing``: a positive number or three; ``window``: 1..7.  CUDA
    tensors or numpy arrays; the inputs are not modified.  One host read of the number of points sizes the outputs and carries the
    label status; after it there is no launch, pass or synchronise per point or per label, and the call ends in one copy back.
    ``num=None`` takes ``int(parsing.max())``, which reads the device once more.  ValueError: a label outside 0..num, ``num`` above
    4095, mismatched shapes, a bad ``spacing``, ``step`` or ``window``."""
    s, step, window = _section_args(spacing, step, window)
    vol, skel, _, _ = _inputs(parsing, skeleton, None)
    if skel is None:
        raise ValueError(f"{_PREFIX}: cross_sections needs the skeleton")
    if num is None:
        num = max(int(vol.max()), 0) if vol.numel() else 0
    return _cross_sections(vol, skel, s, step, window, bool(same_label), int(num))


def branch_tree(counts, adjacency) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The branch tree from the face adjacency, on the host.  ``counts``: voxels of the labels 1..num; ``adjacency``: (num, num),
    non-zero where two labels meet across a face (both as ``label_adjacency`` returns them).  The root is the label with the most
    voxels, the lowest such label on a tie.  Generations go breadth-first by levels, a level in ascending label order; a label's
    parent is the first label to reach it.  -> ``(parent, generation, n_children)``, int32[num] indexed by label - 1: ``parent`` holds
    label values, 0 for the root and -1 for a label that is empty or not reachable from the root; ``generation`` is 0 at the
    root and -1 where ``parent`` is -1."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    num = counts.size
    adj = np.asarray(adjacency).reshape(num, num) != 0
    parent = np.full(num, -1, dtype=np.int32)
    generation = np.full(num, -1, dtype=np.int32)
    n_children = np.zeros(num, dtype=np.int32)
    if num == 0 or counts.max() <= 0:
        return parent, generation, n_children
    root = int(np.argmax(counts))                            # the first of the maxima
    parent[root], generation[root] = 0, 0
    level = [root]
    while level:
        reached = []
        for cur in level:                                    # ascending
            for child in np.flatnonzero(adj[cur] | adj[:, cur]):
                if generation[child] < 0 and counts[child] > 0:
                    parent[child] = cur + 1
                    generation[child] = generation[cur] + 1
                    n_children[cur] += 1
                    reached.append(int(child))
        level = sorted(reached)
    return parent, generation, n_children


def link_lengths(spacing: Sequence[float]) -> np.ndarray:
    """float64[13]: the length of a link of each class under ``spacing``, sqrt(sum_a (d_a s_a)^2)."""
    s = np.asarray(spacing, dtype=np.float64).reshape(3)
    return np.sqrt(((np.asarray(LINK_OFFSETS, dtype=np.float64) * s) ** 2).sum(axis=1))


@dataclasses.dataclass
class BranchTable:
    """One row per label 1..num (index k - 1 = label k).  Integer columns: those of ``branch_stats``.  float64 columns: ``volume``,
    ``centroid`` (num, 3), ``length`` and ``radius_equivalent`` in the units of ``spacing``; ``radius_inscribed_rms`` / ``_min`` /
    ``_max`` in VOXEL units of the unit-sampling EDT, which convert to the units of ``spacing`` by one factor only when the spacing
    is isotropic -- or, where the tables of ``branch_wall_distance`` are given (``wall_count``, ``offset_sq_sum``, ``wall_sq_min``,
    ``wall_sq_max``; None otherwise), in the units of ``spacing`` from the EDT with that spacing.  Tree columns: ``parent`` (label value, 0 root, -1 none), ``generation``, ``n_children``, ``is_leaf``.  Whole tree:
    ``n_branches`` (labels with voxels), ``n_leaves``, ``total_length``, ``max_generation`` (-1 without a root),
    ``branches_per_generation`` (int64[max_generation + 1])."""
    num: int
    spacing: Tuple[float, float, float]
    voxels: np.ndarray
    coord_sum: np.ndarray
    box_min: np.ndarray
    box_max: np.ndarray
    skeleton_voxels: np.ndarray
    links: np.ndarray
    cross_links: np.ndarray
    r2_sum: np.ndarray
    r2_min: np.ndarray
    r2_max: np.ndarray
    volume: np.ndarray
    centroid: np.ndarray
    length: np.ndarray
    radius_equivalent: np.ndarray
    radius_inscribed_rms: np.ndarray
    radius_inscribed_min: np.ndarray
    radius_inscribed_max: np.ndarray
    parent: np.ndarray
    generation: np.ndarray
    n_children: np.ndarray
    is_leaf: np.ndarray
    n_branches: int
    n_leaves: int
    total_length: float
    max_generation: int
    branches_per_generation: np.ndarray
    wall_count: Optional[np.ndarray] = None
    offset_sq_sum: Optional[np.ndarray] = None
    wall_sq_min: Optional[np.ndarray] = None
    wall_sq_max: Optional[np.ndarray] = None
    section_count: Optional[np.ndarray] = None
    area_mean: Optional[np.ndarray] = None
    area_min: Optional[np.ndarray] = None
    area_max: Optional[np.ndarray] = None
    area_median: Optional[np.ndarray] = None
    diameter_major_mean: Optional[np.ndarray] = None
    diameter_minor_mean: Optional[np.ndarray] = None

    def to_dict(self) -> dict:
        """Every column by name; the cross-section columns only where they were computed, so the keys without them are unchanged."""
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self)
                if f.name not in SECTION_COLUMNS or getattr(self, f.name) is not None}

    @classmethod
    def from_stats(cls, stats: Dict[str, np.ndarray], adjacency, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                   wall: Optional[Dict[str, np.ndarray]] = None, sections: Optional["CrossSections"] = None) -> "BranchTable":
        """The derived columns from the integer tables of ``branch_stats`` and a (num, num) face adjacency; host only.  ``wall``: the
        tables of ``branch_wall_distance`` for the same ``spacing``; the inscribed radii are then ``sqrt((s0^2 sum d0^2 + s1^2 sum d1^2
        + s2^2 sum d2^2) / wall_count)``, ``sqrt(wall_sq_min)`` and ``sqrt(wall_sq_max)``, nan where ``wall_count`` is 0.
        ``sections``: a ``CrossSections`` of the same volume; its ``per_branch`` columns are added (None otherwise)."""
        s = np.asarray(spacing, dtype=np.float64).reshape(3)
        if not (np.all(np.isfinite(s)) and np.all(s > 0)):
            raise ValueError(f"{_PREFIX}: spacing must be three positive numbers, got {tuple(spacing)}")
        voxels = np.asarray(stats["voxels"], dtype=np.int64)
        num = int(voxels.size)
        skv = np.asarray(stats["skeleton_voxels"], dtype=np.int64)
        ell = link_lengths(s)
        with np.errstate(divide="ignore", invalid="ignore"):
            volume = voxels.astype(np.float64) * (s[0] * s[1] * s[2])
            centroid = np.where(voxels[:, None] > 0, stats["coord_sum"].astype(np.float64) / voxels[:, None] * s, np.nan)
            length = (stats["links"].astype(np.float64) * ell).sum(axis=1) + 0.5 * (stats["cross_links"].astype(np.float64) * ell).sum(axis=1)
            radius_equivalent = np.where(length > 0, np.sqrt(volume / (np.pi * length)), np.nan)
            measured = (skv > 0) & (np.asarray(stats["r2_max"]) >= 0)        # r2_max stays -1 without sqdist
            rms = np.where(measured, np.sqrt(stats["r2_sum"].astype(np.float64) / skv), np.nan)
            rmin = np.where(measured, np.sqrt(np.where(measured, stats["r2_min"], 0).astype(np.float64)), np.nan)
            rmax = np.where(measured, np.sqrt(np.where(measured, stats["r2_max"], 0).astype(np.float64)), np.nan)
            if wall is not None:
                wall = {k: np.asarray(wall[k]) for k in WALL_TABLES}
                count = wall["wall_count"].astype(np.int64)
                measured = count > 0
                sq = wall["offset_sq_sum"].astype(np.float64)
                rms = np.where(measured, np.sqrt((s[0] * s[0] * sq[:, 0] + s[1] * s[1] * sq[:, 1] + s[2] * s[2] * sq[:, 2]) / count), np.nan)
                rmin = np.where(measured, np.sqrt(np.where(measured, wall["wall_sq_min"], 0.0)), np.nan)
                rmax = np.where(measured, np.sqrt(np.where(measured, wall["wall_sq_max"], 0.0)), np.nan)
        parent, generation, n_children = branch_tree(voxels, adjacency)
        is_leaf = (generation >= 0) & (n_children == 0)
        max_generation = int(generation.max()) if num else -1
        per_generation = np.bincount(generation[generation >= 0], minlength=max_generation + 1).astype(np.int64)
        return cls(num=num, spacing=tuple(float(v) for v in s), **{name: np.asarray(stats[name]) for name, _, _ in _TABLES},
                   volume=volume, centroid=centroid, length=length, radius_equivalent=radius_equivalent, radius_inscribed_rms=rms,
                   radius_inscribed_min=rmin, radius_inscribed_max=rmax, parent=parent, generation=generation, n_children=n_children,
                   is_leaf=is_leaf, n_branches=int((voxels > 0).sum()), n_leaves=int(is_leaf.sum()), total_length=float(length.sum()),
                   max_generation=max_generation, branches_per_generation=per_generation, **(wall or {}),
                   **(sections.per_branch(num) if sections is not None else {}))


def branch_morphometry(parsing, skeleton=None, spacing: Sequence[float] = (1.0, 1.0, 1.0), num: Optional[int] = None,
                       sqdist=None, inscribed: str = "voxel", cross_sections=None) -> BranchTable:
    """The per-branch table of a ``parsing`` volume (``tree_parsing`` or ``airway_parse``): ``BranchTable``.

    ``volume = voxels * s0 s1 s2``; ``centroid = coord_sum / voxels * spacing`` (nan for a label without voxels);
    ``length = sum_c links[:, c] l_c + 1/2 sum_c cross_links[:, c] l_c`` with ``l_c = sqrt(sum_a (d_a s_a)^2)``: the half share of a
    link between two branches closes the gap between them without counting it twice; ``radius_equivalent =
    sqrt(volume / (pi length))``, the radius of the cylinder of that volume and length, correct under anisotropic spacing, nan where
    the length is 0; ``radius_inscribed_rms / _min / _max = sqrt(r2_sum / skeleton_voxels), sqrt(r2_min), sqrt(r2_max)``: the distance
    from the centreline to the wall in VOXEL units of the unit-sampling EDT (nan for a label without skeleton voxels), which is a
    length in the units of ``spacing`` only after multiplying by an isotropic spacing; ``inscribed="physical"`` gives them in the
    units of ``spacing`` under any spacing.  The tree columns come from ``branch_tree`` on the face adjacency of
    ``seunet_label_stats``.

    ``inscribed="physical"``: the three inscribed radii come from ``branch_wall_distance`` on the EDT of ``parsing != 0`` with
    ``sampling=spacing``: ``radius_inscribed_rms = sqrt((s0^2 sum d0^2 + s1^2 sum d1^2 + s2^2 sum d2^2) / wall_count)``, ``_min =
    sqrt(wall_sq_min)``, ``_max = sqrt(wall_sq_max)`` (nan where ``wall_count`` is 0); the table carries ``wall_count``,
    ``offset_sq_sum``, ``wall_sq_min`` and ``wall_sq_max`` (None in voxel mode); ``r2_sum`` / ``r2_min`` / ``r2_max`` keep their
    empty values (0, INT32_MAX, -1), and passing ``sqdist`` is a ValueError.

    ``cross_sections``: a ``CrossSections`` of the same volume, or True to compute one with ``cross_sections(parsing, skeleton,
    spacing, num=num)`` at its defaults; the table then carries, per label over its valid sections, ``section_count``, ``area_mean``,
    ``area_min``, ``area_max``, ``area_median``, ``diameter_major_mean`` and ``diameter_minor_mean`` (nan for a label without a valid
    section; None by default).

    ``skeleton=None`` thins ``parsing != 0`` with ``skeletonize_3d``; ``sqdist=None`` takes the squared EDT of ``parsing != 0`` (a
    volume without a background voxel has none: ValueError).  ``num=None``: ``int(parsing.max())``.  CUDA tensors or numpy arrays in,
    numpy columns out; the inputs are not modified."""
    if inscribed not in ("voxel", "physical"):
        raise ValueError(f"{_PREFIX}: inscribed must be 'voxel' or 'physical', got {inscribed!r}")
    physical = inscribed == "physical"
    if physical and sqdist is not None:
        raise ValueError(f"{_PREFIX}: `sqdist` is the unit-sampling squared distance; it is not used with inscribed='physical'")
    s = prep.normalize_sampling(spacing, "spacing") if physical else None
    if cross_sections is not None and cross_sections is not True and not isinstance(cross_sections, CrossSections):
        raise TypeError(f"{_PREFIX}: cross_sections must be None, True or a CrossSections, got {type(cross_sections).__name__}")
    vol, skel, sq, _ = _inputs(parsing, skeleton, sqdist)
    if num is None:
        num = max(int(vol.max()), 0) if vol.numel() else 0
    num = int(num)
    ind = None
    if skel is None or sq is None:
        mask = (vol != 0).to(torch.uint8)
        if skel is None:
            skel = prep.skeletonize_3d(mask)
        if physical and vol.numel():
            _, ind, _ = prep._edt_sampling(mask, s, False, True)
        elif sq is None and vol.numel():
            sq = prep.distance_transform_edt(mask, return_distances=False, return_sqdist=True)
    stats = _branch_stats(vol, skel, sq, num)
    wall = _branch_wall(vol, skel, ind, s, num) if physical else None
    _, adjacency = prep._label_stats(vol, num)
    sections = cross_sections
    if sections is True:
        sections = _cross_sections(vol, skel, *_section_args(spacing, None, 4), True, num)
    return BranchTable.from_stats(stats, adjacency[1:, 1:], spacing, wall, sections)
