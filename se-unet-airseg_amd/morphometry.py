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
integer columns and its float64 tangents equal tests/cross_section_oracle.py bit for bit.

``airway_walls`` (csrc/airway_wall.hip) reads the CT again: 64 rays in the section plane of every such point,
one wave per point and one ray per lane, find the wall's inner and outer edge by the full-width-at-half-maximum rule; thickness,
wall area percentage and ``AirwayWalls.pi10`` follow on the host, ``branch_morphometry(..., walls=)`` reduces them per branch.  Its
mask, codes, edges and sums equal tests/airway_wall_oracle.py bit for bit."""
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


def _cross_sections(vol, skel, s, step: float, window: int, same_label: bool, num: int, keep: bool = False):
    """``cross_sections`` for device inputs and parameters that are already checked.  ``keep``: -> (CrossSections, the device
    buffer of its rows: 3 m words of tangents, then 6 m words of table rows; None without a point)."""
    lib = _lib.load()
    cap = int(lib.seunet_label_stats_max_num())
    if not 0 <= num <= cap:
        raise ValueError(f"{_PREFIX}: labels up to {cap} are supported, got num = {num}")
    shape = tuple(int(v) for v in vol.shape)
    m, host, buf = 0, None, None
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
    sections = CrossSections.from_columns(table[:, 0:3].copy(), table[:, 3].copy(), table[:, 4].copy(), tangent, table[:, 5].copy(),
                                          table[:, 6:11].copy(), table[:, 11].copy(), step, num, s, window, same_label)
    return (sections, buf) if keep else sections


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


WALL_RAYS = 64                                               # rays per point, one per lane; bit r of ``mask`` = ray r
WALL_CODES = ("measured", "no boundary", "no peak", "no inner contrast", "another lumen", "no outer contrast", "point not measured")
WALL_COLUMNS = ("wall_sections", "wall_thickness_mean", "wall_thickness_median", "wall_area_percent_mean", "wall_area_percent_median")


def _label_rows(label, valid, num):
    """(rows, labels, start, n): the valid rows with a label in 1..num grouped by label (rows in their given order)."""
    rows = np.flatnonzero(valid & (label >= 1) & (label <= num))
    rows = rows[np.argsort(label[rows], kind="stable")]
    labels, start, n = np.unique(label[rows], return_index=True, return_counts=True)
    return rows, labels, start, n


def _label_medians(values, rows, start, n):
    """The median of ``values[rows]`` per group of ``_label_rows``."""
    v = values[rows]
    group = np.repeat(np.arange(start.size), n)
    v = v[np.lexsort((v, group))]
    return 0.5 * (v[start + (n - 1) // 2] + v[start + n // 2])


@dataclasses.dataclass
class AirwayWalls:
    """One row per row of the ``CrossSections`` it was measured on.  From the device: ``mask`` uint64[m], bit r set when ray r was
    measured; ``rays_valid`` int32[m], its popcount; ``sums`` float64[m, 6], the sums over the measured rays of rho_in, rho_out,
    rho_in^2, rho_out^2, rho_out - rho_in and the peak value; with ``return_rays`` also ``codes`` uint8[m, 64] (``WALL_CODES``) and
    ``edges`` float64[m, 64, 2] = (rho_in, rho_out), the distances of the wall's inner and outer half-maximum crossing from the
    lumen centroid (None otherwise).  ``coord`` and ``label`` are the sections'.  float64 columns derived on the host with
    n = ``rays_valid``, nan where n < ``min_rays``: ``inner_radius = sum rho_in / n``; ``outer_radius``; ``wall_thickness =
    sum (rho_out - rho_in) / n``; ``inner_area = pi sum rho_in^2 / n``; ``outer_area``; ``wall_area = outer_area - inner_area``;
    ``wall_area_percent = 100 wall_area / outer_area``; ``inner_perimeter = 2 pi inner_radius``; ``peak``, the mean peak value;
    ``valid = n >= min_rays``.  Lengths are in the units of ``spacing``."""
    num: int
    spacing: Tuple[float, float, float]
    step: float
    ray_step: float
    n_search: int
    min_contrast: float
    same_label: bool
    min_rays: int
    coord: np.ndarray
    label: np.ndarray
    mask: np.ndarray
    rays_valid: np.ndarray
    sums: np.ndarray
    codes: Optional[np.ndarray]
    edges: Optional[np.ndarray]
    inner_radius: np.ndarray
    outer_radius: np.ndarray
    wall_thickness: np.ndarray
    inner_area: np.ndarray
    outer_area: np.ndarray
    wall_area: np.ndarray
    wall_area_percent: np.ndarray
    inner_perimeter: np.ndarray
    peak: np.ndarray
    valid: np.ndarray

    def __len__(self) -> int:
        return int(self.label.shape[0])

    def to_dict(self) -> dict:
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self)}

    @classmethod
    def from_columns(cls, coord, label, mask, sums, codes=None, edges=None, num: Optional[int] = None,
                     spacing: Sequence[float] = (1.0, 1.0, 1.0), step: float = 0.5, ray_step: Optional[float] = None, n_search: int = 10,
                     min_contrast: float = 100.0, same_label: bool = True, min_rays: int = 32) -> "AirwayWalls":
        """The derived columns from the device's; host only."""
        if int(min_rays) != min_rays or not 1 <= int(min_rays) <= WALL_RAYS:
            raise ValueError(f"{_PREFIX}: min_rays must be an integer in 1..{WALL_RAYS}, got {min_rays!r}")
        label = np.asarray(label, dtype=np.int32).reshape(-1)
        m = label.size
        mask = np.ascontiguousarray(mask, dtype=np.uint64).reshape(m)
        sums = np.asarray(sums, dtype=np.float64).reshape(m, 6)
        n = np.unpackbits(mask.view(np.uint8).reshape(m, 8), axis=1).sum(axis=1).astype(np.int32)
        valid = n >= int(min_rays)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = n.astype(np.float64)
            inner_radius, outer_radius, thickness = sums[:, 0] / c, sums[:, 1] / c, sums[:, 4] / c
            inner_area, outer_area, peak = np.pi * sums[:, 2] / c, np.pi * sums[:, 3] / c, sums[:, 5] / c
            wall_area = outer_area - inner_area
            percent = 100.0 * wall_area / outer_area
            perimeter = 2.0 * np.pi * inner_radius
        cols = [np.where(valid, v, np.nan) for v in (inner_radius, outer_radius, thickness, inner_area, outer_area, wall_area, percent,
                                                     perimeter, peak)]
        return cls(int(label.max()) if num is None and m else int(num or 0), tuple(float(v) for v in spacing), float(step),
                   float(step if ray_step is None else ray_step), int(n_search), float(min_contrast), bool(same_label), int(min_rays),
                   np.asarray(coord, dtype=np.int32).reshape(m, 3), label, mask, n, sums,
                   None if codes is None else np.asarray(codes, dtype=np.uint8).reshape(m, WALL_RAYS),
                   None if edges is None else np.asarray(edges, dtype=np.float64).reshape(m, WALL_RAYS, 2), *cols, valid)

    def per_branch(self, num: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Per label 1..num (row k - 1 = label k) over its ``valid`` rows: ``wall_sections`` int64[num]; ``wall_thickness_mean``,
        ``wall_thickness_median``, ``wall_area_percent_mean``, ``wall_area_percent_median`` float64[num], nan for a label without
        one."""
        num = self.num if num is None else int(num)
        out = {"wall_sections": np.zeros(num, np.int64)}
        for k in WALL_COLUMNS[1:]:
            out[k] = np.full(num, np.nan, np.float64)
        rows, labels, start, n = _label_rows(self.label, self.valid, num)
        if rows.size == 0:
            return out
        at = labels - 1
        out["wall_sections"][at] = n
        out["wall_thickness_mean"][at] = np.add.reduceat(self.wall_thickness[rows], start) / n
        out["wall_thickness_median"][at] = _label_medians(self.wall_thickness, rows, start, n)
        out["wall_area_percent_mean"][at] = np.add.reduceat(self.wall_area_percent[rows], start) / n
        out["wall_area_percent_median"][at] = _label_medians(self.wall_area_percent, rows, start, n)
        return out

    def pi10(self, perimeter_range: Sequence[float] = (6.0, 20.0)) -> Dict[str, float]:
        """Pi10: the square root of the wall area of a hypothetical airway with an inner perimeter of 10 (in the units of
        ``spacing``: millimetres).  The least-squares line of ``sqrt(median wall_area)`` on ``median inner_perimeter`` over the
        branches (labels, over their valid rows) whose median perimeter lies in ``perimeter_range`` (ends included) ->
        ``{"intercept", "slope", "pi10": intercept + 10 slope, "branches"}``; nan with fewer than two branches, or when they all
        have the same perimeter."""
        lo, hi = (float(v) for v in perimeter_range)
        nan = {"intercept": float("nan"), "slope": float("nan"), "pi10": float("nan"), "branches": 0}
        rows, _, start, n = _label_rows(self.label, self.valid, max(self.num, int(self.label.max()) if len(self) else 0))
        if rows.size == 0:
            return nan
        x = _label_medians(self.inner_perimeter, rows, start, n)
        y = np.sqrt(np.maximum(_label_medians(self.wall_area, rows, start, n), 0.0))
        keep = (x >= lo) & (x <= hi) & np.isfinite(y)
        x, y = x[keep], y[keep]
        nan["branches"] = int(x.size)
        if x.size < 2:
            return nan
        dx = x - x.mean()
        sxx = float((dx * dx).sum())
        if sxx == 0.0:
            return nan
        slope = float((dx * (y - y.mean())).sum() / sxx)
        intercept = float(y.mean() - slope * x.mean())
        return {"intercept": intercept, "slope": slope, "pi10": intercept + 10.0 * slope, "branches": int(x.size)}


def _ct_in(ct, vol):
    """The CT argument -> an int16 or float32 CUDA tensor of ``vol``'s shape, used where it lies when it is contiguous."""
    if isinstance(ct, np.ndarray):
        if ct.dtype not in (np.int16, np.float32):
            raise TypeError(f"{_PREFIX}: `ct` has dtype {ct.dtype}; expected int16 or float32")
        ct = torch.from_numpy(np.ascontiguousarray(ct)).to(vol.device)
    if not isinstance(ct, torch.Tensor) or not ct.is_cuda:
        raise RuntimeError(f"{_PREFIX}: `ct` must be a CUDA tensor resident on the GPU (there is no CPU path)")
    if ct.dtype not in (torch.int16, torch.float32):
        raise TypeError(f"{_PREFIX}: `ct` has dtype {ct.dtype}; expected int16 or float32")
    if tuple(ct.shape) != tuple(vol.shape):
        raise ValueError(f"{_PREFIX}: `ct` shape {tuple(ct.shape)} differs from `parsing`'s {tuple(vol.shape)}")
    if ct.device != vol.device:
        raise ValueError(f"{_PREFIX}: `ct` is on {ct.device}, `parsing` on {vol.device}")
    return ct.contiguous()


def wall_search(ray_step: float, max_wall: float) -> int:
    """``n_search``: the smallest integer n with ``n * ray_step >= max_wall``; ValueError outside 1..31."""
    ray_step, max_wall = float(ray_step), float(max_wall)
    if not (np.isfinite(ray_step) and ray_step > 0):
        raise ValueError(f"{_PREFIX}: ray_step must be positive and finite, got {ray_step}")
    if not (np.isfinite(max_wall) and max_wall > 0):
        raise ValueError(f"{_PREFIX}: max_wall must be positive and finite, got {max_wall}")
    ratio = max_wall / ray_step
    if not ratio < 64:
        raise ValueError(f"{_PREFIX}: max_wall / ray_step = {ratio:g}: the wall is searched over 1..31 samples")
    n = int(np.ceil(ratio))
    while n > 0 and (n - 1) * ray_step >= max_wall:
        n -= 1
    while n * ray_step < max_wall:
        n += 1
    if not 1 <= n <= 31:
        raise ValueError(f"{_PREFIX}: max_wall / ray_step = {ratio:g}: the wall is searched over 1..31 samples, got n_search = {n}")
    return n


def airway_walls(ct, parsing, skeleton=None, spacing: Sequence[float] = (1.0, 1.0, 1.0), sections: Optional[CrossSections] = None,
                 ray_step: Optional[float] = None, max_wall: Optional[float] = None, min_contrast: float = 100.0, min_rays: int = 32,
                 return_rays: bool = False) -> AirwayWalls:
    """The airway wall at every centreline point, from the CT: ``AirwayWalls``, one row per row of ``sections``.

    From the centroid of a point's lumen section 64 rays are cast in the section plane; along each the CT is sampled every
    ``ray_step`` (``None``: the sections' step) by trilinear interpolation, and ``parsing`` by nearest voxel.  A ray finds where it
    leaves the lumen, the brightest sample within ``max_wall`` (``None``: ``5 min(spacing)``) of it, and the half-maximum crossings
    on both sides of that peak: the wall's inner and outer edge.  A ray is dropped when it finds no boundary or peak, when either
    side of the peak is less than ``min_contrast`` above the darkest sample on that side (an abutting vessel), or when it meets
    another labelled voxel on the way out (a junction, a neighbouring airway).  A point whose section is empty or cut by the sample
    grid is not measured; a point with fewer than ``min_rays`` measured rays has nan columns.  The exact definition, operation by
    operation, is include/seunet_hip.h and tests/airway_wall_oracle.py.

    ``ct``: int16 or float32, the shape of ``parsing`` (``preprocess_ct``'s ``data_cut``; a constant shift moves an edge by float32 rounding only);
    ``sections``: a ``CrossSections`` of the same volume and ``spacing``, whose rows are uploaded in one copy and whose ``same_label``
    the rays follow; ``None`` computes it from ``skeleton`` with the defaults of ``branch_morphometry(cross_sections=True)`` and uses
    its device buffer where it lies.  One launch for all points and rays, and the call ends in one copy back.  ``return_rays`` adds
    ``codes`` and ``edges``.  CUDA tensors or numpy arrays; the inputs are not modified.  ValueError: mismatched shapes, a bad
    ``spacing``, ``ray_step``, ``max_wall`` (``n_search`` outside 1..31), ``min_contrast`` or ``min_rays``."""
    s = prep.normalize_sampling(spacing, "spacing")
    if sections is not None and not isinstance(sections, CrossSections):
        raise TypeError(f"{_PREFIX}: sections must be None or a CrossSections, got {type(sections).__name__}")
    if sections is None and skeleton is None:
        raise ValueError(f"{_PREFIX}: airway_walls needs `sections` or the skeleton to compute them from")
    mc = float(np.float32(min_contrast))
    if not (np.isfinite(mc) and mc > 0):
        raise ValueError(f"{_PREFIX}: min_contrast must be positive and finite in float32, got {min_contrast}")
    if int(min_rays) != min_rays or not 1 <= int(min_rays) <= WALL_RAYS:
        raise ValueError(f"{_PREFIX}: min_rays must be an integer in 1..{WALL_RAYS}, got {min_rays!r}")
    vol, skel, _, _ = _inputs(parsing, skeleton if sections is None else None, None)
    vox = _ct_in(ct, vol)
    rows = None
    if sections is None:
        num = max(int(vol.max()), 0) if vol.numel() else 0
        sections, rows = _cross_sections(vol, skel, *_section_args(s, None, 4), True, num, keep=True)
    elif tuple(sections.spacing) != s:
        raise ValueError(f"{_PREFIX}: `sections` were measured with spacing {tuple(sections.spacing)}, not {s}")
    dr = sections.step if ray_step is None else float(ray_step)
    n = wall_search(dr, 5.0 * min(s) if max_wall is None else max_wall)
    m = len(sections)
    mask, sums = np.zeros(m, np.uint64), np.zeros((m, 6), np.float64)
    codes = np.zeros((m, WALL_RAYS), np.uint8) if return_rays else None
    edges = np.zeros((m, WALL_RAYS, 2), np.float64) if return_rays else None
    if m:
        if not vol.numel():
            raise ValueError(f"{_PREFIX}: `sections` has {m} rows but the volume is empty")
        lib = _lib.load()
        dev = vol.device
        with torch.cuda.device(dev):
            if rows is None:                                  # the one upload: tangents (3 m words), then table rows (6 m words)
                host = np.empty(9 * m, np.int64)
                host[:3 * m].view(np.float64)[:] = sections.tangent.reshape(-1)
                table = host[3 * m:].view(np.int32).reshape(m, 12)
                table[:, 0:3], table[:, 3], table[:, 4], table[:, 5] = sections.coord, sections.label, sections.support, sections.count
                table[:, 6:11], table[:, 11] = sections.moments, sections.rim
                rows = torch.from_numpy(host).to(dev)
            # one buffer of 8-byte words: mask (m), sums (6 m), then edges (128 m) and codes (8 m) where they are wanted
            buf = torch.empty(7 * m + (136 * m if return_rays else 0), dtype=torch.int64, device=dev)
            base = buf.data_ptr()
            _lib.check(lib.seunet_airway_walls(vox.data_ptr(), 0 if vox.dtype == torch.int16 else 1, vol.data_ptr(),
                                               *(int(v) for v in vol.shape), s[0], s[1], s[2], sections.step, dr, n, mc,
                                               int(sections.same_label), m, rows.data_ptr() + 8 * 3 * m, rows.data_ptr(), base,
                                               base + 8 * m, base + 8 * 135 * m if return_rays else None,
                                               base + 8 * 7 * m if return_rays else None, _lib.stream_ptr()), "airway_walls")
            host = buf.cpu().numpy()                          # the one copy back
        mask = host[:m].view(np.uint64).copy()
        sums = host[m:7 * m].view(np.float64).reshape(m, 6).copy()
        if return_rays:
            edges = host[7 * m:135 * m].view(np.float64).reshape(m, WALL_RAYS, 2).copy()
            codes = host[135 * m:].view(np.uint8).reshape(m, WALL_RAYS).copy()
    return AirwayWalls.from_columns(sections.coord, sections.label, mask, sums, codes, edges, sections.num, s, sections.step, dr, n, mc,
                                    sections.same_label, int(min_rays))


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
    wall_sections: Optional[np.ndarray] = None
    wall_thickness_mean: Optional[np.ndarray] = None
    wall_thickness_median: Optional[np.ndarray] = None
    wall_area_percent_mean: Optional[np.ndarray] = None
    wall_area_percent_median: Optional[np.ndarray] = None

    def to_dict(self) -> dict:
        """Every column by name; the cross-section and airway-wall columns only where they were computed, so the keys without them
        are unchanged."""
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self)
                if f.name not in SECTION_COLUMNS + WALL_COLUMNS or getattr(self, f.name) is not None}

    @classmethod
    def from_stats(cls, stats: Dict[str, np.ndarray], adjacency, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                   wall: Optional[Dict[str, np.ndarray]] = None, sections: Optional["CrossSections"] = None,
                   walls: Optional["AirwayWalls"] = None) -> "BranchTable":
        """The derived columns from the integer tables of ``branch_stats`` and a (num, num) face adjacency; host only.  ``wall``: the
        tables of ``branch_wall_distance`` for the same ``spacing``; the inscribed radii are then ``sqrt((s0^2 sum d0^2 + s1^2 sum d1^2
        + s2^2 sum d2^2) / wall_count)``, ``sqrt(wall_sq_min)`` and ``sqrt(wall_sq_max)``, nan where ``wall_count`` is 0.
        ``sections``: a ``CrossSections`` of the same volume; its ``per_branch`` columns are added (None otherwise).  ``walls``: an
        ``AirwayWalls`` of the same volume, likewise."""
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
                   **(sections.per_branch(num) if sections is not None else {}),
                   **(walls.per_branch(num) if walls is not None else {}))


def branch_morphometry(parsing, skeleton=None, spacing: Sequence[float] = (1.0, 1.0, 1.0), num: Optional[int] = None,
                       sqdist=None, inscribed: str = "voxel", cross_sections=None, walls: Optional[AirwayWalls] = None) -> BranchTable:
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

    ``walls``: an ``AirwayWalls`` of the same volume (``airway_walls``); the table then carries, per label over its valid rows,
    ``wall_sections``, ``wall_thickness_mean`` / ``_median`` and ``wall_area_percent_mean`` / ``_median`` (None by default).

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
    if walls is not None and not isinstance(walls, AirwayWalls):
        raise TypeError(f"{_PREFIX}: walls must be None or an AirwayWalls, got {type(walls).__name__}")
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
    return BranchTable.from_stats(stats, adjacency[1:, 1:], spacing, wall, sections, walls)
