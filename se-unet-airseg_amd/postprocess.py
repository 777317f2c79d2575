"""Prediction post-processing on the GPU: the reference's ``double_threshold_iteration`` and the 15 %
border clearing of prediction.py:111-114.

The reference has three copies of the function.  prediction.py:13-37 keeps ``pred*255`` in float64; train.py:25-49 and
test.py:18-42 (the validation / test loops) round it to float32 first (train.py:31, test.py:24), which moves voxels
within a float32 ulp of a threshold to the other class.  ``pred_dtype`` selects the copy ("float64" = prediction.py,
the default; "float32" = train.py / test.py).

The reference's version is a pure-Python triple loop over every voxel with 26 neighbour look-ups (hours for a 512^3
volume); here it is ``seunet_dti`` (csrc/dti.hip), which reproduces the single raster-order sweep bit for bit.
There is no CPU path."""
import ctypes as C
import dataclasses
from typing import Tuple, Union

import numpy as np
import torch

from . import _lib
from ._volume import out as _out, read_status, upload_mask, workspace


def double_threshold_iteration(pred: Union[np.ndarray, torch.Tensor], h_thresh: float, l_thresh: float,
                               pred_dtype: str = "float64"):
    """Same arguments and meaning as prediction.py:13 (``pred_dtype="float32"``: train.py:25 / test.py:18).
    ``pred``: (h, w, z) probabilities.
    numpy in -> float64 numpy of zeros / ones out (what the reference returns, ``gbin / 255``);
    CUDA tensor in -> uint8 CUDA tensor out (stays on the device)."""
    as_numpy = isinstance(pred, np.ndarray)
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("seunet double_threshold_iteration needs a GPU (no CPU path)")
        t = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float64)).cuda()
    else:
        if not pred.is_cuda:
            raise RuntimeError("seunet double_threshold_iteration needs a CUDA tensor or a numpy array (no CPU path)")
        t = pred.detach().to(torch.float64).contiguous()
    if t.dim() != 3:
        raise ValueError(f"double_threshold_iteration expects a 3-D volume, got shape {tuple(t.shape)}")
    if pred_dtype not in ("float64", "float32"):
        raise ValueError(f"pred_dtype {pred_dtype!r}: 'float64' (prediction.py:19) or 'float32' (train.py:31, test.py:24)")
    code = _lib.DTI_F32 if pred_dtype == "float32" else _lib.DTI_F64
    lib = _lib.load()
    h, w, z = (int(v) for v in t.shape)
    with torch.cuda.device(t.device):
        ws = workspace(lib.seunet_dti_workspace_bytes, h, w, z, device=t.device)
        out = torch.empty((h, w, z), dtype=torch.uint8, device=t.device)
        _lib.check(lib.seunet_dti(t.data_ptr(), h, w, z, float(h_thresh), float(l_thresh), code, out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _lib.stream_ptr()), "dti")
    return out.cpu().numpy().astype(np.float64) if as_numpy else out


def zero_borders(pred, lo: float = 0.15, hi: float = 0.85):
    """prediction.py:111-114: clear the slabs below 15 % and above 85 % of the first two axes (in place; numpy or
    tensor).  The two literals are the reference's own (int(0.15 * n), int(0.85 * n))."""
    a, b = pred.shape[0], pred.shape[1]
    pred[0:int(lo * a), :, :] = 0
    pred[int(hi * a):, :, :] = 0
    pred[:, 0:int(lo * b), :] = 0
    pred[:, int(hi * b):, :] = 0
    return pred


def postprocess_prediction(pred, h_thresh: float = 0.5, l_thresh: float = 0.4):
    """prediction.py:110-114: double threshold (0.5 / 0.4), then border clearing.  ``maximum_3d`` (prediction.py:116)
    is the next step: ``maximum_3d(postprocess_prediction(pred))``."""
    return zero_borders(double_threshold_iteration(pred, h_thresh, l_thresh))


# ----------------------------------------------------------------------------------------------------------------------
# largest 26-connected component (+ hole filling) and the ATM'22 metrics, on the device
# ----------------------------------------------------------------------------------------------------------------------
def _as_u8_cuda(a, name):
    """(uint8 CUDA tensor, came-as-numpy).  Unlike prep's masks a tensor of ANY dtype is taken (non-zero = 1) and the rank is the
    caller's to check, so the policy stays here; only the upload is shared."""
    if isinstance(a, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError(f"seunet {name}: needs a GPU (no CPU path)")
        return upload_mask(a), True
    if not a.is_cuda:
        raise RuntimeError(f"seunet {name}: needs a CUDA tensor or a numpy array (no CPU path)")
    return (a != 0).to(torch.uint8).contiguous(), False


def _largest(vol, rule, name):
    t, as_numpy = _as_u8_cuda(vol, name)
    if t.dim() != 3:
        raise ValueError(f"{name} expects a 3-D volume, got shape {tuple(t.shape)}")
    lib = _lib.load()
    h, w, z = (int(v) for v in t.shape)
    with torch.cuda.device(t.device):
        ws = workspace(lib.seunet_cc_workspace_bytes, h, w, z, device=t.device)
        out = torch.empty((h, w, z), dtype=torch.uint8, device=t.device)
        status = torch.zeros(1, dtype=torch.int32, device=t.device)
        _lib.check(lib.seunet_largest_component(t.data_ptr(), h, w, z, rule, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _lib.stream_ptr()), name)
    return out, read_status(status), as_numpy


def largest_component(pred):
    """The component rule of ``evaluation_case`` (train.py:749-757, test.py:243-251): the 26-connected component with the
    most voxels as a uint8 mask (``large_cd``); an empty prediction gives an empty mask (``pred.astype(np.uint8)``).
    numpy in -> uint8 numpy out; CUDA tensor in -> uint8 CUDA tensor out."""
    out, _, as_numpy = _largest(pred, _lib.CC_EVALUATION, "largest_component")
    return _out(out, as_numpy)


def maximum_3d(region01):
    """util.py:58-75 (called at prediction.py:116): largest 26-connected component, replaced by the second largest when it
    misses the three test slices of the last axis, then ``binary_fill_holes``.  Returns a bool array (numpy in) like the
    reference, or a uint8 CUDA tensor (tensor in).  Raises IndexError where the reference does (no component / no second
    component)."""
    out, status, as_numpy = _largest(region01, _lib.CC_MAXIMUM_3D, "maximum_3d")
    if status != 0:
        raise IndexError("list index out of range (maximum_3d: %s, util.py:%d)" %
                         (("the volume has no foreground component", 65) if status == 1 else ("no second component to fall back to", 71)))
    return out.cpu().numpy().astype(bool) if as_numpy else out


class MetricSums:
    """The integer sums metrics.py:14-78 is built from, computed in one pass on the device (``seunet_metric_sums``)."""

    def __init__(self, pred, label=None, skeleton=None, parsing=None, nbins: int = 4096):
        p, _ = _as_u8_cuda(pred, "metrics")
        lab = _as_u8_cuda(label, "metrics")[0] if label is not None else None
        sk = _as_u8_cuda(skeleton, "metrics")[0] if skeleton is not None else None
        pa = None
        if parsing is not None:
            pa = (torch.from_numpy(np.ascontiguousarray(parsing)).cuda() if isinstance(parsing, np.ndarray) else parsing)
            pa = pa.to(device=p.device, dtype=torch.int32).contiguous()
        for t in (lab, sk, pa):
            if t is not None and t.numel() != p.numel():
                raise ValueError("metrics: all volumes must have the prediction's size")
        lib = _lib.load()
        with torch.cuda.device(p.device):
            nb = lib.seunet_metric_out_bytes(nbins)
            out = torch.empty(nb, dtype=torch.uint8, device=p.device)
            _lib.check(lib.seunet_metric_sums(p.data_ptr(), _lib.ptr(lab), _lib.ptr(sk), _lib.ptr(pa), p.numel(), nbins, out.data_ptr(), nb,
                                              _lib.stream_ptr()), "metric_sums")
        raw = out.cpu().numpy()
        sums = raw[:64].view(np.uint64)
        self.n = p.numel()
        self.inter, self.pred, self.label, self.pred_skel, self.skel = (np.uint64(v) for v in sums[:5])
        self.branch_label = raw[64:64 + 4 * nbins].view(np.uint32).astype(np.int64)
        self.branch_pred = raw[64 + 4 * nbins:64 + 8 * nbins].view(np.uint32).astype(np.int64)
        extra = raw[64 + 8 * nbins:64 + 8 * nbins + 8].view(np.int32)
        self.max_id = int(extra[0])
        if int(extra[1]):
            raise ValueError(f"metrics: a branch id >= nbins ({nbins}) was met; pass a larger nbins")


def branch_detected_calculation(pred, label_parsing, label_skeleton, thresh=0.8, sums: "MetricSums" = None):
    """metrics.py:14-29 -> (total_branch_num, detected_branch_num, detected_branch_ratio), from the per-branch skeleton voxel
    counts the device histogram returns: a branch counts as detected when the prediction covers at least ``thresh`` of its
    skeleton voxels.  The reference divides two bincounts (the predicted one zero-padded to the labelled one's length) and
    compares the ratio with ``thresh``; a branch id without skeleton voxels gives 0/0 = NaN there, which never passes."""
    s = sums or MetricSums(pred, None, label_skeleton, label_parsing)
    n_branches = int(s.max_id)                       # ids 1 .. max_id (np.bincount's length follows the largest id present)
    in_label = np.asarray(s.branch_label[1:n_branches + 1], dtype=np.float64)
    covered = np.zeros(n_branches, dtype=np.float64)
    have = np.asarray(s.branch_pred[1:n_branches + 1], dtype=np.float64)
    covered[:have.shape[0]] = have
    frac = np.divide(covered, in_label, out=np.full(n_branches, -1.0), where=in_label > 0)    # (0/0: a miss, like NaN >= thresh)
    hit = frac >= thresh
    detected = int(np.count_nonzero(hit))
    return n_branches, detected, round(detected * 100 / n_branches, 2)


def dice_coefficient_score_calculation(pred, label, smooth=1e-5, sums: "MetricSums" = None):
    """metrics.py:32-37."""
    s = sums or MetricSums(pred, label)
    return round(((2.0 * s.inter + smooth) / (s.pred + s.label + smooth)) * 100, 2)


def tree_length_calculation(pred, label_skeleton, smooth=1e-5, sums: "MetricSums" = None):
    """metrics.py:40-44."""
    s = sums or MetricSums(pred, None, label_skeleton)
    return round((s.pred_skel + smooth) / (s.skel + smooth) * 100, 2)


def false_positive_rate_calculation(pred, label, smooth=1e-5, sums: "MetricSums" = None):
    """metrics.py:47-52."""
    s = sums or MetricSums(pred, label)
    fp = np.uint64(s.pred - s.inter) + smooth
    return round(fp * 100 / (np.float64(s.n - int(s.label)) + smooth), 3)


def false_negative_rate_calculation(pred, label, smooth=1e-5, sums: "MetricSums" = None):
    """metrics.py:55-60."""
    s = sums or MetricSums(pred, label)
    fn = np.uint64(s.label - s.inter) + smooth
    return round(fn * 100 / (s.label + smooth), 3)


def sensitivity_calculation(pred, label, sums: "MetricSums" = None):
    """metrics.py:63-65."""
    return round(100 - false_negative_rate_calculation(pred, label, sums=sums), 3)


def specificity_calculation(pred, label, sums: "MetricSums" = None):
    """metrics.py:68-70."""
    return round(100 - false_positive_rate_calculation(pred, label, sums=sums), 3)


def precision_calculation(pred, label, smooth=1e-5, sums: "MetricSums" = None):
    """metrics.py:73-78."""
    s = sums or MetricSums(pred, label)
    tp = s.inter + smooth
    return round(tp * 100 / (s.pred + smooth), 3)


def evaluation_case(pred, label, skeleton, parsing, nbins: int = 4096):
    """The arithmetic of ``evaluation_case`` (train.py:740-775, minus its file reads): largest 26-connected component of
    ``pred``, then (TD, BD, DSC, Pre, Sen, Spe) against the mask, the skeleton (``skeleton > 0``) and the branch parsing.
    One labelling pass + one reduction pass on the device; the percentages are rounded on the host like metrics.py."""
    large_cd = largest_component(pred if not isinstance(pred, np.ndarray) else torch.from_numpy(np.ascontiguousarray(pred != 0)).cuda())
    s = MetricSums(large_cd, label, skeleton, parsing, nbins)
    _, _, bd = branch_detected_calculation(None, None, None, sums=s)
    dsc = dice_coefficient_score_calculation(None, None, sums=s)
    td = tree_length_calculation(None, None, sums=s)
    sen = sensitivity_calculation(None, None, sums=s)
    spe = specificity_calculation(None, None, sums=s)
    pre = precision_calculation(None, None, sums=s)
    return td, bd, dsc, pre, sen, spe


def cldice_score(pred_mask, label_mask, pred_skeleton=None, label_skeleton=None, return_parts: bool = False):
    """The hard clDice score (Shit et al., CVPR 2021) of two binary volumes: ``tprec = |S_P and V_L| / |S_P|``, ``tsens = |S_L and
    V_P| / |S_L|``, ``2 tprec tsens / (tprec + tsens)`` in float64.  Missing skeletons come from ``skeletonize_3d``; the four
    counts are exact integers from one counting pass on the device (``seunet_cldice_counts``), read back once.  A ratio whose
    skeleton is empty counts as 0, and so does the score when both ratios are 0 (never nan: tests/cldice_oracle.py says why).
    numpy arrays or CUDA tensors of any dtype (non-zero = 1).  ``return_parts``: ``(score, tprec, tsens, counts)``."""
    from .prep import skeletonize_3d
    vp, _ = _as_u8_cuda(pred_mask, "cldice_score")
    vl, _ = _as_u8_cuda(label_mask, "cldice_score")
    if vp.dim() != 3 or vl.shape != vp.shape:
        raise ValueError(f"cldice_score expects two 3-D volumes of one shape, got {tuple(vp.shape)} and {tuple(vl.shape)}")
    if vp.numel() == 0:
        raise ValueError("cldice_score: empty volume")
    sp = skeletonize_3d(vp) if pred_skeleton is None else _as_u8_cuda(pred_skeleton, "cldice_score")[0]
    sl = skeletonize_3d(vl) if label_skeleton is None else _as_u8_cuda(label_skeleton, "cldice_score")[0]
    for t in (sp, sl):
        if t.shape != vp.shape:
            raise ValueError(f"cldice_score: a skeleton of shape {tuple(t.shape)} for masks of shape {tuple(vp.shape)}")
    with torch.cuda.device(vp.device):
        counts = torch.empty(4, dtype=torch.int64, device=vp.device)
        _lib.check(_lib.load().seunet_cldice_counts(sp.data_ptr(), vl.data_ptr(), sl.data_ptr(), vp.data_ptr(), vp.numel(),
                                                    counts.data_ptr(), _lib.stream_ptr()), "cldice_counts")
    c = [int(v) for v in counts.cpu().tolist()]
    tprec = np.float64(c[0]) / np.float64(c[1]) if c[1] else np.float64(0.0)
    tsens = np.float64(c[2]) / np.float64(c[3]) if c[3] else np.float64(0.0)
    score = float(2.0 * tprec * tsens / (tprec + tsens)) if tprec + tsens != 0 else 0.0
    return (score, float(tprec), float(tsens), tuple(c)) if return_parts else score


# ----------------------------------------------------------------------------------------------------------------------
# Boundary metrics in the units of the voxel spacing: surface distances, order statistics, HD / ASSD / NSD
# ----------------------------------------------------------------------------------------------------------------------
SELECT_MAX_RANKS = 8
SURFACE_MAX_TOLERANCES = 8


@dataclasses.dataclass(frozen=True)
class SurfaceMetrics:
    """What ``surface_metrics`` returns; distances in the units of ``spacing``.  ``hd``: the Hausdorff distance, the largest
    surface distance of either direction.  ``hd_percentile``: the larger of the two directions' ``percentile``-th percentiles;
    ``hd_percentile_pooled``: the percentile of both directions' distances together (MedPy's ``hd95``).  ``asd_ab`` / ``asd_ba``:
    the mean distance from the first mask's surface to the second's and back; ``assd``: the mean over both.  ``nsd``: per
    tolerance, the fraction of all surface voxels within it (surface Dice).  ``n_a`` / ``n_b``: the surface voxels."""
    hd: float
    hd_percentile: float
    hd_percentile_pooled: float
    asd_ab: float
    asd_ba: float
    assd: float
    nsd: Tuple[float, ...]
    n_a: int
    n_b: int


def _surface_masks(a, b, what):
    ta, as_numpy = _as_u8_cuda(a, what)
    tb, _ = _as_u8_cuda(b, what)
    if ta.dim() != 3 or tb.shape != ta.shape:
        raise ValueError(f"{what}: the two masks must be 3-D volumes of one shape, got {tuple(ta.shape)} and {tuple(tb.shape)}")
    if ta.numel() == 0:
        raise ValueError(f"{what}: empty volume")
    if tb.device != ta.device:
        raise ValueError(f"{what}: the two masks are on different devices")
    return ta, tb, as_numpy


def _surface_count(ta, tb):
    """The count call: (n_a, n_b, box, workspace)."""
    lib = _lib.load()
    n0, n1, n2 = (int(v) for v in ta.shape)
    ws = workspace(lib.seunet_surface_workspace_bytes, n0, n1, n2, device=ta.device, what="seunet surface")
    n_a, n_b, box = C.c_longlong(0), C.c_longlong(0), (C.c_int * 6)()
    _lib.check(lib.seunet_surface_count(ta.data_ptr(), tb.data_ptr(), n0, n1, n2, C.byref(n_a), C.byref(n_b), box, ws.data_ptr(),
                                        ws.numel(), _lib.stream_ptr()), "surface_count")
    return int(n_a.value), int(n_b.value), box, ws


def _surface_emit(ta, s, n_a, n_b, box, ws, want_voxels):
    lib = _lib.load()
    n0, n1, n2 = (int(v) for v in ta.shape)
    dev = ta.device
    ews = workspace(lib.seunet_surface_emit_workspace_bytes, box[1] - box[0], box[3] - box[2], box[5] - box[4], device=dev,
                    what="seunet surface")
    dist = torch.empty(n_a + n_b, dtype=torch.float64, device=dev)
    voxels = torch.empty(n_a + n_b, dtype=torch.int32, device=dev) if want_voxels else None
    _lib.check(lib.seunet_surface_emit(n0, n1, n2, box, s[0], s[1], s[2], n_a, n_b, dist.data_ptr(), _lib.ptr(voxels), ws.data_ptr(),
                                       ws.numel(), ews.data_ptr(), ews.numel(), _lib.stream_ptr()), "surface_emit")
    return dist, voxels


def surface_distances(a, b, spacing=(1, 1, 1), return_voxels: bool = False):
    """The surface distances of two masks (numpy arrays or CUDA tensors of any dtype, non-zero = 1, one 3-D shape) under the
    voxel ``spacing`` (a positive number or three): ``(D, n_a, n_b)``.  ``D`` is float64: for each of the ``n_a`` border voxels
    of ``a`` in raster order the distance to the nearest border voxel of ``b``, then the ``n_b`` distances of ``b``'s border
    voxels to ``a``'s.  A border voxel is a set voxel with one of its six neighbours unset or outside the volume; the distances
    are ``scipy.ndimage.distance_transform_edt(~border, sampling=spacing)`` read at the other border, bit for bit
    (tests/surface_oracle.py).  ``return_voxels``: also the int32 linear index in the volume of each of the ``n_a + n_b`` border
    voxels.  numpy in -> numpy out; CUDA tensors in -> CUDA tensors out.  ValueError when a mask has no voxel."""
    from .prep import normalize_sampling
    s = normalize_sampling(spacing, "spacing")
    ta, tb, as_numpy = _surface_masks(a, b, "seunet surface_distances")
    with torch.cuda.device(ta.device):
        n_a, n_b, box, ws = _surface_count(ta, tb)
        if n_a == 0 or n_b == 0:
            raise ValueError(f"seunet surface_distances: a mask without voxels has no surface distances ({n_a} and {n_b} surface voxels)")
        dist, voxels = _surface_emit(ta, s, n_a, n_b, box, ws, return_voxels)
    res = (_out(dist, as_numpy), n_a, n_b)
    return res + (_out(voxels, as_numpy),) if return_voxels else res


def _select_ranks(values, ranks, segments, out):
    """``seunet_select_ranks`` into ``out`` (a float64 device vector of len(ranks))."""
    lib = _lib.load()
    k = len(ranks)
    arr = lambda v: (C.c_longlong * k)(*[int(x) for x in v])
    ws = workspace(lib.seunet_select_ranks_workspace_bytes, k, device=values.device, what="seunet order_statistics")
    _lib.check(lib.seunet_select_ranks(values.data_ptr(), values.numel(), arr([b for b, _ in segments]), arr([e for _, e in segments]),
                                       arr(ranks), k, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "select_ranks")


def order_statistics(values, ranks, segments=None):
    """Exact order statistics on the device.  ``values``: a float64 CUDA vector of FINITE, NON-NEGATIVE numbers (they are ordered by
    their bit patterns; it is not modified).  ``ranks``: up to 8 ints; ``segments``: per rank a ``(begin, end)`` pair (default: all
    of ``values``), which may overlap.  Returns a float64 CUDA vector: entry r is the element of rank ``ranks[r]`` (0 = smallest)
    of ``values[begin_r:end_r]``, the value ``sort`` would put there.  A radix select (csrc/surface.hip): no sort, no host round
    trip, and the call does not wait for the device."""
    if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64 and values.dim() == 1):
        raise ValueError("seunet order_statistics: `values` must be a 1-D float64 CUDA tensor")
    values = values.contiguous()
    n = values.numel()
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= SELECT_MAX_RANKS:
        raise ValueError(f"seunet order_statistics: `ranks` must hold 1 .. {SELECT_MAX_RANKS} ranks, got {len(ranks)}")
    segments = [(0, n)] * len(ranks) if segments is None else [(int(b), int(e)) for b, e in segments]
    if len(segments) != len(ranks):
        raise ValueError(f"seunet order_statistics: {len(segments)} `segments` for {len(ranks)} ranks")
    for r, (b, e) in zip(ranks, segments):
        if not 0 <= b < e <= n:
            raise ValueError(f"seunet order_statistics: `segments`: [{b}, {e}) is empty or outside the {n} values")
        if not 0 <= r < e - b:
            raise ValueError(f"seunet order_statistics: `ranks`: rank {r} outside a segment of {e - b}")
    with torch.cuda.device(values.device):
        out = torch.empty(len(ranks), dtype=torch.float64, device=values.device)
        _select_ranks(values, ranks, segments, out)
    return out


def _percentile_ranks(n: int, q: float):
    """The two ranks and the weight of numpy's default (linear) percentile of ``n`` values: ``(lo, hi, g)`` in numpy's own
    float64 arithmetic (numpy 2.2, ``_quantile``: virtual index ``(n - 1) * (q / 100)``)."""
    vi = np.multiply(np.float64(n - 1), np.true_divide(np.float64(q), np.float64(100)))
    lo = np.floor(vi)
    g = np.subtract(vi, lo)
    lo = int(lo)
    return lo, min(lo + 1, n - 1), g


def _percentile_lerp(a, b, g):
    """numpy's ``_lerp``: ``a + (b - a) * g``, replaced by ``b - (b - a) * (1 - g)`` where ``g >= 0.5``."""
    a, b, g = np.float64(a), np.float64(b), np.float64(g)
    diff = np.subtract(b, a)
    return np.subtract(b, np.multiply(diff, np.subtract(np.float64(1), g))) if g >= 0.5 else np.add(a, np.multiply(diff, g))


def surface_metrics(pred, label, spacing=(1, 1, 1), percentile: float = 95.0, tolerances=(1.0,), empty: str = "raise") -> SurfaceMetrics:
    """The boundary metrics of two masks (as ``surface_distances`` takes them) in the units of ``spacing``: Hausdorff distance,
    its ``percentile``-th percentile per direction and pooled (MedPy's ``hd95``), average (symmetric) surface distances and the
    surface Dice at each of up to 8 ``tolerances`` -- see ``SurfaceMetrics``.  Percentiles are numpy's default (linear)
    ``np.percentile`` of the float64 distances, exactly: the order statistics come from a radix select on the device, the
    interpolation is numpy's arithmetic on the host.  Maxima and counts are exact; the means are float64 sums of a fixed shape
    (the same bits on every run).  Border extraction, distance transforms on the bounding box, gather, summary and select all
    run on the device (csrc/surface.hip); the host waits twice: for the sizes, and for one small record of results.
    ``empty``: a mask without voxels raises ValueError (``"raise"``, like MedPy) or gives ``inf`` for every distance and 0.0 for
    every ``nsd`` entry (``"inf"``)."""
    from .prep import normalize_sampling
    s = normalize_sampling(spacing, "spacing")
    q = float(percentile)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"seunet surface_metrics: `percentile` must lie in [0, 100], got {percentile!r}")
    tol = [float(t) for t in np.atleast_1d(np.asarray(tolerances, dtype=np.float64))]
    if len(tol) > SURFACE_MAX_TOLERANCES or any(not t >= 0.0 for t in tol):
        raise ValueError(f"seunet surface_metrics: `tolerances` must be at most {SURFACE_MAX_TOLERANCES} non-negative numbers, got {tolerances!r}")
    if empty not in ("raise", "inf"):
        raise ValueError(f"seunet surface_metrics: `empty` must be 'raise' or 'inf', got {empty!r}")
    ta, tb, _ = _surface_masks(pred, label, "seunet surface_metrics")
    lib = _lib.load()
    dev = ta.device
    ntol = len(tol)
    with torch.cuda.device(dev):
        n_a, n_b, box, ws = _surface_count(ta, tb)
        if n_a == 0 or n_b == 0:
            if empty == "raise":
                raise ValueError(f"seunet surface_metrics: a mask without voxels has no surface distances ({n_a} and {n_b} surface voxels)")
            inf = float("inf")
            return SurfaceMetrics(inf, inf, inf, inf, inf, inf, (0.0,) * ntol, n_a, n_b)
        dist, _ = _surface_emit(ta, s, n_a, n_b, box, ws, False)
        n = n_a + n_b
        parts = [(0, n_a), (n_a, n), (0, n)]                      # d_AB, d_BA, both
        pr = [_percentile_ranks(e - b, q) for b, e in parts]
        # one record: six order statistics, then the summary (its partial sums stay on the device)
        head = 8 * (6 + 6 + 2 * ntol)
        rec = torch.empty(48 + int(lib.seunet_surface_summary_bytes(ntol)), dtype=torch.uint8, device=dev)
        _select_ranks(dist, [r for lo, hi, _ in pr for r in (lo, hi)], [p for p in parts for _ in (0, 1)], rec[:48].view(torch.float64))
        _lib.check(lib.seunet_surface_summary(dist.data_ptr(), n_a, n_b, (C.c_double * max(ntol, 1))(*tol), ntol, rec[48:].data_ptr(),
                                              _lib.stream_ptr()), "surface_summary")
        raw = rec[:head].cpu().numpy()
    stat = raw[:48].view(np.float64)
    words = raw[48:].view(np.uint64)
    assert int(words[0]) == n_a and int(words[1]) == n_b
    mx = words[2:4].view(np.float64)
    sums = words[4:6].view(np.float64)
    le = words[6:].astype(np.int64).reshape(2, ntol)
    pct = [_percentile_lerp(stat[2 * i], stat[2 * i + 1], pr[i][2]) for i in range(3)]
    return SurfaceMetrics(hd=float(max(mx[0], mx[1])), hd_percentile=float(max(pct[0], pct[1])), hd_percentile_pooled=float(pct[2]),
                          asd_ab=float(sums[0] / np.float64(n_a)), asd_ba=float(sums[1] / np.float64(n_b)),
                          assd=float((sums[0] + sums[1]) / np.float64(n)),
                          nsd=tuple(float(np.float64(int(le[0, k]) + int(le[1, k])) / np.float64(n)) for k in range(ntol)),
                          n_a=n_a, n_b=n_b)
