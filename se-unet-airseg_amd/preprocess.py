"""CT preprocessing on the GPU (README step 1): the lung-field mask, the crop box and the cut volumes of the reference's
``savenpy`` / ``cutmask`` (preprocessing.py:26-130) with its helpers ``th_2t``, ``get_l`` and ``large_connected_domain26``
(util.py:95-165).  DESIGN.md section 3c.

The input is the int16 CT in the orientation the reference has after its transposes (preprocessing.py:33-45); file IO and
those transposes stay with the caller.  The voxel work runs in csrc/lung.hip and csrc/components.hip; what is left on the host
is the arithmetic on 300 histogram bins (peaks, ``measureDists``, the threshold, the padding value) and on the 3x2 box.  The
histograms come from 65536 per-value counts made on the device: ``np.histogram`` over the distinct values with the counts as
weights has the same edges and the same bin of every value as ``np.histogram`` over the voxels, because numpy's edge and
index arithmetic is per value.

numpy in -> numpy out; CUDA tensor in -> CUDA tensor out.  There is no CPU path."""
import ctypes
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._volume import out as _out, workspace
from .postprocess import _largest, maximum_3d

HU_SHIFT = 1024          # preprocessing.py:47
PAD_TH = -800            # preprocessing.py:53
BOX_MARGIN = 5           # preprocessing.py:86
MIN_AREA = 2000          # util.py:147-150

Array = Union[np.ndarray, torch.Tensor]


def _ct_cuda(ct, name) -> Tuple[torch.Tensor, bool]:
    if isinstance(ct, np.ndarray):
        if ct.dtype != np.int16:
            raise TypeError(f"seunet {name}: the CT must be int16, got {ct.dtype}")
        if not torch.cuda.is_available():
            raise RuntimeError(f"seunet {name}: needs a GPU (no CPU path)")
        t, as_numpy = torch.from_numpy(np.ascontiguousarray(ct)).cuda(), True
    elif isinstance(ct, torch.Tensor):
        if not ct.is_cuda:
            raise RuntimeError(f"seunet {name}: needs a CUDA tensor or a numpy array (no CPU path)")
        if ct.dtype != torch.int16:
            raise TypeError(f"seunet {name}: the CT must be int16, got {ct.dtype}")
        t, as_numpy = ct.contiguous(), False
    else:
        raise TypeError(f"seunet {name}: expected a numpy array or a CUDA tensor, got {type(ct).__name__}")
    if t.dim() != 3:
        raise ValueError(f"seunet {name}: expected a 3-D volume, got shape {tuple(t.shape)}")
    return t, as_numpy


# ---- host arithmetic on the histograms -------------------------------------------------------------------------------------
def histogram_from_counts(counts: np.ndarray, bins: int = 300):
    """``np.histogram(a, bins)`` of the int16 volume ``a`` whose per-value counts are ``counts`` (65536 entries, entry b counting
    the value ``int16(b)``): the same counts (int64) and the same float64 edges."""
    counts = np.asarray(counts)
    idx = np.flatnonzero(counts)
    if idx.size == 0:
        raise ValueError("histogram_from_counts: no voxel counted")
    values = idx.astype(np.uint16).view(np.int16)
    lo, hi = values.min(), values.max()
    return np.histogram(values, bins=bins, range=(lo, hi), weights=counts[idx].astype(np.int64))


def _peaks(hy: np.ndarray, hx: np.ndarray) -> Tuple[int, int]:
    """First peak = first index of the largest count; second = first index of the largest float32
    ``(hx[k + 1] - hx[first]) ** 2 * hy[k]`` (util.py:101-107, preprocessing.py:57-65)."""
    first = int(np.argmax(hy))
    dists = np.zeros(300, np.float32)
    dists[:hy.shape[0]] = (hx[1:hy.shape[0] + 1] - hx[first]) ** 2 * hy
    return first, int(np.argmax(dists))


def padding_value(hist) -> float:
    """preprocessing.py:55-68: the padding value ``aaa`` (float64) from the 300-bin histogram of the shifted CT, taken from
    the first edge >= -800 on."""
    hy, hx = hist
    k0 = int(np.flatnonzero(hx >= PAD_TH)[0])          # IndexError when no edge reaches -800, as np.where(...)[0][0]
    hy, hx = hy[k0:], hx[k0:]
    if hy.shape[0] == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    first, second = _peaks(hy, hx)
    first_peak, second_peak = hx[first], hx[second]
    return second_peak if second_peak < first_peak else first_peak


def threshold_from_hist(hist, kmax: int = 300) -> float:
    """util.py:95-117 on a ``kmax``-bin histogram: the left edge of the first minimum after both flanks of the two peaks are
    raised to the maximum."""
    hy, hx = hist
    hy = np.array(hy, copy=True)
    first, second = _peaks(hy, hx)
    top = hy.max()
    if second > first:
        hy[second:] = top
        hy[:first] = top
    else:
        hy[first:] = top
        hy[:second] = top
    return hx[int(np.argmin(hy))]


def clamped_counts(counts: np.ndarray, aaa: float) -> np.ndarray:
    """The value counts after ``case_pixels[case_pixels <= -800] = aaa`` (float64 truncated into int16)."""
    out = np.array(counts, dtype=np.int64, copy=True)
    values = np.arange(65536, dtype=np.uint16).view(np.int16)
    low = values <= PAD_TH
    moved = int(out[low].sum())
    out[low] = 0
    out[int(np.int16(np.trunc(aaa))) & 0xffff] += moved
    return out


def crop_box(lo, hi, shape) -> np.ndarray:
    """preprocessing.py:83-90 and :100-104: the 3x2 box of the mask's min / max coordinates with a margin of 5, the lower
    bound clipped at 0 and the upper at the shape, then the whole-volume box appended (6x2 int64)."""
    lo = np.asarray(lo, dtype=np.int64)
    hi = np.asarray(hi, dtype=np.int64)
    shape = np.asarray(shape, dtype=np.int64)
    box = np.stack([np.maximum(lo - BOX_MARGIN, 0), np.minimum(hi + BOX_MARGIN, shape)], axis=1)
    return np.concatenate([box, np.stack([np.zeros(3, np.int64), shape], axis=1)], axis=0)


# ---- device steps ----------------------------------------------------------------------------------------------------------
def value_counts(ct: torch.Tensor, shift: int = 0) -> np.ndarray:
    """65536 int64 counts of ``int16(ct + shift)`` (entry b counts the value ``int16(b)``)."""
    lib = _lib.load()
    with torch.cuda.device(ct.device):
        counts = torch.empty(65536, dtype=torch.int32, device=ct.device)
        _lib.check(lib.seunet_value_counts(ct.data_ptr(), ct.numel(), int(shift), counts.data_ptr(), _lib.stream_ptr()), "value_counts")
    return counts.cpu().numpy().view(np.uint32).astype(np.int64)


def _shift_clamp(ct: torch.Tensor, aaa: Optional[float]) -> torch.Tensor:
    lib = _lib.load()
    out = torch.empty_like(ct)
    clamp_to = int(np.int16(np.trunc(aaa))) if aaa is not None else 0
    with torch.cuda.device(ct.device):
        _lib.check(lib.seunet_shift_clamp(ct.data_ptr(), ct.numel(), HU_SHIFT, int(aaa is not None), PAD_TH, clamp_to, out.data_ptr(),
                                          _lib.stream_ptr()), "shift_clamp")
    return out


def _get_l(t: torch.Tensor, T: float, min_area: int) -> torch.Tensor:
    lib = _lib.load()
    h, w, z = (int(v) for v in t.shape)
    with torch.cuda.device(t.device):
        ws = workspace(lib.seunet_get_l_workspace_bytes, h, w, z, device=t.device)
        out = torch.empty((h, w, z), dtype=torch.uint8, device=t.device)
        _lib.check(lib.seunet_get_l(t.data_ptr(), h, w, z, float(T), int(min_area), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _lib.stream_ptr()), "get_l")
    return out


def _combine(a: torch.Tensor, b: torch.Tensor, op: int) -> torch.Tensor:
    lib = _lib.load()
    out = torch.empty_like(a)
    with torch.cuda.device(a.device):
        _lib.check(lib.seunet_mask_combine(a.data_ptr(), b.data_ptr(), a.numel(), op, out.data_ptr(), _lib.stream_ptr()), "mask_combine")
    return out


def _mask_extent(mask: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
    lib = _lib.load()
    h, w, z = (int(v) for v in mask.shape)
    with torch.cuda.device(mask.device):
        box = torch.empty(6, dtype=torch.int32, device=mask.device)
        _lib.check(lib.seunet_mask_box(mask.data_ptr(), h, w, z, box.data_ptr(), _lib.stream_ptr()), "mask_box")
    b = box.cpu().numpy().astype(np.int64)
    if b[1] < 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")   # np.min of an empty np.where
    return b[0::2], b[1::2]


def _crop(t: torch.Tensor, box: np.ndarray) -> torch.Tensor:
    lib = _lib.load()
    b = [int(v) for v in np.asarray(box)[:3].reshape(-1)]
    shape = tuple(int(v) for v in t.shape)
    for a in range(3):
        if not 0 <= b[2 * a] < b[2 * a + 1] <= shape[a]:
            raise ValueError(f"crop: box {b} is not a non-empty box inside the volume {shape}")
    out = torch.empty([b[2 * a + 1] - b[2 * a] for a in range(3)], dtype=t.dtype, device=t.device)
    arr = (ctypes.c_int * 6)(*b)
    with torch.cuda.device(t.device):
        _lib.check(lib.seunet_crop3d(t.data_ptr(), t.element_size(), shape[0], shape[1], shape[2], arr, out.data_ptr(),
                                     _lib.stream_ptr()), "crop3d")
    return out


# ---- the reference's functions ---------------------------------------------------------------------------------------------
def th_2t(ct: Array, format: str = "dcm") -> float:
    """util.py:95-117: the threshold ``T`` (float64) of the int16 volume ``ct`` (``format='jpg'``: 50 bins instead of 300)."""
    t, _ = _ct_cuda(ct, "th_2t")
    if format not in ("dcm", "jpg"):
        raise ValueError(f"th_2t: format {format!r} ('dcm': 300 bins, 'jpg': 50)")
    kmax = 50 if format == "jpg" else 300
    return threshold_from_hist(histogram_from_counts(value_counts(t), kmax), kmax)


def get_l(ct: Array, T: float, min_area: int = MIN_AREA):
    """util.py:120-152: the per-slice lung field of the int16 volume ``ct`` (uint8, numpy or CUDA tensor like the input)."""
    t, as_numpy = _ct_cuda(ct, "get_l")
    return _out(_get_l(t, T, min_area), as_numpy)


def large_connected_domain26(mask: Array):
    """util.py:156-165: the largest 26-connected component (equal counts: the highest label) with its 3-D holes filled, uint8.
    Raises IndexError for an empty mask, like the reference."""
    out, status, as_numpy = _largest(mask, _lib.CC_LARGEST_FILLED, "large_connected_domain26")
    if status != 0:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0 (large_connected_domain26: the mask is empty, util.py:162)")
    return _out(out, as_numpy)


def cut_mask(mask: Array, box) -> Array:
    """preprocessing.py:115-130 (cutmask) without the file IO: ``large_connected_domain26(mask)`` cropped to ``box`` (the
    6x2 box ``preprocess_ct`` returns; rows 0-2 are used), uint8."""
    as_numpy = isinstance(mask, np.ndarray)
    out = large_connected_domain26(torch.from_numpy(np.ascontiguousarray(mask)).cuda() if as_numpy else mask)
    return _out(_crop(out, box), as_numpy)


def preprocess_ct(ct: Array, mode: str = "prepro"):
    """preprocessing.py:47-112 (savenpy after the file read and the transposes) -> ``(data_cut, lung_mask, box)``.

    ``data_cut``: the shifted int16 CT (``ct + 1024``, padding clamped) cropped to the box, as the reference saves it
    (its loaders subtract 1024); ``lung_mask``: the lung mask cropped to the box, uint8; ``box``: the 6x2 int64 array of
    ``*_box.npy``.  ``mode='prediction'`` returns the whole clamped volume and ``None, None``.  Raises IndexError where the
    reference does (no lung component: ``maximum_3d``)."""
    if mode not in ("prepro", "prediction"):
        raise ValueError(f"preprocess_ct: mode {mode!r} ('prepro' or 'prediction')")
    t, as_numpy = _ct_cuda(ct, "preprocess_ct")
    counts = value_counts(t, HU_SHIFT)
    hist = histogram_from_counts(counts)
    values = np.arange(65536, dtype=np.uint16).view(np.int16)
    cmin = int(values[counts > 0].min())
    aaa = padding_value(hist) if cmin <= PAD_TH else None
    cp = _shift_clamp(t, aaa)
    if mode == "prediction":
        return _out(cp, as_numpy), None, None
    T = threshold_from_hist(histogram_from_counts(clamped_counts(counts, aaa) if aaa is not None else counts))
    L = _get_l(cp, T, MIN_AREA)
    L1 = maximum_3d(L)
    L2 = maximum_3d(_combine(L, L1, 0))
    mask = _combine(L1, L2, 1)
    lo, hi = _mask_extent(mask)
    box = crop_box(lo, hi, t.shape)
    return _out(_crop(cp, box), as_numpy), _out(_crop(mask, box), as_numpy), box
