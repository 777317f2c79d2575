"""Vectorised numpy / scipy restatement of the reference's CT preprocessing (preprocessing.py:47-130, util.py:95-165) for
volumes made at test time.  The per-slice work of ``get_l`` runs on the whole volume at once with structures that have no
extent along axis 2, so no component or hole crosses from one slice to the next; scipy numbers components by their first voxel
in raster order, which within one slice is the raster order of (i, j), the reference's tie rule."""
import os
import sys

import numpy as np
from scipy import ndimage

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "oracle"))
import components_oracle  # noqa: E402

PLANE8 = np.zeros((3, 3, 3), bool)
PLANE8[:, :, 1] = True
PLANE4 = np.zeros((3, 3, 3), bool)
PLANE4[1, :, 1] = PLANE4[:, 1, 1] = True


def peaks(hy, hx):
    first = int(np.argmax(hy))
    d = np.zeros(300, np.float32)
    d[:len(hy)] = (hx[1:len(hy) + 1] - hx[first]) ** 2 * hy
    return first, int(np.argmax(d))


def padding_value(hist):
    hy, hx = hist
    k0 = int(np.flatnonzero(hx >= -800)[0])
    first, second = peaks(hy[k0:], hx[k0:])
    return min(hx[k0 + first], hx[k0 + second])


def th_2t(a, kmax=300):
    hy, hx = np.histogram(a.ravel(), kmax)
    first, second = peaks(hy, hx)
    top = hy.max()
    lo, hi = (first, second) if second > first else (second, first)
    hy[hi:] = top
    hy[:lo] = top
    return hx[int(np.argmin(hy))]


def processed_slices(Z):
    sl = np.zeros(Z, bool)
    for n in range(int(0.05 * Z) - 1, int(0.95 * Z)):
        sl[n] = True
    return sl


def _slice_top(lab, num, k):
    """Per slice, the labels of the k largest components (ties: the smaller label) and their sizes; label 0 / size 0 = none."""
    Z = lab.shape[2]
    cnt = np.bincount(lab.ravel(), minlength=num + 1)
    labels = np.arange(1, num + 1)
    first = np.zeros(num + 1, np.int64)
    flat = lab.ravel()
    nz = np.flatnonzero(flat)
    first[flat[nz[::-1]]] = nz[::-1]                           # the smallest index of every label
    zs = first[1:] % Z
    order = np.lexsort((labels, -cnt[1:], zs))                 # by slice, then most pixels, then smallest label
    top_l = np.zeros((Z, k), np.int64)
    top_c = np.zeros((Z, k), np.int64)
    zs_o = zs[order]
    starts = np.searchsorted(zs_o, np.arange(Z))
    ends = np.searchsorted(zs_o, np.arange(Z), side="right")
    for j in range(k):
        ok = starts + j < ends
        idx = order[np.minimum(starts + j, len(order) - 1)] if len(order) else np.zeros(Z, np.int64)
        top_l[ok, j] = labels[idx[ok]]
        top_c[ok, j] = cnt[1:][idx[ok]]
    return top_l, top_c


def get_l(ct, T, min_area=2000):
    X, Y, Z = ct.shape
    sl = processed_slices(Z)
    A = (ct.astype(np.float64) >= T) & sl[None, None, :]
    lab, num = ndimage.label(A, structure=PLANE8)
    top_l, _ = _slice_top(lab, num, 1)
    lut = np.zeros(num + 1, bool)
    lut[top_l[:, 0]] = True
    lut[0] = False
    img1 = lut[lab]
    has = top_l[:, 0] > 0
    filled = ndimage.binary_fill_holes(img1, structure=PLANE4)
    holes = filled & ~img1 & (sl & has)[None, None, :]
    hl, hn = ndimage.label(holes, structure=PLANE8)
    tl, tc = _slice_top(hl, hn, 2)
    keep = np.zeros(hn + 1, bool)
    for j in range(2):
        big = tc[:, j] > min_area
        keep[tl[big, j]] = True
    keep[0] = False
    return keep[hl].astype(np.uint8)


def maximum_3d(v):
    return components_oracle.maximum_3d(v)


def large_connected_domain26(mask):
    lab, num = ndimage.label(mask != 0, structure=np.ones((3, 3, 3)))
    if num == 0:
        raise IndexError("empty mask")
    cnt = np.bincount(lab.ravel())[1:]
    best = int(np.flatnonzero(cnt == cnt.max())[-1]) + 1          # the highest label among equal counts
    return ndimage.binary_fill_holes(lab == best).astype(np.uint8)


def preprocess_ct(ct, mode="prepro"):
    cp = (ct + np.int16(1024)).astype(np.int16)
    aaa = None
    if cp.min() <= -800:
        aaa = padding_value(np.histogram(cp.ravel(), 300))
        cp[cp <= -800] = aaa
    if mode == "prediction":
        return cp, None, None, {"aaa": aaa}
    T = th_2t(cp)
    L = get_l(cp, T)
    L1 = maximum_3d(L)
    L2 = maximum_3d(L ^ L1)
    mask = L1 | L2
    xx, yy, zz = np.where(mask)
    lo = np.array([xx.min(), yy.min(), zz.min()])
    hi = np.array([xx.max(), yy.max(), zz.max()])
    shape = np.array(ct.shape)
    box = np.stack([np.maximum(lo - 5, 0), np.minimum(hi + 5, shape)], 1).astype(np.int64)
    box = np.concatenate([box, np.stack([np.zeros(3, np.int64), shape], 1)], 0)
    s = tuple(slice(box[a, 0], box[a, 1]) for a in range(3))
    return cp[s], mask[s].astype(np.uint8), box, {"aaa": aaa, "T": T, "L": L, "L1": L1, "L2": L2, "Mask": mask}


def cut_mask(mask, box):
    out = large_connected_domain26(mask)
    return out[box[0, 0]:box[0, 1], box[1, 0]:box[1, 1], box[2, 0]:box[2, 1]]
