"""Stage-2 / stage-3 preparation on the GPU: exact EDT, hard-mining candidate sets, LIB weight and break weight.

The reference computes these on the CPU with scipy / skimage / cc3d (data.py:304-306, 455-458 on every stage-2/3
``__getitem__``; lib_weight.py:12-17, 36-53 and weight_br.py:113-177 once per case).  Here they are HIP kernels
(csrc/edt.hip) on volumes resident in HBM; the candidate lists are bit-packed masks downloaded once per case and indexed on
the host, so a draw costs no device synchronisation.  Masks are uint8 volumes with non-zero = 1; there is no CPU path."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, topology
from ._volume import mask_in, out as _out, read_status, workspace
from .postprocess import maximum_3d

_BLOCK_WORDS = 8          # 512 voxels per prefix-sum block
SKELETON_ROUND_LAUNCHES = 32   # kRoundLaunches of csrc/skeleton.hip (scripts/bench_skeleton.py counts launches with it)


def _vol(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"seunet prep: `{name}` must be a CUDA tensor resident on the GPU (there is no CPU path)")
    if t.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"seunet prep: `{name}` has dtype {t.dtype}; expected uint8 (0/1)")
    if t.dim() != 3:
        raise ValueError(f"seunet prep: `{name}` must be (n0, n1, n2), got {tuple(t.shape)}")
    return (t.to(torch.uint8) if t.dtype == torch.bool else t).contiguous()


def _same(a, b, na, nb):
    if a.shape != b.shape:
        raise ValueError(f"seunet prep: `{nb}` shape {tuple(b.shape)} differs from `{na}`'s {tuple(a.shape)}")
    if a.device != b.device:
        raise ValueError(f"seunet prep: `{nb}` is on {b.device}, `{na}` on {a.device}")


def _status(status, what):
    if read_status(status) != 0:
        raise ValueError(f"seunet prep: {what}")


def normalize_sampling(sampling, what: str = "sampling") -> Tuple[float, float, float]:
    """``sampling`` as three float64 values, like scipy's ``_normalize_sequence``: a scalar is repeated over the three axes, a
    sequence must have length 3.  ValueError for any other length and for values that are not positive and finite."""
    s = np.asarray(sampling, dtype=np.float64)
    if s.ndim == 0:
        s = np.repeat(s, 3)
    if s.shape != (3,):
        raise ValueError(f"seunet prep: `{what}` must be a number or a sequence of 3 numbers, got shape {s.shape}")
    if not (np.all(np.isfinite(s)) and np.all(s > 0)):
        raise ValueError(f"seunet prep: `{what}` must be positive and finite, got {tuple(float(v) for v in s)}")
    return tuple(float(v) for v in s)


def _edt_sampling(vol, s, want_dist: bool, want_indices: bool, want_lin: bool = False):
    """The sampled EDT of a checked device mask: (dist, indices, lin), None where not wanted.  ValueError without a zero voxel."""
    n0, n1, n2 = (int(v) for v in vol.shape)
    lib = _lib.load()
    dev = vol.device
    with torch.cuda.device(dev):
        ws = workspace(lib.seunet_edt_sampling_workspace_bytes, n0, n1, n2, device=dev, min_bytes=1)
        dist = torch.empty((n0, n1, n2), dtype=torch.float64, device=dev) if want_dist else None
        ind = torch.empty((3, n0, n1, n2), dtype=torch.int32, device=dev) if want_indices else None
        lin = torch.empty((n0, n1, n2), dtype=torch.int32, device=dev) if want_lin else None
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.seunet_edt_sampling(vol.data_ptr(), n0, n1, n2, s[0], s[1], s[2], _lib.ptr(dist), _lib.ptr(ind), _lib.ptr(lin),
                                           status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "edt_sampling")
        _status(status, "distance_transform_edt: the volume has no zero voxel (the distance is undefined)")
    return dist, ind, lin


def distance_transform_edt(volume: torch.Tensor, return_distances: bool = True, return_indices: bool = False,
                           return_sqdist: bool = False, *, sampling=None):
    """``scipy.ndimage.distance_transform_edt(volume, sampling=..., return_indices=...)`` on the GPU: for every voxel the
    distance to the nearest zero voxel.  ``dist`` (float64) and ``indices`` (int32, (3, n0, n1, n2)) are bitwise
    scipy's, ties included; ``sqdist`` is the int32 squared distance.  Returns the requested outputs in the order
    (sqdist, dist, indices), a single tensor when one is requested.  A volume with no zero voxel raises ValueError.

    ``sampling=None``: unit sampling, the integer passes of csrc/edt.hip.  ``sampling`` a positive finite number or three of them:
    the voxel spacing along each axis, scipy's feature transform in float64 (csrc/edt_sampling.hip);
    ``dist`` is then in the units of ``sampling``, and ``return_sqdist`` is a ValueError (there is no integer squared distance)."""
    vol = _vol(volume, "volume")
    if not (return_distances or return_indices or return_sqdist):
        raise ValueError("seunet prep: at least one of return_distances / return_indices / return_sqdist must be set")
    if sampling is not None:
        s = normalize_sampling(sampling)
        if return_sqdist:
            raise ValueError("seunet prep: return_sqdist is the integer squared distance of unit sampling; it is not defined with `sampling`")
        dist, ind, _ = _edt_sampling(vol, s, bool(return_distances), bool(return_indices))
        out = tuple(t for t in (dist, ind) if t is not None)
        return out[0] if len(out) == 1 else out
    n0, n1, n2 = (int(v) for v in vol.shape)
    lib = _lib.load()
    dev = vol.device
    with torch.cuda.device(dev):
        ws = workspace(lib.seunet_edt_workspace_bytes, n0, n1, n2, device=dev, min_bytes=1)
        sq = torch.empty((n0, n1, n2), dtype=torch.int32, device=dev) if return_sqdist else None
        dist = torch.empty((n0, n1, n2), dtype=torch.float64, device=dev) if return_distances else None
        ind = torch.empty((3, n0, n1, n2), dtype=torch.int32, device=dev) if return_indices else None
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.seunet_edt(vol.data_ptr(), n0, n1, n2, _lib.ptr(sq), _lib.ptr(dist), _lib.ptr(ind), status.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "edt")
        _status(status, "distance_transform_edt: the volume has no zero voxel (the distance is undefined)")
    out = tuple(t for t in (sq, dist, ind) if t is not None)
    return out[0] if len(out) == 1 else out


def skeletonize_3d(volume, return_passes: bool = False):
    """The centreline volume the reference takes from ``skimage.morphology.skeletonize_3d(label)`` (ske_and_parse.py:83,
    weight_br.py:128, prediction.py:127), thinned on the GPU (csrc/skeleton.hip): Lee, Kashyap and Chu (1994) with the border
    order and raster-order re-check of the common implementations; equality with skimage has not been checked.  The
    definition is DESIGN.md section 3d; the result equals tests/skeleton_oracle.py bit for bit and is deterministic.

    CUDA uint8 / bool tensor in -> uint8 CUDA tensor (0/1) on the same device; numpy array in (any dtype, non-zero =
    foreground) -> uint8 numpy out, like ``postprocess.largest_component``.  The input is not modified; an empty volume gives
    zeros.  The result is the ``skeleton`` argument of ``break_weight``, ``hard_mining_candidates``, the ``from_case``
    constructors and ``evaluation_case``.  ``return_passes``: also return the number of thinning passes run (the last one,
    which deletes nothing, included)."""
    vol, as_numpy = _mask_in(volume, "volume")
    n0, n1, n2 = (int(v) for v in vol.shape)
    dev = vol.device
    out = torch.zeros((n0, n1, n2), dtype=torch.uint8, device=dev)
    passes = torch.zeros(1, dtype=torch.int32, device=dev)
    if vol.numel():
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = workspace(lib.seunet_skeleton_workspace_bytes, n0, n1, n2, device=dev, what="seunet prep: skeletonize_3d")
            _lib.check(lib.seunet_skeletonize(vol.data_ptr(), n0, n1, n2, out.data_ptr(), passes.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr()), "skeletonize")
    skel = _out(out, as_numpy)
    return (skel, int(passes.item())) if return_passes else skel


class _Axis:
    """``cs[ax]``: one axis of the ``np.where`` triple, indexed lazily."""

    def __init__(self, cs: "CandidateSet", ax: int):
        self._cs, self._ax = cs, ax

    def __len__(self) -> int:
        return len(self._cs)

    def __getitem__(self, k) -> int:
        return self._cs.coords(k)[self._ax]


class CandidateSet:
    """The voxels of a mask in raster order, like ``np.where(mask)``, without materialising the index triple:
    ``len(cs[0])`` is the count and ``cs[ax][k]`` the ``ax`` coordinate of the k-th voxel.  Storage: the bit-packed mask
    (bit j of word w = voxel 64 w + j) on the host plus popcount prefix sums per 512-voxel block; ``cs[ax][k]`` is a binary
    search and one block unpack.  ``draw_stage2_plan`` / ``draw_stage3_plan`` accept it wherever they take a triple."""

    def __init__(self, words: np.ndarray, shape: Sequence[int]):
        self.shape = tuple(int(v) for v in shape)
        n = int(np.prod(self.shape, dtype=np.int64))
        nw = (n + 63) // 64
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        if words.size < nw:
            raise ValueError(f"CandidateSet: {words.size} words for {n} voxels")
        words = words[:nw].copy()
        if n % 64:
            words[-1] &= np.uint64((1 << (n % 64)) - 1)
        pad = (-nw) % _BLOCK_WORDS
        self._words = np.concatenate([words, np.zeros(pad, np.uint64)])
        blocks = np.bitwise_count(self._words).reshape(-1, _BLOCK_WORDS).sum(axis=1, dtype=np.int64)
        self._prefix = np.concatenate([np.zeros(1, np.int64), np.cumsum(blocks)])
        self._count = int(self._prefix[-1])
        self._last = (None, None)

    @classmethod
    def from_numpy(cls, mask: np.ndarray) -> "CandidateSet":
        """Host path: the set of ``np.where(mask)``."""
        mask = np.asarray(mask)
        bits = np.packbits(mask.reshape(-1) != 0, bitorder="little")
        bits = np.concatenate([bits, np.zeros((-bits.size) % 8, np.uint8)])
        return cls(bits.view("<u8"), mask.shape)

    @classmethod
    def from_mask(cls, mask: torch.Tensor) -> "CandidateSet":
        """The set of ``np.where(mask != 0)`` of a device volume (e.g. ``loc_break = where(br_skel == 1)``, weight_br.py:171):
        packed on the device, downloaded once."""
        m = _vol(mask, "mask")
        n = m.numel()
        with torch.cuda.device(m.device):
            bits = torch.empty((n + 63) // 64, dtype=torch.int64, device=m.device)
            _lib.check(_lib.load().seunet_mask_bits(m.data_ptr(), n, bits.data_ptr(), _lib.stream_ptr()), "mask_bits")
            host = bits.cpu().numpy().view(np.uint64)
        return cls(host, m.shape)

    def __len__(self) -> int:
        return self._count

    def __getitem__(self, ax: int) -> _Axis:
        if not 0 <= int(ax) < len(self.shape):
            raise IndexError(f"CandidateSet: axis {ax} of a {len(self.shape)}-d set")
        return _Axis(self, int(ax))

    def linear(self, k) -> int:
        """Raster index of the k-th voxel."""
        k = int(k)
        if k < 0:
            k += self._count
        if not 0 <= k < self._count:
            raise IndexError(f"CandidateSet: index {k} out of range for {self._count} voxels")
        b = int(np.searchsorted(self._prefix, k, side="right")) - 1
        block = self._words[b * _BLOCK_WORDS:(b + 1) * _BLOCK_WORDS]
        pos = np.flatnonzero(np.unpackbits(block.view(np.uint8), bitorder="little"))
        return b * 64 * _BLOCK_WORDS + int(pos[k - int(self._prefix[b])])

    def coords(self, k) -> Tuple[int, ...]:
        k = int(k)
        if self._last[0] != k:            # _start_near reads the three axes of one k in a row
            self._last = (k, tuple(int(v) for v in np.unravel_index(self.linear(k), self.shape)))
        return self._last[1]

    def to_numpy(self) -> Tuple[np.ndarray, ...]:
        """The materialised ``np.where`` triple (tests, small volumes)."""
        n = int(np.prod(self.shape, dtype=np.int64))
        bits = np.unpackbits(self._words.view(np.uint8), bitorder="little")[:n]
        return np.unravel_index(np.flatnonzero(bits), self.shape)


def hard_mining_candidates(label: torch.Tensor, skeleton: torch.Tensor, pred: torch.Tensor) -> Tuple[CandidateSet, CandidateSet]:
    """``(loc_skeleton, loc_small)`` of ``AirwayHMData.crop`` / ``AirwayHMData3.crop`` (data.py:304-306, :455-458):
    ``where(skeleton * (1 - pred))`` = skeleton != 0 and pred != 1, and ``where(distance_transform_edt(label) * skeleton < 2)``
    = skeleton == 0 or a zero label voxel within squared distance 3.  One launch, two bit masks downloaded."""
    label, skeleton, pred = _vol(label, "label"), _vol(skeleton, "skeleton"), _vol(pred, "pred")
    _same(label, skeleton, "label", "skeleton")
    _same(label, pred, "label", "pred")
    n0, n1, n2 = (int(v) for v in label.shape)
    nw = (label.numel() + 63) // 64
    with torch.cuda.device(label.device):
        bits = torch.empty((2, nw), dtype=torch.int64, device=label.device)
        _lib.check(_lib.load().seunet_hard_mining_masks(label.data_ptr(), skeleton.data_ptr(), pred.data_ptr(), n0, n1, n2,
                                                        bits[0].data_ptr(), bits[1].data_ptr(), _lib.stream_ptr()),
                   "hard_mining_masks")
        host = bits.cpu().numpy().view(np.uint64)
    return CandidateSet(host[0], label.shape), CandidateSet(host[1], label.shape)


def lib_table() -> np.ndarray:
    """344 float32 entries: ``-log10(float32(k) / float32(343))``, entry 0 = ``-log10(1)`` (lib_weight.py:12-17 in numpy's own
    float32 arithmetic; the kernel looks the 7x7x7 counts up here and never calls log10 itself)."""
    k = np.arange(344, dtype=np.float32)
    q = k / np.float32(343)
    q[q == 0] = 1
    return (-np.log10(q)).astype(np.float32)


def lib_weight(label: torch.Tensor) -> torch.Tensor:
    """The float16 LIB weight ``save_lib_weight`` writes (lib_weight.py:36-53, without ``** 2.5``), bitwise: 7x7x7 box count
    of the label with mode 'mirror', / 343, 0 -> 1, -log10, * label, float16 (signed zeros included)."""
    label = _vol(label, "label")
    n0, n1, n2 = (int(v) for v in label.shape)
    lib = _lib.load()
    table = np.ascontiguousarray(lib_table())
    with torch.cuda.device(label.device):
        ws = workspace(lib.seunet_lib_weight_workspace_bytes, n0, n1, n2, device=label.device)
        out = torch.empty((n0, n1, n2), dtype=torch.float16, device=label.device)
        _lib.check(lib.seunet_lib_weight(label.data_ptr(), n0, n1, n2, table.ctypes.data, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr()), "lib_weight")
    return out


def break_weight(label: torch.Tensor, pred: torch.Tensor, skeleton: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``save_weight_break`` (weight_br.py:113-177) with the skeleton passed in (the reference's ``skeletonize_3d(label)``):
    returns ``(w_br float16, br_skel uint8)``, bitwise the reference's; ``CandidateSet.from_mask(br_skel)`` is its saved
    ``loc_break``.  When the reference's maxf is 0 both volumes are zeros (an empty ``loc_break``; the reference saves a zero
    volume there).  An empty skeleton raises ValueError."""
    label, pred, skeleton = _vol(label, "label"), _vol(pred, "pred"), _vol(skeleton, "skeleton")
    _same(label, pred, "label", "pred")
    _same(label, skeleton, "label", "skeleton")
    n0, n1, n2 = (int(v) for v in label.shape)
    lib = _lib.load()
    dev = label.device
    with torch.cuda.device(dev):
        ws = workspace(lib.seunet_break_weight_workspace_bytes, n0, n1, n2, device=dev)
        w = torch.empty((n0, n1, n2), dtype=torch.float16, device=dev)
        brs = torch.empty((n0, n1, n2), dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.seunet_break_weight(label.data_ptr(), pred.data_ptr(), skeleton.data_ptr(), n0, n1, n2, w.data_ptr(),
                                           brs.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                   "break_weight")
        _status(status, "break_weight: the skeleton is empty")
    return w, brs


# ---- airway tree parsing: the ATM'22 branch labelling (csrc/parse.hip) -------------------------------

def _mask_in(a, name):
    """A 0/1 volume argument -> (uint8 CUDA tensor, came-as-numpy): numpy of any dtype, or a uint8 / bool CUDA tensor (``_vol``)."""
    return mask_in(a, name, "seunet prep", _vol)


def _labels_in(a, name):
    """An integer label volume argument -> (int32 CUDA tensor, came-as-numpy)."""
    if isinstance(a, np.ndarray):
        if a.ndim != 3:
            raise ValueError(f"seunet prep: `{name}` must be (n0, n1, n2), got {tuple(a.shape)}")
        if not torch.cuda.is_available():
            raise RuntimeError(f"seunet prep: `{name}` needs a GPU (there is no CPU path)")
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda(), True
    if not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise RuntimeError(f"seunet prep: `{name}` must be a CUDA tensor resident on the GPU (there is no CPU path)")
    if a.dim() != 3:
        raise ValueError(f"seunet prep: `{name}` must be (n0, n1, n2), got {tuple(a.shape)}")
    if a.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8):
        raise TypeError(f"seunet prep: `{name}` has dtype {a.dtype}; expected an integer label volume")
    return a.to(torch.int32).contiguous(), False


def _skeleton_parsing(skel, min_voxels):
    n0, n1, n2 = (int(v) for v in skel.shape)
    dev = skel.device
    parse = torch.zeros((n0, n1, n2), dtype=torch.uint8, device=dev)
    cd = torch.zeros((n0, n1, n2), dtype=torch.int32, device=dev)
    if skel.numel() == 0:
        return parse, cd, 0
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = workspace(lib.seunet_skeleton_branches_workspace_bytes, n0, n1, n2, device=dev, what="seunet prep: skeleton_parsing")
        num = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.seunet_skeleton_branches(skel.data_ptr(), n0, n1, n2, int(min_voxels), cd.data_ptr(), parse.data_ptr(),
                                                num.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "skeleton_branches")
        return parse, cd, int(num.item())


def skeleton_parsing(skeleton, min_voxels: int = 5):
    """``skeleton_parsing`` of the ATM'22 parser (atm22_skel_parse.py:83-101) -> ``(skeleton_parse uint8, cd int32, num)``,
    bitwise the reference's: skeleton voxels whose 3x3x3 sum (``ndimage.convolve``, mode 'reflect') exceeds 3 are removed, the
    rest is labelled with 26-connectivity, components under ``min_voxels`` voxels are removed, and the survivors are numbered
    as the reference's second ``ndimage.label`` numbers them.  CUDA tensor in -> CUDA tensors out, numpy in -> numpy out; the
    input is not modified.  Reading ``num`` synchronises once."""
    skel, as_numpy = _mask_in(skeleton, "skeleton")
    parse, cd, num = _skeleton_parsing(skel, min_voxels)
    return _out(parse, as_numpy), _out(cd, as_numpy), num


def _assign(parse, label, cd):
    n0, n1, n2 = (int(v) for v in label.shape)
    dev = label.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = workspace(lib.seunet_parse_assign_workspace_bytes, n0, n1, n2, device=dev, min_bytes=1)
        out = torch.empty((n0, n1, n2), dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.seunet_parse_assign(parse.data_ptr(), cd.data_ptr(), label.data_ptr(), n0, n1, n2, out.data_ptr(),
                                           status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "parse_assign")
        _status(status, "tree_parsing_func: skeleton_parse is empty (the nearest branch is undefined)")
    return out


def tree_parsing_func(skeleton_parse, label, cd):
    """``tree_parsing_func`` (atm22_skel_parse.py:103-108; also the last line of ``ske_and_parse.airway_parse``): every voxel of
    ``label`` gets the number ``cd`` holds at the nearest voxel of ``skeleton_parse``, nearest as scipy's
    ``distance_transform_edt(1 - skeleton_parse, return_indices=True)`` decides it, ties included; 0 outside the label.  int32,
    bitwise the reference's.  An empty ``skeleton_parse`` raises ValueError."""
    parse, np0 = _mask_in(skeleton_parse, "skeleton_parse")
    lab, np1 = _mask_in(label, "label")
    c, np2 = _labels_in(cd, "cd")
    _same(parse, lab, "skeleton_parse", "label")
    _same(parse, c, "skeleton_parse", "cd")
    if parse.numel() == 0:
        raise ValueError("seunet prep: tree_parsing_func: skeleton_parse is empty (the nearest branch is undefined)")
    return _out(_assign(parse, lab, c), np0 and np1 and np2)


def _label_stats(parsing, num):
    """(counts int64[num + 1], adjacency bool[num + 1, num + 1]) of an int32 device volume with values 0..num."""
    lib = _lib.load()
    num = int(num)
    cap = int(lib.seunet_label_stats_max_num())
    if not 0 <= num <= cap:
        raise ValueError(f"seunet prep: label statistics support labels up to {cap}, got num = {num}")
    n0, n1, n2 = (int(v) for v in parsing.shape)
    words = (num + 1 + 63) // 64
    dev = parsing.device
    with torch.cuda.device(dev):
        counts = torch.empty(num + 1, dtype=torch.int32, device=dev)
        bits = torch.empty((num + 1, words), dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        if parsing.numel():
            _lib.check(lib.seunet_label_stats(parsing.data_ptr(), n0, n1, n2, num, counts.data_ptr(), bits.data_ptr(), status.data_ptr(),
                                              _lib.stream_ptr()), "label_stats")
        else:
            counts.zero_(); bits.zero_(); status.zero_()
        _status(status, f"label statistics: the volume holds a label outside 0..{num}")
        c = counts.cpu().numpy().view(np.uint32).astype(np.int64)
        b = bits.cpu().numpy().view(np.uint8)
    adj = np.unpackbits(b, axis=1, bitorder="little")[:, :num + 1].astype(bool)
    return c, adj


def label_adjacency(parsing, num: int):
    """The two statistics the refinement of the ATM'22 parser takes from a label volume, in one pass on the device:
    ``counts`` (int64[num], voxels of label k + 1: ``loc_trachea``, atm22_skel_parse.py:110-118) and ``ad`` (uint8[num, num],
    ``ad[i, j] = 1`` iff labels i + 1 and j + 1 meet across a face: ``adjacent_map``, :120-135).  numpy arrays.  A label outside
    0..num raises ValueError, as does a ``num`` above the kernel's cap (4095)."""
    vol, _ = _labels_in(parsing, "parsing")
    c, adj = _label_stats(vol, num)
    return c[1:], adj[1:, 1:].astype(np.uint8)


def _parent_children(ad: np.ndarray, trachea: int, num: int):
    """Breadth-first parent / children relation from the trachea (0-based), atm22_skel_parse.py:137-165: a level is taken from
    its end, children in ascending order, a visited node takes a further parent when it lies exactly one generation below, and
    the generation counter is uint8 (it wraps)."""
    parent = np.zeros((num, num), dtype=np.uint8)
    children = np.zeros((num, num), dtype=np.uint8)
    generation = np.zeros(num, dtype=np.uint8)
    parent[trachea, trachea] = 1
    level = [trachea]
    while level:
        todo, level = level, []
        while todo:
            cur = todo.pop()
            for child in np.flatnonzero(ad[cur] > 0):
                if not parent[child].any():
                    parent[child, cur] = 1
                    children[cur, child] = 1
                    generation[child] = generation[cur] + 1
                    level.append(int(child))
                elif generation[cur] + 1 == generation[child]:
                    parent[child, cur] = 1
                    children[cur, child] = 1
    return parent, children


def _merge_steps(parent: np.ndarray, children: np.ndarray):
    """The (from, to) label replacements (1-based values) of one merge sweep and the 0-based labels it deletes, in the
    reference's order (atm22_skel_parse.py:219-243 = :167-196): all parents of a multi-parent node fuse into the first, then an
    only child fuses into its parent."""
    steps, deleted = [], []
    for node in np.flatnonzero(parent.sum(axis=1) > 1):
        ps = np.flatnonzero(parent[node] > 0)
        for p in ps[1:]:
            steps.append((int(p) + 1, int(ps[0]) + 1))
            if p not in deleted:
                deleted.append(int(p))
    for node in np.flatnonzero(children.sum(axis=1) == 1):
        if node in deleted:
            continue
        child = int(np.flatnonzero(children[node] == 1)[0])
        if child not in deleted:
            steps.append((child + 1, int(node) + 1))
            deleted.append(child)
    return steps, deleted


def refine_labels(counts: np.ndarray, adjacency: np.ndarray, num: int):
    """The refinement loop of tree_parsing.py:148-159 on the statistics of the unrefined volume instead of the volume:
    ``counts`` (int[num + 1]) and ``adjacency`` (bool[num + 1, num + 1]) indexed by label value.  Every step of the loop replaces
    one label value by another everywhere, so a table over the values follows it exactly: the counts of fused values add and
    their adjacency rows unite.  -> ``(lut int32[num + 1], final num, rounds)`` with ``final = lut[unrefined]``."""
    size = int(num) + 1
    counts = np.asarray(counts, dtype=np.int64).copy()
    adj = np.asarray(adjacency, dtype=bool).copy()
    lut = np.arange(size, dtype=np.int64)
    rounds = 0
    while num > 0:
        trachea = int(np.argsort(counts[1:num + 1].astype(np.float64))[-1])
        parent, children = _parent_children(adj[1:num + 1, 1:num + 1].astype(np.uint8), trachea, num)
        steps, deleted = _merge_steps(parent, children)
        if not deleted:
            break
        rounds += 1
        m = np.arange(size, dtype=np.int64)                  # value at the start of the round -> value now
        for _ in range(2):                                   # whether_refinement merges in place, tree_refinement merges again
            for a, b in steps:
                m[m == a] = b
        gone = np.asarray(deleted)
        for i in range(num):                                 # compaction, in place and in ascending order
            if i not in deleted:
                m[m == i + 1] = i + 1 - int((gone < i).sum())
        num -= len(deleted)
        counts = np.bincount(m, weights=counts, minlength=size).astype(np.int64)
        a, b = np.nonzero(adj)
        adj = np.zeros_like(adj)
        adj[m[a], m[b]] = True
        adj[np.arange(size), np.arange(size)] = False
        lut = m[lut]
    return lut.astype(np.int32), int(num), rounds


def tree_parsing(label, skeleton=None, refine: bool = True, return_num: bool = False):
    """The ATM'22 parser from the skeleton on (tree_parsing.py:114-159 without meshes and pictures): the int32 ``parsing`` volume
    ``evaluation_case`` and ``branch_detected_calculation`` take, bitwise the reference's.  ``skeleton=None`` thins the label
    with ``skeletonize_3d``.  Steps: ``skeleton_parsing``, ``tree_parsing_func``, then the refinement loop, which runs on the host
    on one pass of label statistics (``refine_labels``) and is applied by one look-up pass.  ``refine=False`` stops before the
    loop.  ``return_num``: also return the number of branches.  CUDA tensor in -> CUDA tensor out, numpy in -> numpy out."""
    lab, as_numpy = _mask_in(label, "label")
    if skeleton is None:
        skel = skeletonize_3d(lab)
    else:
        skel, _ = _mask_in(skeleton, "skeleton")
        _same(lab, skel, "label", "skeleton")
    parse, cd, num = _skeleton_parsing(skel, 5)
    if num == 0:
        raise ValueError("seunet prep: tree_parsing: no skeleton branch of 5 voxels or more (the nearest branch is undefined)")
    parsing = _assign(parse, lab, cd)
    if refine:
        counts, adj = _label_stats(parsing, num)
        lut, num, _ = refine_labels(counts, adj, num)
        table = torch.from_numpy(lut).to(lab.device)
        with torch.cuda.device(lab.device):
            _lib.check(_lib.load().seunet_relabel(parsing.data_ptr(), parsing.numel(), table.data_ptr(), table.numel(),
                                                  parsing.data_ptr(), _lib.stream_ptr()), "relabel")
    out = _out(parsing, as_numpy)
    return (out, num) if return_num else out


def relabel(parsing, lut):
    """``lut[parsing]`` on the device (``seunet_relabel``): int32 out; a value outside the table gives 0."""
    vol, as_numpy = _labels_in(parsing, "parsing")
    table = torch.as_tensor(np.ascontiguousarray(np.asarray(lut.cpu() if isinstance(lut, torch.Tensor) else lut), dtype=np.int32)).to(vol.device)
    out = torch.empty_like(vol)
    if vol.numel():
        with torch.cuda.device(vol.device):
            _lib.check(_lib.load().seunet_relabel(vol.data_ptr(), vol.numel(), table.data_ptr(), table.numel(), out.data_ptr(),
                                                  _lib.stream_ptr()), "relabel")
    return _out(out, as_numpy)


# ---- airway tree parsing: the reference's own parser (csrc/morph.hip, components.hip, parse.hip, topology.py) -----

def _morph(vol, op, what):
    n0, n1, n2 = (int(v) for v in vol.shape)
    dev = vol.device
    out = torch.empty((n0, n1, n2), dtype=torch.uint8, device=dev)
    if vol.numel():
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = workspace(lib.seunet_binary_morph_workspace_bytes, n0, n1, n2, device=dev, min_bytes=1)
            _lib.check(lib.seunet_binary_morph(vol.data_ptr(), n0, n1, n2, op, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), what)
    return out


def binary_dilation(volume):
    """``skimage.morphology.binary_dilation(volume)`` with its default footprint, the cross of the 6 face neighbours, as
    ``scipy.ndimage.binary_dilation`` states it (outside the volume = 0; not checked against skimage).  uint8 0/1 out; CUDA tensor
    in -> CUDA tensor out, numpy in -> numpy out; the input is not modified."""
    vol, as_numpy = _mask_in(volume, "volume")
    return _out(_morph(vol, _lib.MORPH_DILATE, "binary_dilation"), as_numpy)


def binary_erosion(volume, border_value: int = 0):
    """``scipy.ndimage.binary_erosion(volume, border_value=...)`` with the 6-neighbour cross: outside the volume counts as
    ``border_value`` (0 or 1)."""
    if border_value not in (0, 1, False, True):
        raise ValueError(f"seunet prep: binary_erosion: border_value {border_value!r} (0 or 1)")
    vol, as_numpy = _mask_in(volume, "volume")
    return _out(_morph(vol, _lib.MORPH_ERODE_BORDER1 if border_value else _lib.MORPH_ERODE_BORDER0, "binary_erosion"), as_numpy)


def binary_closing(volume):
    """``skimage.morphology.binary_closing(volume)`` with the 6-neighbour cross: ``binary_erosion(binary_dilation(volume),
    border_value=1)``, bit for bit, in one call on the packed bits (the reading of skimage 0.21-0.24; not checked against
    skimage)."""
    vol, as_numpy = _mask_in(volume, "volume")
    return _out(_morph(vol, _lib.MORPH_CLOSE, "binary_closing"), as_numpy)


def binary_fill_holes(volume):
    """``scipy.ndimage.binary_fill_holes(volume)``: the volume plus the 6-connected background that does not reach its border.
    uint8 0/1 out."""
    vol, as_numpy = _mask_in(volume, "volume")
    n0, n1, n2 = (int(v) for v in vol.shape)
    dev = vol.device
    out = torch.empty((n0, n1, n2), dtype=torch.uint8, device=dev)
    if vol.numel():
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = workspace(lib.seunet_cc_workspace_bytes, n0, n1, n2, device=dev)
            _lib.check(lib.seunet_fill_holes(vol.data_ptr(), n0, n1, n2, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                       "fill_holes")
    return _out(out, as_numpy)


def _mask_extent(vol):
    """The 6 ints of ``seunet_mask_box`` on the host: {min, max} per axis; max = -1 for an empty mask."""
    n0, n1, n2 = (int(v) for v in vol.shape)
    with torch.cuda.device(vol.device):
        box = torch.empty(6, dtype=torch.int32, device=vol.device)
        _lib.check(_lib.load().seunet_mask_box(vol.data_ptr(), n0, n1, n2, box.data_ptr(), _lib.stream_ptr()), "mask_box")
        return [int(v) for v in box.cpu().numpy()]


def _mask_coords(mask):
    """``np.argwhere(mask != 0)`` of a device volume, (m, 3) int64 in raster order: the bits are packed on the device
    (``seunet_mask_bits``) and only the non-zero words are unpacked on the host, so a skeleton costs its own size, not the volume's."""
    n = mask.numel()
    with torch.cuda.device(mask.device):
        bits = torch.empty((n + 63) // 64, dtype=torch.int64, device=mask.device)
        _lib.check(_lib.load().seunet_mask_bits(mask.data_ptr(), n, bits.data_ptr(), _lib.stream_ptr()), "mask_bits")
        words = bits.cpu().numpy().view(np.uint64)
    if n % 64:
        words[-1] &= np.uint64((1 << (n % 64)) - 1)
    at = np.flatnonzero(words)
    word, bit = np.nonzero(np.unpackbits(words[at].view(np.uint8).reshape(-1, 8), axis=1, bitorder="little"))
    lin = at[word].astype(np.int64) * 64 + bit
    return np.stack(np.unravel_index(lin, tuple(mask.shape)), axis=1).astype(np.int64)


def _largest_in_slice(vol, k):
    """Voxels of the largest 8-connected component of the slice ``[:, :, k]`` (0 for an empty slice)."""
    n0, n1, n2 = (int(v) for v in vol.shape)
    lib = _lib.load()
    dev = vol.device
    with torch.cuda.device(dev):
        sl = torch.empty((n0, n1, 1), dtype=torch.uint8, device=dev)
        _lib.check(lib.seunet_crop3d(vol.data_ptr(), 1, n0, n1, n2, _lib.int_array([0, n0, 0, n1, k, k + 1]), sl.data_ptr(),
                                     _lib.stream_ptr()), "crop3d")
        ws = workspace(lib.seunet_cc_workspace_bytes, n0, n1, 1, device=dev)
        comp = torch.empty((n0, n1, 1), dtype=torch.uint8, device=dev)
        _lib.check(lib.seunet_largest_component(sl.data_ptr(), n0, n1, 1, _lib.CC_EVALUATION, comp.data_ptr(), None, ws.data_ptr(),
                                                ws.numel(), _lib.stream_ptr()), "largest_component")
        return int(comp.sum(dtype=torch.int64).item())


def slice_moments(mask, k: int):
    """``(count, sum of i0, sum of i1)`` over the non-zero voxels of ``mask[:, :, k]``, exact Python ints (``seunet_slice_moments``)."""
    vol, _ = _mask_in(mask, "mask")
    n0, n1, n2 = (int(v) for v in vol.shape)
    if not 0 <= int(k) < n2:
        raise ValueError(f"seunet prep: slice_moments: slice {k} of an axis of {n2}")
    with torch.cuda.device(vol.device):
        out = torch.empty(3, dtype=torch.int64, device=vol.device)
        _lib.check(_lib.load().seunet_slice_moments(vol.data_ptr(), n0, n1, n2, int(k), out.data_ptr(), _lib.stream_ptr()), "slice_moments")
        return tuple(int(v) for v in out.cpu().numpy().view(np.uint64))


def scatter_labels(lin_index, values, shape):
    """``(cd int32, skeleton_parse uint8)`` device volumes of ``shape`` with ``cd.flat[lin_index[j]] = values[j]`` (one launch into
    zeroed volumes; every index once).  An index outside the volume raises ValueError."""
    n0, n1, n2 = (int(v) for v in shape)
    lin = torch.from_numpy(np.ascontiguousarray(lin_index, dtype=np.int64)).cuda()
    val = torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).cuda()
    if lin.shape != val.shape or lin.dim() != 1:
        raise ValueError("seunet prep: scatter_labels: lin_index and values must be 1-D and of one length")
    dev = lin.device
    with torch.cuda.device(dev):
        cd = torch.zeros((n0, n1, n2), dtype=torch.int32, device=dev)
        parse = torch.zeros((n0, n1, n2), dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().seunet_scatter_labels(_lib.ptr(lin) if lin.numel() else None, _lib.ptr(val) if val.numel() else None,
                                                     lin.numel(), cd.numel(), cd.data_ptr(), parse.data_ptr(), status.data_ptr(),
                                                     _lib.stream_ptr()), "scatter_labels")
        _status(status, "airway_parse: cd: a branch voxel lies outside the volume")
    return cd, parse


def airway_parse_stages(label, merge_t: int = 5):
    """``airway_parse`` with every intermediate result, as a dict: ``order``, ``label_trans``, ``skeleton``, ``B0`` / ``B`` (the
    sorted skeleton before / after smoothing), ``mainpart``, ``table1`` / ``merged`` (branch tables before / after merging),
    ``codes``, ``cd``, ``skeleton_parse`` and ``parsing`` (device tensors for the volumes)."""
    lab, _ = _mask_in(label, "label")
    n0, n1, n2 = (int(v) for v in lab.shape)
    box = _mask_extent(lab) if lab.numel() else [0, -1] * 3
    if box[5] < 0:
        raise ValueError("airway_parse: orientation: the mask is empty")
    k2, k8 = topology.orientation_slices(box[4], box[5])
    order = topology.orientation(_largest_in_slice(lab, k2), _largest_in_slice(lab, k8))
    closed = _morph(binary_fill_holes(_morph(lab, _lib.MORPH_DILATE, "binary_dilation")), _lib.MORPH_CLOSE, "binary_closing")
    try:
        lt = maximum_3d(closed)
    except IndexError as e:
        raise ValueError(f"airway_parse: label_trans: {e}") from None
    skel = skeletonize_3d(lt)
    coords = _mask_coords(skel)
    ext = _mask_extent(lt)
    trace = {}
    merged, codes = topology.graph_stage(coords, (n0, n1, n2), order, (ext[4], ext[5]), lambda k: slice_moments(lt, k), merge_t, trace)
    lin, val = topology.branch_labels(merged, (n0, n1, n2))
    cd, parse = scatter_labels(lin, val, (n0, n1, n2))
    parsing = _assign(parse, lab, cd)
    trace.update(order=order, label_trans=lt, skeleton=skel, cd=cd, skeleton_parse=parse, parsing=parsing)
    return trace


def airway_parse(label, merge_t: int = 5, return_branches: bool = False):
    """``ske_and_parse.airway_parse(label, merge_t)`` (ske_and_parse.py:20-65), the branch labelling the reference trains and
    evaluates with: its own parser ``Topology_Tree.sub()`` + ``.merge()`` (ours_skel_parse.py:515-619), not the ATM'22 one of
    ``tree_parsing``.  -> the int32 ``parsing`` volume ``evaluation_case`` takes.  ``label``: a byte mask, non-zero = 1 (what
    ``large_connected_domain26`` returns); it is not modified.  CUDA tensor in -> CUDA tensor out, numpy in -> numpy out.

    Dense stages on the GPU (orientation, dilation, hole fill, closing, ``maximum_3d``, ``skeletonize_3d``, the nearest-branch
    assignment), the graph stage on the host on the skeleton's voxels (``topology.py``).  Both sorts of the reference are stable
    here, and where the reference raises (an empty mask, fewer than three branches after merging, a father number past its child
    table, a voxel outside the volume) ``ValueError`` names the stage: DESIGN.md section 3g.  ``return_branches``: also the merged
    branch table, a list of dicts ``index``, ``fatherindex``, ``start``, ``member``, optionally ``end``, and the ``grade()`` code
    strings ``grade`` / ``father_grade``."""
    as_numpy = isinstance(label, np.ndarray)
    st = airway_parse_stages(label, merge_t)
    out = _out(st["parsing"], as_numpy)
    if not return_branches:
        return out
    branches = [dict(b, grade=c, father_grade=f) for b, (c, f) in zip(st["merged"], st["codes"])]
    return out, branches
