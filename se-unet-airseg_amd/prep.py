"""Stage-2 / stage-3 preparation on the GPU: exact EDT, hard-mining candidate sets, LIB weight and break weight.

The reference computes these on the CPU with scipy / skimage / cc3d (data.py:304-306, 455-458 on every stage-2/3
``__getitem__``; lib_weight.py:12-17, 36-53 and weight_br.py:113-177 once per case).  Here they are HIP kernels
(csrc/edt.hip) on volumes resident in HBM; the candidate lists are bit-packed masks downloaded once per case and indexed on
the host, so a draw costs no device synchronisation.  Masks are uint8 volumes with non-zero = 1; there is no CPU path."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

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
    if int(status.item()) != 0:
        raise ValueError(f"seunet prep: {what}")


def distance_transform_edt(volume: torch.Tensor, return_distances: bool = True, return_indices: bool = False,
                           return_sqdist: bool = False):
    """``scipy.ndimage.distance_transform_edt(volume, return_indices=...)`` with unit sampling, on the GPU: for every voxel
    the distance to the nearest zero voxel.  ``dist`` (float64) and ``indices`` (int32, (3, n0, n1, n2)) are bitwise
    scipy's, ties included; ``sqdist`` is the int32 squared distance.  Returns the requested outputs in the order
    (sqdist, dist, indices), a single tensor when one is requested.  A volume with no zero voxel raises ValueError."""
    vol = _vol(volume, "volume")
    if not (return_distances or return_indices or return_sqdist):
        raise ValueError("seunet prep: at least one of return_distances / return_indices / return_sqdist must be set")
    n0, n1, n2 = (int(v) for v in vol.shape)
    lib = _lib.load()
    dev = vol.device
    with torch.cuda.device(dev):
        ws_bytes = lib.seunet_edt_workspace_bytes(n0, n1, n2)
        ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=dev)
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
    as_numpy = isinstance(volume, np.ndarray)
    if as_numpy:
        if volume.ndim != 3:
            raise ValueError(f"seunet prep: `volume` must be (n0, n1, n2), got {tuple(volume.shape)}")
        if not torch.cuda.is_available():
            raise RuntimeError("seunet prep: `volume` needs a GPU (there is no CPU path)")
        vol = torch.from_numpy(np.ascontiguousarray(volume != 0).view(np.uint8)).cuda()
    else:
        vol = _vol(volume, "volume")
    n0, n1, n2 = (int(v) for v in vol.shape)
    dev = vol.device
    out = torch.zeros((n0, n1, n2), dtype=torch.uint8, device=dev)
    passes = torch.zeros(1, dtype=torch.int32, device=dev)
    if vol.numel():
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws_bytes = int(lib.seunet_skeleton_workspace_bytes(n0, n1, n2))
            if ws_bytes == 0:
                raise ValueError(f"seunet prep: skeletonize_3d: {_lib.last_error()}")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.seunet_skeletonize(vol.data_ptr(), n0, n1, n2, out.data_ptr(), passes.data_ptr(), ws.data_ptr(), ws_bytes,
                                              _lib.stream_ptr()), "skeletonize")
    skel = out.cpu().numpy() if as_numpy else out
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
        ws = torch.empty(int(lib.seunet_lib_weight_workspace_bytes(n0, n1, n2)), dtype=torch.uint8, device=label.device)
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
        ws = torch.empty(int(lib.seunet_break_weight_workspace_bytes(n0, n1, n2)), dtype=torch.uint8, device=dev)
        w = torch.empty((n0, n1, n2), dtype=torch.float16, device=dev)
        brs = torch.empty((n0, n1, n2), dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.seunet_break_weight(label.data_ptr(), pred.data_ptr(), skeleton.data_ptr(), n0, n1, n2, w.data_ptr(),
                                           brs.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                   "break_weight")
        _status(status, "break_weight: the skeleton is empty")
    return w, brs
