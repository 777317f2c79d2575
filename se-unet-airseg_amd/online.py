"""Online hard mining of the reference's stage-2 / stage-3 loops, kept in HBM.

The reference (train.py:442-453, :249-261) turns every sample's loss into a file name, copies the batch to the host and keeps
the ``limits`` samples with the largest loss as ``.npy`` files (``save_data_online`` / ``save_data_online3``, train.py:78-138);
after the epoch ``OnlineHMData`` / ``OnlineHMData3`` (data.py:586-630) reload them and they are replayed one sample per step
in shuffled order (train.py:469-491, :276-303).  ``OnlineHardPool`` is that mechanism on the device: ``add`` is two launches
and no synchronise, ``replay`` synchronises once and then gathers its batches from the pool.

Differences from the reference: equal keys are evicted oldest first and never overwrite each other (there:
one file name, and ``os.listdir`` order); a NaN or infinite key is skipped (there it corrupts the sorted list).

Under one-process-per-GPU data parallelism every rank keeps a pool of its own; the ranks must agree on the number of replay
steps themselves (for instance an all-reduce MIN of ``len(pool)``), or the gradient exchange hangs.
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional

import torch

from . import _lib

MAX_ADD = 1024        # samples per add() call (SEUNET_POOL_MAX_BATCH)
MAX_REPLAY = 32       # samples per replay batch (SEUNET_POOL_MAX_GATHER)


def replay_order(keys, seq, rate: float) -> List[int]:
    """Slots in the order ``OnlineHMData.__init__`` leaves its ``name_list``: ascending by (key, seq), then the last
    ``int(rate * n)`` of them taken literally as ``order[-int(rate * n):]`` (data.py:592) -- a product of 0 selects everything."""
    order = sorted(range(len(keys)), key=lambda i: (float(keys[i]), int(seq[i])))
    return order[-int(rate * len(order)):]


class OnlineHardPool:
    """The ``limit`` hardest samples seen since ``clear()``, resident on the device.

    Storage, allocated once: data (K, 2, V) f32, weight (K, 1, V) f32, label (K, 1, V) u8, optionally skel (K, 1, V) u8,
    keys (K) f32, seq (K) i64, state (2) i64 = {count, next sequence number}; V = cube^3 (``cube`` may also be a (d, h, w)
    triple; V must be a multiple of 16).  f32 is what the reference saves for
    data and weight (the weight is w^(U+2) with a random U, so it cannot be rebuilt from the case); label and skeleton must
    hold 0.0 and 1.0 only and are kept as bytes (the reference stores int8)."""

    def __init__(self, limit: int, cube: int = 128, with_skel: bool = False, device=None):
        limit = int(limit)
        if limit < 0 or limit > 65535:
            raise ValueError(f"OnlineHardPool: limit {limit} (0..65535)")
        shape = (int(cube),) * 3 if isinstance(cube, int) else tuple(int(c) for c in cube)      # (a (d, h, w) triple also serves)
        if len(shape) != 3 or min(shape) < 1 or (shape[0] * shape[1] * shape[2]) % 16:
            raise ValueError(f"OnlineHardPool: cube {cube!r}: the voxels of a sample must be a positive multiple of 16")
        voxels = shape[0] * shape[1] * shape[2]
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("OnlineHardPool lives in GPU memory (no CPU fallback)")
        self.limit, self.shape, self.voxels, self.with_skel, self.device = limit, shape, voxels, bool(with_skel), device
        self.data = torch.empty((limit, 2, voxels), dtype=torch.float32, device=device)
        self.weight = torch.empty((limit, 1, voxels), dtype=torch.float32, device=device)
        self.label = torch.empty((limit, 1, voxels), dtype=torch.uint8, device=device)
        self.skel = torch.empty((limit, 1, voxels), dtype=torch.uint8, device=device) if with_skel else None
        self.keys = torch.empty(limit, dtype=torch.float32, device=device)
        self.seq = torch.empty(limit, dtype=torch.int64, device=device)
        self.state = torch.zeros(2, dtype=torch.int64, device=device)
        self._slots = torch.empty(MAX_ADD, dtype=torch.int32, device=device)
        # pinned landing places of replay()'s one download
        self._h_keys = torch.empty(limit, dtype=torch.float32, pin_memory=True)
        self._h_seq = torch.empty(limit, dtype=torch.int64, pin_memory=True)
        self._h_state = torch.empty(2, dtype=torch.int64, pin_memory=True)

    def clear(self) -> None:
        """The per-epoch reset (train.py:404-414, :205-217 empty the directory): zeroes ``state``, frees nothing."""
        self.state.zero_()

    def __len__(self) -> int:
        """Samples stored (one synchronise)."""
        return int(self.state[0].item())

    def _sample_tensor(self, t, channels, batch, what):
        if not (torch.is_tensor(t) and t.is_cuda and t.device == self.device):
            raise ValueError(f"OnlineHardPool.add: {what} must be a tensor on {self.device}")
        if t.dim() < 1 or t.shape[0] != batch or t.numel() != batch * channels * self.voxels:
            raise ValueError(f"OnlineHardPool.add: {what} of shape {tuple(t.shape)} is not ({batch}, {channels}) + {self.shape}")
        return t.detach().to(torch.float32).contiguous()

    def add(self, keys, data, label, weight, skel=None):
        """Offer a batch: ``keys`` (B,) f32 (``per_sample_loss``), ``data`` (B, 2, d, h, w), ``label`` / ``weight`` /
        ``skel`` (B, 1, d, h, w) f32 on the pool's device.  One select launch and one scatter launch on the current stream; no
        synchronise.  Returns the (B,) int32 device tensor of the slots taken (-1: not stored), valid until the next ``add``."""
        if not (torch.is_tensor(keys) and keys.is_cuda and keys.device == self.device and keys.dim() == 1):
            raise ValueError(f"OnlineHardPool.add: keys must be a 1-D tensor on {self.device}")
        batch = keys.numel()
        if batch < 1 or batch > MAX_ADD:
            raise ValueError(f"OnlineHardPool.add: {batch} samples per call (1..{MAX_ADD})")
        if (skel is not None) != self.with_skel:
            raise ValueError("OnlineHardPool.add: a skeleton is passed exactly when the pool was made with_skel=True")
        keys = keys.detach().to(torch.float32).contiguous()
        data = self._sample_tensor(data, 2, batch, "data")
        label = self._sample_tensor(label, 1, batch, "label")
        weight = self._sample_tensor(weight, 1, batch, "weight")
        skel = self._sample_tensor(skel, 1, batch, "skel") if self.with_skel else None
        lib = _lib.load()
        slots = self._slots[:batch]
        with torch.cuda.device(self.device):
            stream = _lib.stream_ptr()
            _lib.check(lib.seunet_pool_select(keys.data_ptr(), batch, _lib.ptr(self.keys) or None, _lib.ptr(self.seq) or None,
                                              self.state.data_ptr(), self.limit, slots.data_ptr(), stream), "pool_select")
            if self.limit > 0:
                _lib.check(lib.seunet_pool_scatter(slots.data_ptr(), batch, self.limit, self.voxels, data.data_ptr(), label.data_ptr(),
                                                   weight.data_ptr(), _lib.ptr(skel), self.data.data_ptr(), self.label.data_ptr(),
                                                   self.weight.data_ptr(), _lib.ptr(self.skel), stream), "pool_scatter")
        return slots

    def gather(self, slots) -> Dict[str, torch.Tensor]:
        """The samples in ``slots`` (host ints, at most 32) as the f32 tensors train.py:479-481 builds: ``data``
        (n, 2, d, h, w), ``label`` / ``weight`` [/ ``skel``] (n, 1, d, h, w).  No synchronise."""
        slots = [int(v) for v in slots]
        n = len(slots)
        if n < 1 or n > MAX_REPLAY:
            raise ValueError(f"OnlineHardPool.gather: {n} samples per call (1..{MAX_REPLAY})")
        out = {"data": torch.empty((n, 2) + self.shape, dtype=torch.float32, device=self.device),
               "label": torch.empty((n, 1) + self.shape, dtype=torch.float32, device=self.device),
               "weight": torch.empty((n, 1) + self.shape, dtype=torch.float32, device=self.device)}
        if self.with_skel:
            out["skel"] = torch.empty((n, 1) + self.shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().seunet_pool_gather(_lib.int_array(slots), n, self.limit, self.voxels, self.data.data_ptr(),
                                                      self.label.data_ptr(), self.weight.data_ptr(), _lib.ptr(self.skel),
                                                      out["data"].data_ptr(), out["label"].data_ptr(), out["weight"].data_ptr(),
                                                      _lib.ptr(out.get("skel")), _lib.stream_ptr()), "pool_gather")
        return out

    def snapshot(self):
        """(keys, seq) of the stored samples as host tensors of ``len(pool)`` entries (one synchronise)."""
        with torch.cuda.device(self.device):
            self._h_keys.copy_(self.keys, non_blocking=True)
            self._h_seq.copy_(self.seq, non_blocking=True)
            self._h_state.copy_(self.state, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        count = int(self._h_state[0])
        return self._h_keys[:count].clone(), self._h_seq[:count].clone()

    def replay(self, batch_size: int = 1, rate: float = 1.0, generator: Optional[torch.Generator] = None) -> Iterator[Dict[str, torch.Tensor]]:
        """The replay pass after an epoch (OnlineHMData + DataLoader(shuffle=True, drop_last=True), train.py:469-477): one
        synchronise at its start to download keys, seq and the count, none afterwards.  The stored samples are sorted ascending
        by (key, seq), the last ``int(rate * n)`` kept (``replay_order``), permuted with ``torch.randperm(n, generator=
        generator)`` and yielded ``batch_size`` at a time as dicts of ``gather``; the incomplete last batch is dropped.  Do not
        ``add`` or ``clear`` before the iterator is exhausted: the batches are read from the pool as they are asked for."""
        batch_size = int(batch_size)
        if batch_size < 1 or batch_size > MAX_REPLAY:
            raise ValueError(f"OnlineHardPool.replay: batch_size {batch_size} (1..{MAX_REPLAY})")
        keys, seq = self.snapshot()
        chosen = replay_order(keys.tolist(), seq.tolist(), rate)
        perm = torch.randperm(len(chosen), generator=generator).tolist()
        for j in range(len(chosen) // batch_size):
            yield self.gather([chosen[p] for p in perm[j * batch_size:(j + 1) * batch_size]])
