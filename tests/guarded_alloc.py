"""Dirty scratch memory and red zones for the tensors the wrappers allocate.

The Python wrappers of this package allocate every workspace, packed weight, status word and output with ``torch.empty``,
``torch.zeros``, ``torch.empty_like`` or ``torch.zeros_like`` at call time, looked up as attributes of the ``torch`` module.
``guarded_allocations(fill, seed)`` replaces those four attributes while it is active.  A call whose result would live on a
guarded device (and that has no ``out=``) is served from a larger 1-D byte buffer laid out as

    [ front red zone: 4096 B ][ payload: numel * itemsize B ][ back red zone: 4096 B ]

* The red zones hold seeded pseudo-random bytes (a constant would miss a kernel that happens to write that constant), and
  ``check()`` compares every zone handed out so far with what was recorded.
* 4096 bytes is a condition, not a measurement: a multiple of the 512-byte alignment torch itself gives, so the payload
  keeps ``data_ptr() % 512 == 0``, and four times the 1024 bytes one wave writes with 16-byte stores, so a one-row or
  one-tile overrun lands inside a zone.
* The payload of the ``empty`` forms is set by ``fill``: ``0x00``, ``0xFF`` or ``"random"`` (seeded bytes).  A kernel that
  reads scratch memory its own call did not write gives different results under different fills (``same_bits``).  The
  payload of the ``zeros`` forms stays zero -- that is the wrappers' contract with the library -- but gets red zones.
* ``guard(t)`` copies a tensor the caller made (inputs, parameters, gradients, optimizer moments) into such a buffer, so
  reads and writes beside inputs and in-out tensors are covered too.

Known limit: allocations made inside torch's C++ (``.contiguous()``, ``.clone()``, ``.to()``, ``.cuda()``, arithmetic
results) are not intercepted.  Those are fully written copies, so they cannot expose stale scratch; a store beside one of
them is not seen.

This is a plain helper module: no pytest configuration, nothing that changes how Python starts.
"""
import contextlib
import numbers
import os
import struct
import sys

import numpy as np
import torch

RED_ZONE = 4096
ALIGN = 512
FILLS = (0x00, 0xFF, "random")
_NAMES = ("empty", "zeros", "empty_like", "zeros_like")
_MEMO_ATTRS = ("_last",)          # CandidateSet's one-entry lookup cache: not part of a result
_HERE = os.path.abspath(__file__)

_active = None


class _Record:
    __slots__ = ("base", "off", "nbytes", "expect", "shape", "dtype", "site", "kind")

    def describe(self):
        return f"{self.kind} shape={tuple(self.shape)} dtype={self.dtype} at {self.site}"


class _Guard:
    def __init__(self, fill, seed, devices):
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {FILLS}, not {fill!r}")
        self.fill, self.seed = fill, int(seed)
        self.devices = tuple(torch.device(d).type for d in devices)
        self.rng = np.random.RandomState(self.seed)
        self.gens = {}
        self.records = []
        self.orig = {n: getattr(torch, n) for n in _NAMES}

    # ---- which calls are served -------------------------------------------------------------------
    def guarded(self, device):
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        return torch.device(device).type in self.devices

    # ---- the buffer ---------------------------------------------------------------------------------
    def alloc(self, shape, dtype, device, strides, zero, requires_grad, kind):
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        item = self.orig["empty"]((), dtype=dtype, device="meta").element_size()
        nbytes = numel * item
        empty = self.orig["empty"]
        base = empty(RED_ZONE + nbytes + RED_ZONE + ALIGN, dtype=torch.uint8, device=device)
        off = (-(base.data_ptr() + RED_ZONE)) % ALIGN            # torch's CPU allocator aligns to 64 bytes only
        zones = self.rng.randint(0, 256, size=2 * RED_ZONE, dtype=np.uint8)
        expect = torch.from_numpy(zones).to(base.device)
        base[off:off + RED_ZONE] = expect[:RED_ZONE]
        base[off + RED_ZONE + nbytes:off + 2 * RED_ZONE + nbytes] = expect[RED_ZONE:]
        body = base[off + RED_ZONE:off + RED_ZONE + nbytes]
        if zero or self.fill == 0x00:
            body.zero_()
        elif self.fill == 0xFF:
            body.fill_(0xFF)
        else:
            body.random_(0, 256, generator=self.generator(base.device))
        t = body.view(dtype)
        t = t.as_strided(shape, strides) if strides is not None else t.view(shape)
        if requires_grad:
            t.requires_grad_(True)
        r = _Record()
        r.base, r.off, r.nbytes, r.expect, r.shape, r.dtype, r.kind = base, off, nbytes, expect, shape, dtype, kind
        r.site = _call_site()
        self.records.append(r)
        return t

    def generator(self, device):
        key = str(device)
        if key not in self.gens:
            self.gens[key] = torch.Generator(device=device).manual_seed(self.seed)
        return self.gens[key]

    # ---- the four stand-ins ------------------------------------------------------------------------
    def plain(self, name):
        orig, zero = self.orig[name], name == "zeros"

        def fn(*size, **kw):
            if "out" in kw or kw.get("pin_memory") or kw.get("names") is not None or \
                    kw.get("layout", torch.strided) not in (None, torch.strided) or not self.guarded(kw.get("device")):
                return orig(*size, **kw)
            try:
                if "size" in kw:
                    shape = kw["size"]
                elif len(size) == 1 and not isinstance(size[0], numbers.Integral):
                    shape = size[0]
                else:
                    shape = size
                shape = tuple(int(s) for s in shape)
            except TypeError:
                return orig(*size, **kw)
            dtype = kw.get("dtype") or torch.get_default_dtype()
            mf = kw.get("memory_format")
            strides = None
            if mf not in (None, torch.contiguous_format):
                strides = self.orig["empty"](shape, dtype=dtype, device="meta", memory_format=mf).stride()
            device = kw.get("device")
            if device is None:
                device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
            return self.alloc(shape, dtype, device, strides, zero, bool(kw.get("requires_grad", False)), "torch." + name)
        fn.__name__ = fn.__qualname__ = name
        return fn

    def like(self, name):
        orig, zero = self.orig[name], name == "zeros_like"

        def fn(inp, **kw):
            if not isinstance(inp, torch.Tensor):
                return orig(inp, **kw)
            device = kw.get("device")
            if device is None:
                device = inp.device
            if "out" in kw or kw.get("pin_memory") or inp.is_sparse or \
                    kw.get("layout", torch.strided) not in (None, torch.strided) or not self.guarded(device):
                return orig(inp, **kw)
            dtype = kw.get("dtype") or inp.dtype
            mf = kw.get("memory_format", torch.preserve_format)
            meta = self.orig["empty_like"](inp, dtype=dtype, device="meta", memory_format=mf)
            strides = None if meta.is_contiguous() else meta.stride()
            return self.alloc(inp.shape, dtype, device, strides, zero, bool(kw.get("requires_grad", False)), "torch." + name)
        fn.__name__ = fn.__qualname__ = name
        return fn


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})"


@contextlib.contextmanager
def guarded_allocations(fill, seed, devices=("cuda",)):
    """Serve torch.empty / zeros / empty_like / zeros_like on ``devices`` from red-zoned buffers (module docstring).  Yields the
    guard; its ``records`` list holds one entry per allocation.  The four attributes are restored on exit, also on error."""
    global _active
    if _active is not None:
        raise RuntimeError("guarded_allocations does not nest")
    g = _Guard(fill, seed, devices)
    try:
        _active = g
        torch.empty, torch.zeros = g.plain("empty"), g.plain("zeros")
        torch.empty_like, torch.zeros_like = g.like("empty_like"), g.like("zeros_like")
        yield g
    finally:
        for n in _NAMES:
            setattr(torch, n, g.orig[n])
        _active = None


def _need():
    if _active is None:
        raise RuntimeError("no guarded_allocations context is active")
    return _active


def guard(t):
    """A copy of ``t`` inside a red-zoned buffer of the active context (same shape, dtype, device, strides of a contiguous
    tensor, requires_grad).  A tensor on a device the context does not guard is returned as it is."""
    g = _need()
    if not g.guarded(t.device):
        return t
    out = g.alloc(t.shape, t.dtype, t.device, None, True, False, "guard")
    with torch.no_grad():
        out.copy_(t)
    if t.requires_grad:
        out.requires_grad_(True)
    return out


def check():
    """Synchronise, then compare every red zone handed out so far with its recorded bytes.  Returns the number of allocations
    verified; raises AssertionError naming the allocation, the zone and the damaged byte range relative to the payload
    (negative offsets: before its first byte; the back zone starts at offset ``nbytes``)."""
    g = _need()
    if "cuda" in g.devices and torch.cuda.is_available():
        torch.cuda.synchronize()
    for i, r in enumerate(g.records):
        lo = r.off
        hi = r.off + RED_ZONE + r.nbytes
        cur = torch.cat([r.base[lo:lo + RED_ZONE], r.base[hi:hi + RED_ZONE]])
        if torch.equal(cur, r.expect):
            continue
        bad = (cur != r.expect).cpu().numpy()
        for zone, part, origin in (("front", bad[:RED_ZONE], -RED_ZONE), ("back", bad[RED_ZONE:], r.nbytes)):
            idx = np.flatnonzero(part)
            if idx.size:
                raise AssertionError(f"red zone damaged: allocation #{i} {r.describe()}, payload of {r.nbytes} bytes: {zone} zone, "
                                     f"{idx.size} bytes changed, first at payload offset {origin + int(idx[0])}, "
                                     f"last at payload offset {origin + int(idx[-1])}")
    return len(g.records)


# ---- bitwise comparison of nested results ---------------------------------------------------------------------
def _bytes_of_tensor(t):
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().reshape(-1).view(torch.uint8)


def _leaf(a, b, path):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
            raise AssertionError(f"{path}: {type(a).__name__} against {type(b).__name__}")
        if a.shape != b.shape or a.dtype != b.dtype:
            raise AssertionError(f"{path}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}")
        x, y = _bytes_of_tensor(a), _bytes_of_tensor(b.to(a.device))
        if not torch.equal(x, y):
            ne = x != y
            k = int(ne.to(torch.uint8).argmax())
            item = max(1, x.numel() // max(1, a.numel()))
            el = k // item
            where = tuple(int(v) for v in np.unravel_index(el, tuple(a.shape))) if a.dim() else ()
            av, bv = a.detach().reshape(-1)[el].item(), b.detach().reshape(-1)[el].item()
            raise AssertionError(f"{path}: {int(ne.sum())} of {x.numel()} bytes differ, first at element {where} (byte {k}): "
                                 f"{av!r} against {bv!r}")
        return
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)):
            raise AssertionError(f"{path}: {type(a).__name__} against {type(b).__name__}")
        if a.shape != b.shape or a.dtype != b.dtype:
            raise AssertionError(f"{path}: {a.shape} {a.dtype} against {b.shape} {b.dtype}")
        x, y = np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8)
        if not np.array_equal(x, y):
            k = int(np.flatnonzero(x != y)[0])
            el = k // max(1, a.dtype.itemsize)
            where = tuple(int(v) for v in np.unravel_index(el, a.shape)) if a.ndim else ()
            raise AssertionError(f"{path}: {int((x != y).sum())} of {x.size} bytes differ, first at element {where} (byte {k}): "
                                 f"{a.reshape(-1)[el]!r} against {b.reshape(-1)[el]!r}")
        return
    if isinstance(a, np.generic) or isinstance(b, np.generic):
        return _leaf(np.asarray(a), np.asarray(b), path)
    if type(a) is not type(b):
        raise AssertionError(f"{path}: {type(a).__name__} {a!r} against {type(b).__name__} {b!r}")
    if isinstance(a, float):
        if struct.pack("<d", a) != struct.pack("<d", b):
            raise AssertionError(f"{path}: {a!r} ({struct.pack('<d', a).hex()}) against {b!r} ({struct.pack('<d', b).hex()})")
        return
    if isinstance(a, complex):
        _leaf(a.real, b.real, path + ".real")
        return _leaf(a.imag, b.imag, path + ".imag")
    if a is None or isinstance(a, (bool, int, str, bytes, torch.dtype, torch.device, torch.Size)):
        if a != b:
            raise AssertionError(f"{path}: {a!r} against {b!r}")
        return
    if isinstance(a, dict):
        if list(a.keys()) != list(b.keys()):
            raise AssertionError(f"{path}: keys {list(a.keys())} against {list(b.keys())}")
        for k in a:
            _leaf(a[k], b[k], f"{path}[{k!r}]")
        return
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            raise AssertionError(f"{path}: {len(a)} items against {len(b)}")
        for i, (u, v) in enumerate(zip(a, b)):
            _leaf(u, v, f"{path}[{i}]")
        return
    if hasattr(a, "__dict__"):                                   # CandidateSet, MetricSums and the like: their attributes
        da = {k: v for k, v in vars(a).items() if k not in _MEMO_ATTRS}
        db = {k: v for k, v in vars(b).items() if k not in _MEMO_ATTRS}
        if sorted(da) != sorted(db):
            raise AssertionError(f"{path}: attributes {sorted(da)} against {sorted(db)}")
        for k in sorted(da):
            _leaf(da[k], db[k], f"{path}.{k}")
        return
    raise AssertionError(f"{path}: same_bits cannot compare {type(a).__name__}")


def same_bits(a, b, what="result"):
    """Compare two nested results (tensors, numpy arrays, tuples, lists, dicts, plain objects through their attributes, Python
    scalars) bit for bit -- floats through integer views, so NaN payloads and the sign of zero count.  Returns True; raises
    AssertionError naming the first differing leaf."""
    _leaf(a, b, what)
    return True


# ---- the pattern of the GPU files ---------------------------------------------------------------------------------
VERIFIED = {}     # family -> [operations run under the guard, guarded allocations check() verified] (for the run's report)


def three_fills(op, family="", devices=("cuda",)):
    """Run ``op()`` once under each fill (0x00, 0xFF, random), each run with red-zone seeds of its own.  ``op`` makes its
    inputs itself and passes them through ``guard()``.  Asserts (a) ``check()`` after each run and (b) that the three results
    are ``same_bits``; returns the first result."""
    results = []
    for seed, fill in enumerate(FILLS):
        with guarded_allocations(fill, 1000 + seed, devices):
            results.append(op())
            n = check()
        tally = VERIFIED.setdefault(family, [0, 0])
        tally[1] += n
    VERIFIED[family][0] += 1
    same_bits(results[0], results[1], f"{family}: fill 0x00 against fill 0xFF")
    same_bits(results[0], results[2], f"{family}: fill 0x00 against random fill")
    return results[0]
