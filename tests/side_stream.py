"""Run an operation on a side stream, behind a producer that is still busy when the operation is called.

Every entry point of the library takes a stream, and the Python wrappers pass ``torch.cuda.current_stream()``.  On the default
stream a launch, memset or copy that goes to stream 0 instead, or a host read that waits for another stream than the one the
work is on, gives the right answer all the same.  ``run_behind_delay`` makes such a mistake visible:

1. the input buffers are allocated on the default stream and filled with **poison** -- another valid input of the same shapes
   and types (another seed, another fixture case), never bytes the operation would reject -- and the device is synchronised;
2. a fresh ``torch.cuda.Stream()`` (non-blocking: the default stream does not wait for it) becomes current; on it a
   ``torch.cuda._sleep(cycles)`` is queued, the event ``gate`` is recorded, and only then ``buf.copy_(real)`` for each input;
3. ``gate.query()`` must be False: the real data does not exist yet when the operation is called;
4. the operation runs under that stream;
5. for operations documented as not synchronising the host, ``gate.query()`` must still be False when the call returns;
6. the stream is synchronised and the results (tensors and whatever Python values the operation read back) are returned.

Work that ran on another stream, or a host read that did not wait for the side stream, has seen the poison; the caller compares
the results with expected values bit for bit (``guarded_alloc.same_bits``).

``calibrate()`` times one ``_sleep`` with two events and scales it to ``DELAY_MS``.  That figure is a condition, not a
measurement: what matters are the two ``gate.query()`` asserts, and ``ENQUEUE_MS`` keeps the host time every delayed call that
must not wait took, so that the figure can be judged against it (tests/test_streams_gpu.py: 5.9 ms at the most on an MI355X).

This is a plain helper module: no pytest configuration, nothing that changes how Python starts."""
import time

import numpy as np
import torch

DELAY_MS = 50.0
ENQUEUE_MS = {}              # label -> host milliseconds from the gate's record to the operation's return, the longest seen
_CAL = {}                    # device index -> (cycles per millisecond)


def calibrate(target_ms=None):
    """``_sleep`` cycles for ``target_ms`` (default ``DELAY_MS``) on the current device, from one timed ``_sleep`` per process."""
    target_ms = DELAY_MS if target_ms is None else target_ms
    dev = torch.cuda.current_device()
    if dev not in _CAL:
        probe = 20_000_000
        torch.cuda._sleep(1000)                                  # (the kernel's one-time load is not part of the timing)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.0, ms
        _CAL[dev] = probe / ms
    return int(_CAL[dev] * target_ms)


def to_device(v):
    """A host tensor or array as a new device tensor (a device tensor is cloned); None stays None."""
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v))
    return v.cuda() if not v.is_cuda else v.clone()


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def check_poison(real, poison):
    """Same count, shapes and types, and at least one input whose bits differ: the poison is another input, not the same one."""
    assert len(real) == len(poison), (len(real), len(poison))
    differ = False
    for i, (r, p) in enumerate(zip(real, poison)):
        assert (r is None) == (p is None), i
        if r is None:
            continue
        assert r.shape == p.shape and r.dtype == p.dtype, (i, tuple(r.shape), r.dtype, tuple(p.shape), p.dtype)
        differ = differ or not torch.equal(_bits(r), _bits(p))
    assert differ, "the poison equals the real inputs"


class Delayed:
    """One side stream with a pending delay in front of the real inputs: step 1 of the module docstring in ``__init__``, steps
    2-3 in ``open``, 4-5 in ``call``, 6 in ``finish``.  Several can be open at once (make them all, then open them all): each
    has a stream and a gate of its own."""

    def __init__(self, make_inputs, poison_inputs, cycles=None, label=""):
        self.label = label
        self.real = [to_device(v) for v in make_inputs()]
        self.bufs = [to_device(v) for v in poison_inputs()]
        check_poison(self.real, self.bufs)
        self.cycles = calibrate() if cycles is None else int(cycles)
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream()
        self.gate = torch.cuda.Event()

    def open(self):
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(self.cycles)
            self.gate.record()
            self.t0 = time.perf_counter()
            for buf, real in zip(self.bufs, self.real):
                if buf is not None:
                    buf.copy_(real, non_blocking=True)
        self.assert_pending("before the operation is called")
        return self

    def assert_pending(self, when):
        ms = (time.perf_counter() - self.t0) * 1e3
        assert self.gate.query() is False, (f"{self.label}: gate.query() is True {when}, {ms:.2f} ms of host time after the delay was "
                                            f"queued: the delay was over, or the host has waited for the stream")

    def call(self, op, no_host_sync=False):
        with torch.cuda.stream(self.stream):
            out = op(*self.bufs)
        ms = (time.perf_counter() - self.t0) * 1e3
        if no_host_sync:
            ENQUEUE_MS[self.label] = max(ENQUEUE_MS.get(self.label, 0.0), ms)
            self.assert_pending("when the operation returned")
        return out

    def finish(self):
        self.stream.synchronize()


def run_behind_delay(make_inputs, poison_inputs, op, no_host_sync=False, cycles=None, label=""):
    """``op(*buffers)`` under a fresh side stream whose buffers receive ``make_inputs()`` only after a delay; until then they hold
    ``poison_inputs()``.  Both callables return a list of host (or device) tensors / numpy arrays / None.  Returns ``op``'s result
    after synchronising the side stream.  ``no_host_sync``: ``op`` is documented not to wait for the device, and the delay must
    still be pending when it returns."""
    d = Delayed(make_inputs, poison_inputs, cycles, label or getattr(op, "__name__", "op"))
    try:
        return d.open().call(op, no_host_sync)
    finally:
        d.finish()
