"""tests/guarded_alloc.py on the CPU device: the detector fires where it must, with the right location, and stays silent
where nothing is wrong.  (The GPU files open with the same two controls on the device.)"""
import re

import numpy as np
import pytest
import torch

import guarded_alloc as G
from guarded_alloc import RED_ZONE, check, guard, guarded_allocations, same_bits

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}


def _cpu(fill=0xFF, seed=1):
    return guarded_allocations(fill, seed, devices=("cpu",))


def _restored():
    return all(getattr(torch, n) is f for n, f in _ORIG.items())


@pytest.mark.parametrize("fill", G.FILLS)
def test_shape_forms_give_aligned_contiguous_payloads(fill):
    with _cpu(fill) as g:
        cases = [(torch.empty(5), (5,)), (torch.empty(2, 3), (2, 3)), (torch.empty((2, 3)), (2, 3)),
                 (torch.empty(size=(2, 3)), (2, 3)), (torch.empty(torch.Size([4, 1, 3]), dtype=torch.bfloat16), (4, 1, 3)),
                 (torch.empty((), dtype=torch.float64), ()), (torch.empty(0, dtype=torch.int64), (0,)),
                 (torch.zeros(3, 5, dtype=torch.int32), (3, 5)), (torch.zeros((7,), dtype=torch.uint8), (7,)),
                 (torch.empty_like(torch.ones(2, 9)), (2, 9)), (torch.zeros_like(torch.ones(3, 2), dtype=torch.float16), (3, 2))]
        for t, shape in cases:
            assert tuple(t.shape) == shape and t.is_contiguous() and t.data_ptr() % 512 == 0, (shape, t.stride(), t.data_ptr() % 512)
        assert [c[0].dtype for c in cases[4:6]] == [torch.bfloat16, torch.float64]
        assert cases[10][0].dtype == torch.float16
        assert len(g.records) == len(cases) and check() == len(cases)
        byte = {0x00: 0, 0xFF: 255}.get(fill)
        if byte is not None:
            assert bool((cases[1][0].view(torch.uint8) == byte).all())
        else:
            assert len(np.unique(torch.empty(4096, dtype=torch.uint8).numpy())) > 200
        for t in (cases[7][0], cases[8][0], cases[10][0]):                     # the zeros forms stay zero under every fill
            assert int(t.view(torch.uint8).count_nonzero()) == 0
    assert _restored()


def test_requires_grad_memory_format_and_pass_through():
    with _cpu() as g:
        t = torch.empty(2, 3, requires_grad=True)
        assert t.requires_grad and t.is_leaf
        cl = torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        assert cl.stride() == _ORIG["empty"]((2, 3, 4, 5), memory_format=torch.channels_last).stride() and cl.data_ptr() % 512 == 0
        src = torch.ones(2, 3, 4, 5).permute(0, 2, 3, 1)                       # dense, not contiguous: preserve_format keeps strides
        assert torch.empty_like(src).stride() == src.stride()
        assert torch.empty_like(src, memory_format=torch.contiguous_format).is_contiguous()
        n = len(g.records)
        out = _ORIG["empty"](4)
        assert torch.empty(4, out=out) is out                                  # out=: not served
        assert torch.empty(3, device="meta").device.type == "meta"             # another device: not served
        assert len(g.records) == n
        assert check() == n
    with guarded_allocations(0xFF, 0) as g:                                    # the default guards cuda only
        torch.empty(3)
        torch.zeros_like(torch.ones(2))
        assert len(g.records) == 0
    assert _restored()


def test_guard_copies_into_a_guarded_buffer():
    with _cpu() as g:
        src = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()         # not contiguous
        p = torch.nn.Parameter(torch.ones(5))
        a, b = guard(src), guard(p)
        assert torch.equal(a, src) and a.is_contiguous() and a.data_ptr() % 512 == 0 and a.data_ptr() != src.data_ptr()
        assert b.requires_grad and b.is_leaf and torch.equal(b.detach(), p.detach())
        assert len(g.records) == 2 and check() == 2
    with pytest.raises(RuntimeError):
        guard(torch.ones(2))
    with pytest.raises(RuntimeError):
        check()


def _offsets(msg):
    m = re.search(r"first at payload offset (-?\d+), last at payload offset (-?\d+)", msg)
    assert m, msg
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("where,zone", [("just_before", "front"), ("far_front", "front"), ("just_after", "back"), ("far_back", "back")])
def test_a_planted_byte_is_reported_with_its_offset(where, zone):
    with _cpu(0x00, seed=3) as g:
        torch.empty(8)                                                         # a clean neighbour before
        t = torch.empty((3, 5), dtype=torch.float16)                          # 30 bytes: the back zone starts unaligned
        torch.zeros(4)                                                         # and one after
        r = g.records[1]
        assert r.nbytes == 30 and r.base.data_ptr() + r.off + RED_ZONE == t.data_ptr()
        want = {"just_before": -1, "far_front": -RED_ZONE, "just_after": 30, "far_back": 30 + RED_ZONE - 1}[where]
        assert check() == 3
        r.base[r.off + RED_ZONE + want] ^= 0x5A                                # one byte, through the base buffer
        with pytest.raises(AssertionError) as e:
            check()
        msg = str(e.value)
        assert _offsets(msg) == (want, want), msg
        assert f"{zone} zone" in msg and "1 bytes changed" in msg and "allocation #1" in msg
        assert "shape=(3, 5)" in msg and "torch.float16" in msg and "test_guarded_alloc_host.py" in msg
        r.base[r.off + RED_ZONE + want] ^= 0x5A
        assert check() == 3                                                    # put back: silent again


def test_a_damaged_range_is_reported_first_to_last():
    with _cpu(seed=4) as g:
        t = torch.empty(16, dtype=torch.uint8)
        r = g.records[0]
        tail = r.base[r.off + RED_ZONE + 16:r.off + RED_ZONE + 16 + 40]
        tail.copy_(tail ^ 0xFF)
        with pytest.raises(AssertionError) as e:
            check()
        assert _offsets(str(e.value)) == (16, 55) and "40 bytes changed" in str(e.value)
        del t


def test_a_function_that_writes_exactly_its_payload_is_clean():
    def op(n):
        out = torch.empty(n, dtype=torch.int16)
        out.copy_(torch.arange(n, dtype=torch.int16))
        scratch = torch.zeros_like(out)
        scratch += out
        return out + scratch

    results = []
    for seed, fill in enumerate(G.FILLS):
        with _cpu(fill, seed) as g:
            results.append(op(1031))
            assert check() == 2
    assert same_bits(results[0], results[1]) and same_bits(results[0], results[2])


def test_a_stale_read_differs_between_fills_and_same_bits_says_where():
    def op(n):
        return {"n": n, "out": (torch.empty(n, dtype=torch.int32).sum(), torch.zeros(2))}      # reads what nobody wrote

    res = []
    for seed, fill in enumerate((0x00, 0xFF)):
        with _cpu(fill, seed):
            res.append(op(7))
            check()
    assert int(res[0]["out"][0]) == 0 and int(res[1]["out"][0]) == -7
    with pytest.raises(AssertionError, match=r"result\['out'\]\[0\]: .*0 against -7"):
        same_bits(res[0], res[1])


def test_same_bits_on_nested_results():
    class Obj:
        def __init__(self, v):
            self.words, self.count, self._last = np.array([1, 2, v], np.uint64), 3, (v, None)

    nan1 = torch.tensor([float("nan"), 1.0])
    nan2 = nan1.clone()
    assert same_bits(nan1, nan2) and same_bits((1, 2.5, "a", None, True), (1, 2.5, "a", None, True))
    assert same_bits(Obj(5), Obj(5)) and same_bits({"a": [np.float32(1.5)]}, {"a": [np.float32(1.5)]})
    nan2.view(torch.int32)[0] ^= 1                                             # another NaN payload
    with pytest.raises(AssertionError, match=r"element \(0,\)"):
        same_bits(nan1, nan2)
    with pytest.raises(AssertionError, match=r"r\[1\]\[2\]"):
        same_bits((0, [1, 2, 0.0]), (0, [1, 2, -0.0]), "r")                    # the sign of zero counts
    with pytest.raises(AssertionError, match=r"result\.words: .*element \(2,\)"):
        same_bits(Obj(5), Obj(6))
    with pytest.raises(AssertionError, match="float32"):
        same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(AssertionError, match=r"\(1, 1\)"):
        same_bits(np.zeros((2, 2)), np.array([[0.0, 0.0], [0.0, 1.0]]))
    with pytest.raises(AssertionError, match="int 1 against float 1.0"):
        same_bits(1, 1.0)


def test_the_four_names_are_restored_also_after_an_error():
    with pytest.raises(ZeroDivisionError):
        with _cpu():
            assert torch.empty is not _ORIG["empty"] and torch.zeros_like is not _ORIG["zeros_like"]
            1 / 0
    assert _restored()
    with _cpu():
        with pytest.raises(RuntimeError, match="nest"):
            with _cpu():
                pass
        assert torch.empty is not _ORIG["empty"]                                # the refused inner context took nothing down
    assert _restored() and G._active is None
