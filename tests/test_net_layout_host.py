"""Workspace layout of the whole-network executor as the library reports it (host only, no GPU).

``Plan::take`` (csrc/net.cpp) carves every intermediate of the network out of one caller-owned workspace and logs each take;
``seunet_debug_net_layout`` reports that log: the workspace's buffers in the order taken, then the separate input-gradient
scratch's under ``ig:`` names.  Checked here: the buffers tile the workspace, the totals are the ones the queries answer, the
placement facts the kernels rely on (``src_dist``, dc5's adjacent sources), which optional buffers exist for which descriptor,
and the workspace sizes, recorded from the library when the plan was still a list of anonymous offsets.

The descriptors: the twelve of tests/test_route_host.py; ``n_classes`` 3 with a recomputed and with a materialised x-branch;
the naive kernels with 2 and 3 input channels; ragged extents; and the one whose two-source blocks are more than 4 GB apart."""
import ctypes as C

import pytest

from test_route_host import DESCS as ROUTE_DESCS, GATED

NAIVE = 1
# (batch, in_channel, n_classes, (d, h, w), width, dtype, impl) -> seunet_net_workspace_bytes, recorded
RECORDED = {
    (4, 2, 1, (128,) * 3, 1, "bf16", 0): 11276056832, (4, 2, 1, (128,) * 3, 1, "fp16", 0): 11276056832,
    (4, 2, 1, (128,) * 3, 1, "fp32", 0): 22218887424, (1, 2, 1, (64,) * 3, 1, "bf16", 0): 413430016,
    (1, 2, 1, (64,) * 3, 1, "fp16", 0): 413430016, (1, 2, 1, (64,) * 3, 1, "fp32", 0): 761383168,
    (2, 2, 1, (32,) * 3, 1, "bf16", 0): 151843584, (1, 2, 1, (160,) * 3, 2, "bf16", 0): 10866605568,
    (2, 2, 1, (160,) * 3, 2, "bf16", 0): 21652321024, (2, 2, 1, (160,) * 3, 2, "fp16", 0): 21652321024,
    (1, 3, 1, (64,) * 3, 1, "bf16", 0): 450763264, (4, 3, 1, (128,) * 3, 1, "fp16", 0): 12478484992,
    (2, 2, 3, (32,) * 3, 1, "fp32", 0): 249407488, (1, 3, 3, (32,) * 3, 1, "bf16", 0): 114833920,
    (1, 2, 1, (64,) * 3, 1, "bf16", NAIVE): 450818560, (1, 3, 1, (64,) * 3, 1, "fp32", NAIVE): 836989440,
    (1, 1, 1, (40, 48, 56), 1, "fp16", 0): 206767872, (16, 2, 1, (128,) * 3, 2, "bf16", 0): 88360569088,
}
DESCS = list(RECORDED)
# the two-source blocks and the ops that write their sources (reference SE_UNet.py:203-229), in source order
SOURCES = {"dc1": ("up0", "ec93"), "dc22": ("dc2", "dc1"), "dc3": ("up1", "ec63"), "dc42": ("dc4", "dc3"), "dc5": ("up2", "ec33")}
POOLS = ["pool0", "pool1", "pool2"]


def up(v, a=256):
    return (v + a - 1) // a * a


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    _lib.load()
    assert _lib.CONV_NAIVE == NAIVE
    return _lib


def make(L, desc):
    from seunet_amd.SE_UNet import make_desc
    batch, inch, k, (d, h, w), width, dtype, impl = desc
    return make_desc(batch, inch, k, d, h, w, width, L.dtype_code(dtype), impl, 0.01)


def hook(L):
    f = L.load().seunet_debug_net_layout                     # diagnostic export, not in the public header
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    return f


def layout(L, desc):
    """([(name, offset, bytes)] of the workspace, the same of the input-gradient scratch), each in the order taken."""
    f, nd = hook(L), make(L, desc)
    name, off, nbytes = C.create_string_buffer(64), C.c_size_t(), C.c_size_t()
    spans = []
    while f(C.byref(nd), len(spans), name, 64, C.byref(off), C.byref(nbytes)) == 0:
        spans.append((name.value.decode(), int(off.value), int(nbytes.value)))
    assert len({n for n, _, _ in spans}) == len(spans)       # one name per buffer
    ws = [s for s in spans if not s[0].startswith("ig:")]
    assert spans[:len(ws)] == ws                             # the scratch's entries come last
    return ws, spans[len(ws):]


def assert_tiles(spans, total, what):
    """Ascending, 256-byte aligned, each buffer starting where the one before it ended (rounded up), ending at `total`."""
    assert spans and spans[0][1] == 0, what
    for (name, off, nbytes), (_, nxt, _) in zip(spans, spans[1:] + [("end", total, 0)]):
        assert off % 256 == 0, (what, name)
        assert up(off + nbytes) == nxt, (what, name)


def test_descriptors_are_the_route_tests_and_the_listed_extras():
    assert DESCS[:12] == [(b, i, 1, (s,) * 3, w, dt, 0) for b, i, s, w, dt in ROUTE_DESCS] and len(DESCS) == 18


@pytest.mark.parametrize("desc", DESCS, ids=str)
def test_buffers_tile_the_workspace_and_the_scratch(L, desc):
    lib, nd = L.load(), make(L, desc)
    batch, inch, _, (d, h, w), _, _, _ = desc
    ws, ig = layout(L, desc)
    total = int(lib.seunet_net_workspace_bytes(C.byref(nd)))
    assert total == RECORDED[desc]
    assert_tiles(ws, total, desc)
    # the input-gradient scratch: one f32 [N][V_l][in_channel] term per level 0 .. 2, a buffer of its own
    assert [n for n, _, _ in ig] == ["ig:gx:0", "ig:gx:1", "ig:gx:2"]
    assert [b for _, _, b in ig] == [batch * (d >> l) * (h >> l) * (w >> l) * inch * 4 for l in range(3)]
    assert_tiles(ig, int(lib.seunet_net_input_grad_bytes(C.byref(nd))), desc)


@pytest.mark.parametrize("desc", DESCS, ids=str)
def test_two_source_blocks_are_where_conv_info_says(L, desc):
    from seunet_amd.SE_UNet import conv_plan
    ws, _ = layout(L, desc)
    at = {n: (off, nbytes) for n, off, nbytes in ws}
    plan = {c["name"]: c for c in conv_plan(make(L, desc))}
    assert sorted(n for n, c in plan.items() if len(c["src_c"]) == 2) == sorted(SOURCES)
    for block, (a, b) in SOURCES.items():
        assert at["out:" + b][0] - at["out:" + a][0] == plan[block]["src_dist"], (desc, block)
    # dc5's sources are placed next to each other, ec33's output first (one 32-bit descriptor reaches both)
    assert at["out:up2"][0] == up(sum(at["out:ec33"]))


@pytest.mark.parametrize("desc", DESCS, ids=str)
def test_optional_buffers_exist_exactly_when_their_path_runs(L, desc):
    _, inch, k, _, _, _, impl = desc
    names = {n for n, _, _ in layout(L, desc)[0]}
    # a max-pool written by its aggregation block's epilogue keeps arg-max words: the recomputed x-branch, <= 2 input channels
    fused = inch <= 2 and impl != NAIVE
    assert {n for n in names if n.startswith("argmax:")} == ({"argmax:" + p for p in POOLS} if fused else set())
    assert {n for n in names if n.startswith("xtot:")} == ({"xtot:x33", "xtot:x63", "xtot:x93"} if fused else set())
    assert {n for n in names if n.startswith(("raw:x", "wp_f:x"))} == (set() if fused else {f"{w}:x{b}" for w in ("raw", "wp_f") for b in (33, 63, 93)})
    # the side maps of the general head path: n_classes > 1
    side = {"side:" + b for b in GATED} | {"gside", "cls_part", "cls_bias"}
    assert names & side == (side if k > 1 else set())
    assert {n for n in names if n.startswith("side:")} <= side


def test_bad_descriptor_and_index_out_of_range(L):
    f = hook(L)
    name, off, nbytes = C.create_string_buffer(64), C.c_size_t(), C.c_size_t()
    good = (1, 2, 1, (64,) * 3, 1, "bf16", 0)
    ws, ig = layout(L, good)
    nd = make(L, good)
    n = len(ws) + len(ig)
    assert f(C.byref(nd), n - 1, name, 64, C.byref(off), C.byref(nbytes)) == 0 and name.value == b"ig:gx:2"
    assert f(C.byref(nd), n, name, 64, C.byref(off), C.byref(nbytes)) != 0
    assert f(C.byref(nd), -1, name, 64, C.byref(off), C.byref(nbytes)) != 0
    bad = make(L, (1, 2, 1, (100, 64, 64), 1, "bf16", 0))
    assert f(C.byref(bad), 0, name, 64, C.byref(off), C.byref(nbytes)) != 0 and "multiples of 8" in L.last_error()
