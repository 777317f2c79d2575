"""Workspace layout of the volume operations as the library reports it (host only, no GPU).

Every volume operation (largest component, lung field, EDT, LIB / break weight, skeleton, skeleton branches, double threshold)
takes one caller-allocated workspace.  csrc/volume.h holds one layout per operation: the ``seunet_*_workspace_bytes`` query
walks it over a null base, the launcher walks it over the workspace, and ``seunet_debug_volume_layout`` reports the same walk.
The byte counts below were recorded from the library when each query still held a formula of its own next to the launcher's
pointer arithmetic; a change of that layer must leave all of them where they are.  They are checked a second time against
the closed forms, computed here from the extents alone.

The shapes: one voxel, fewer than 256 voxels, rows that end just below and just above a 64-voxel word, voxel counts that are
no multiple of 256, rows longer than 256, more than 256 rows, the benchmark-sized volumes and a whole CT."""
import ctypes as C

import pytest

SHAPES = [(1, 1, 1), (3, 4, 5), (9, 8, 63), (9, 8, 65), (5, 40, 37), (3, 5, 257), (2, 129, 3), (17, 5, 130), (64, 64, 64), (96, 80, 72),
          (176, 200, 24), (512, 512, 320)]

# query -> bytes per shape, recorded
BYTES = {
    "cc": [768, 768, 36608, 38144, 59648, 31488, 6912, 88832, 2097408, 4423936, 6758656, 671088896],
    "get_l": [1280, 1280, 37888, 40192, 60928, 38144, 7424, 92416, 2098688, 4425984, 6759168, 671096320],
    "edt": [1280, 1280, 55040, 56832, 89088, 47360, 10496, 133376, 3145728, 6635520, 10137600, 1006632960],
    "lib_weight": [512, 512, 9216, 9728, 14848, 8192, 2048, 22528, 524288, 1105920, 1689600, 167772160],
    "break_weight": [3328, 3328, 114688, 119296, 185856, 99328, 22528, 278528, 6553856, 13824256, 21120256, 2097152256],
    "skeleton_branches": [1024, 1024, 41216, 43008, 67072, 35584, 7936, 100096, 2363392, 4985344, 7616512, 756285440],
    "dti": [16, 192, 1152, 2304, 3200, 1200, 4128, 4080, 65536, 245760, 563200, 20971520],
    "skeleton": [1536, 3072, 9728, 12544, 23808, 7424, 41216, 18432, 347136, 894976, 2870784, 54871040],
    "parse_assign": [1280, 1280, 55040, 56832, 89088, 47360, 10496, 133376, 3145728, 6635520, 10137600, 1006632960],
}
# op code of seunet_debug_volume_layout, sub-buffers, alignment of each
OPS = {"cc": (0, 3, 256), "get_l": (1, 5, 256), "edt": (2, 5, 256), "lib_weight": (3, 2, 256), "break_weight": (4, 9, 256),
       "skeleton_branches": (5, 4, 256), "dti": (6, 2, 8), "skeleton": (7, 6, 256), "parse_assign": (8, 5, 256)}

# (2048, 2048, 512) = 2^31 voxels: only the two queries that check the voxel count answer 0; the others size it (recorded)
BYTES_2G = {"cc": 17179869440, "get_l": 17179881472, "edt": 25769803776, "lib_weight": 4294967296, "break_weight": 53687091456,
            "skeleton_branches": 0, "dti": 536870912, "skeleton": 0, "parse_assign": 25769803776}
# an extent of 32768 is past what the EDT's int16 features hold; the launchers refuse it ("32767"), the queries size it (recorded)
EDT_FAMILY = ["edt", "lib_weight", "break_weight", "parse_assign"]
SHAPES_32768 = [(32768, 1, 1), (1, 32768, 2), (4, 4, 32768)]
BYTES_32768 = {"edt": [393216, 786432, 6291456], "lib_weight": [65536, 131072, 1048576],
               "break_weight": [819456, 1638656, 13107456], "parse_assign": [393216, 786432, 6291456]}


def up(v, a=256):
    return (v + a - 1) // a * a


def skeleton_words(s):
    w = (s[2] + 63) // 64
    return (s[0] + 2) * (s[1] + 2) * (w + 2), s[0] * s[1] * w        # padded words, words that hold voxels


def sub_buffers(name, s):
    """Bytes of each sub-buffer before its padding, in workspace order, from the extents alone."""
    n = s[0] * s[1] * s[2]
    edt = [2 * n, 2 * n, 2 * n, 2 * n, 4 * n]
    if name == "cc":
        return [4 * n, 4 * n, 32]
    if name == "get_l":
        return [4 * n, 4 * n] + [8 * s[2]] * 3
    if name in ("edt", "parse_assign"):
        return edt
    if name == "lib_weight":
        return [n, n]
    if name == "break_weight":
        return [sum(up(b) for b in edt), 4 * n, 4 * n, n, n, n, n, n, 8]
    if name == "skeleton_branches":
        return [4 * n, 4 * n, n, 4 * ((n + 255) // 256)]
    if name == "dti":
        return [8 * s[0] * s[1] * ((s[2] + 63) // 64)] * 2
    padded, words = skeleton_words(s)
    return [64, 8 * padded, 8 * padded, 8 * padded, 4 * words, 4 * words]


def closed_form(name, s):
    """The totals as the operations' documentation states them."""
    n = s[0] * s[1] * s[2]
    a4, a2, a1 = up(4 * n), up(2 * n), up(n)
    if name == "cc":
        return 2 * a4 + 256
    if name == "get_l":
        return 2 * a4 + 3 * up(8 * s[2])
    if name in ("edt", "parse_assign"):
        return 4 * a2 + a4
    if name == "lib_weight":
        return 2 * a1
    if name == "break_weight":
        return 4 * a2 + a4 + 2 * a4 + 5 * a1 + 256
    if name == "skeleton_branches":
        return 2 * a4 + a1 + up(4 * ((n + 255) // 256))
    if name == "dti":
        return 2 * s[0] * s[1] * ((s[2] + 63) // 64) * 8
    padded, words = skeleton_words(s)
    return 256 + 3 * up(8 * padded) + 2 * up(4 * words)


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    _lib.load()
    return _lib


def query(L, name, s):
    f = getattr(L.load(), f"seunet_{name}_workspace_bytes")
    f.restype, f.argtypes = C.c_size_t, [C.c_int] * 3
    return int(f(*s))


def layout(L, name, s):
    f = L.load().seunet_debug_volume_layout                  # diagnostic export, not in the public header
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t), C.c_int]
    buf = (C.c_size_t * 32)()
    count = f(OPS[name][0], s[0], s[1], s[2], buf, 16)
    return count, [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(max(count, 0))]


@pytest.mark.parametrize("name", list(BYTES))
def test_workspace_bytes_are_the_recorded_ones_and_the_closed_forms(L, name):
    assert len(BYTES[name]) == len(SHAPES)
    for s, want in zip(SHAPES, BYTES[name]):
        assert query(L, name, s) == want, (name, s)
        assert closed_form(name, s) == want, (name, s)


@pytest.mark.parametrize("name", list(BYTES))
def test_sub_buffers_tile_the_workspace(L, name):
    _, count, align = OPS[name]
    for s in SHAPES:
        got, spans = layout(L, name, s)
        assert got == count, (name, s)
        assert [b for _, b in spans] == [up(b, align) for b in sub_buffers(name, s)], (name, s)
        assert spans[0][0] == 0
        for (off, nbytes), (nxt, _) in zip(spans, spans[1:]):
            assert off % align == 0 and nxt % align == 0
            assert off + nbytes == nxt                       # ascending, disjoint, and as close as the parent packed them
        assert sum(spans[-1]) == query(L, name, s), (name, s)


def test_break_weight_starts_with_a_whole_edt_workspace(L):
    for s in SHAPES:
        _, spans = layout(L, "break_weight", s)
        assert spans[0] == (0, query(L, "edt", s)), s
        assert spans[1][0] == query(L, "edt", s)


def test_get_l_keys_are_adjacent(L):
    """launch_get_l clears best, top1 and top2 with one memset from `best`."""
    for s in SHAPES:
        _, spans = layout(L, "get_l", s)
        (b, nb), (t1, n1), (t2, n2) = spans[2:]
        assert nb == n1 == n2 == up(8 * s[2])
        assert t1 == b + nb and t2 == t1 + n1
        assert t2 + n2 == query(L, "get_l", s)


def _stale(L):
    """Leave a known message in seunet_last_error() so that a query that reports nothing is told from one that does."""
    assert query(L, "skeleton", (0, 0, 0)) == 0
    msg = L.last_error()
    assert "(0, 0, 0)" in msg
    return msg


@pytest.mark.parametrize("name", list(BYTES))
def test_rejected_extents(L, name):
    stale = _stale(L)
    assert query(L, name, (0, 4, 4)) == 0
    assert f"{name}_workspace_bytes" in L.last_error() and "bad dimensions" in L.last_error() and L.last_error() != stale
    assert layout(L, name, (0, 4, 4))[0] == 0
    stale = _stale(L)
    got = query(L, name, (2048, 2048, 512))
    assert got == BYTES_2G[name]
    if got == 0:
        assert name in ("skeleton", "skeleton_branches")
        assert f"{name}_workspace_bytes" in L.last_error() and "bad dimensions" in L.last_error() and L.last_error() != stale
    else:
        assert L.last_error() == stale


def test_skeleton_layout_of_rejected_extents_is_empty(L):
    assert layout(L, "skeleton", (2048, 2048, 512))[0] == 0


@pytest.mark.parametrize("name", EDT_FAMILY)
def test_edt_family_queries_size_an_extent_of_32768(L, name):
    for s, want in zip(SHAPES_32768, BYTES_32768[name]):
        stale = _stale(L)
        assert query(L, name, s) == want == closed_form(name, s), (name, s)
        assert L.last_error() == stale


def test_unknown_op(L):
    assert layout(L, "cc", (4, 4, 4))[0] == 3
    f = L.load().seunet_debug_volume_layout
    assert f(99, 4, 4, 4, None, 0) == -1
