"""Launch geometry of the marching kernels as the planning queries report it (host only, no GPU).

Every marching kernel cuts a volume into patches, z segments and parity classes, and the cut decides how many statistics
slots or weight-gradient slabs a launch writes.  The queries (``*_slots``, ``*_workspace_bytes``) size the buffers from the
same cut, the network plan lays its arena out from them, and ``src_dist`` follows from the arena.  The numbers below were
recorded from the library before the queries and the launchers were made to share one cut function per kernel; a refactor
of that layer must leave all of them where they are.

The shapes reach every branch of the cut functions: a sample with fewer than 8 planes, the ``planes / 8`` cap on the segments
((1, 80, 8, 64)), dilation 2 with an odd depth, H and W that are no multiples of the patch, 128^3 at batch 1 and 4; for
conv_march both channel configurations and the 64 -> 32 / 32 -> 64 mixes, because its cut depends on the batch and on the
number of N blocks.

The x2 up-sampling passes have a cut as well: it names the kernel form (gather, tiled or z-marching) a (storage type, channels,
extents) combination runs on.  ``UP2_FORMS`` pins that form for every shape of ``test_ops_gpu.test_upsample2_forward_backward_shapes``
-- which takes its shapes from here -- and ``HEAD_BWD_TMP_FLOATS`` pins the workspace of the heads' backward."""
import ctypes as C
import hashlib
import json

import pytest

from test_route_host import DESCS

# (n, d, h, w)
SHAPES = [(1, 4, 16, 32), (1, 7, 9, 33), (1, 12, 16, 32), (1, 80, 8, 64), (2, 33, 20, 40), (3, 17, 36, 100), (1, 64, 64, 64),
          (4, 32, 32, 32), (1, 128, 128, 128), (4, 128, 128, 128), (2, 160, 160, 160)]
DILS = [1, 2]
MARCH_CH = [(32, 32), (64, 64), (64, 32), (32, 64)]
WS_CH = [(8, 8), (8, 16), (16, 16), (16, 32), (32, 16)]
WG_TAPS, WG_CIN, WG_COUT = [1, 27], [1, 2, 8, 16, 32, 64, 96, 128, 192, 256, 512], [8, 16, 32, 64, 128, 256]

# [shape][dilation]
STREAM_SLOTS = [[2, 4], [4, 8], [4, 4], [20, 20], [30, 36], [60, 80], [64, 64], [16, 16], [64, 128], [64, 128], [100, 200]]
# [shape][dilation][channels]
MARCH_SLOTS = [[[8, 16, 8, 8], [8, 16, 16, 8]], [[28, 42, 28, 28], [32, 48, 48, 32]], [[6, 12, 6, 6], [24, 48, 48, 24]],
 [[16, 32, 16, 16], [24, 48, 48, 24]], [[30, 50, 30, 30], [60, 100, 100, 60]], [[60, 72, 60, 60], [80, 72, 72, 80]],
 [[112, 224, 112, 112], [256, 256, 256, 256]], [[32, 64, 32, 32], [32, 64, 64, 32]],
 [[256, 256, 256, 256], [256, 256, 256, 256]], [[64, 128, 64, 64], [128, 256, 256, 128]],
 [[500, 600, 500, 500], [1000, 2000, 2000, 1000]]]
# [shape][dilation][channels]
WGRAD_STREAM_BYTES = [[[13824, 27648, 55296, 110592, 110592], [27648, 55296, 110592, 221184, 221184]],
 [[27648, 55296, 110592, 221184, 221184], [55296, 110592, 221184, 442368, 442368]],
 [[27648, 55296, 110592, 221184, 221184], [27648, 55296, 110592, 221184, 221184]],
 [[138240, 276480, 552960, 1105920, 1105920], [138240, 276480, 552960, 1105920, 1105920]],
 [[414720, 829440, 1658880, 3317760, 3317760], [497664, 995328, 1990656, 3981312, 3981312]],
 [[1244160, 2488320, 4976640, 9953280, 9953280], [1658880, 3317760, 6635520, 13271040, 13271040]],
 [[884736, 1769472, 3538944, 7077888, 7077888], [884736, 1769472, 3538944, 7077888, 7077888]],
 [[442368, 884736, 1769472, 3538944, 3538944], [442368, 884736, 1769472, 3538944, 3538944]],
 [[1769472, 3538944, 7077888, 14155776, 14155776], [1769472, 3538944, 7077888, 14155776, 14155776]],
 [[1769472, 3538944, 7077888, 14155776, 14155776], [3538944, 7077888, 14155776, 28311552, 28311552]],
 [[2764800, 5529600, 11059200, 22118400, 22118400], [2764800, 5529600, 11059200, 22118400, 22118400]]]
# [taps][cin][cout]
WGRAD_BYTES = [[[2097408, 2097408, 2097408, 4194560, 8388864, 16777472], [2097408, 2097408, 2097408, 4194560, 8388864, 16777472],
  [2097408, 2097408, 2097408, 4194560, 8388864, 16777472], [2097408, 2097408, 2097408, 4194560, 8388864, 16777472],
  [2097408, 2097408, 2097408, 4194560, 8388864, 16777472], [2097408, 2097408, 2097408, 4194560, 8388864, 16777472],
  [2097408, 2097408, 4194560, 8388864, 16777472, 33554688], [2097408, 2097408, 4194560, 8388864, 16777472, 33554688],
  [3145984, 3145984, 6291712, 12583168, 25166080, 50331904], [4194560, 4194560, 8388864, 16777472, 33554688, 67109120],
  [8388864, 8388864, 16777472, 33554688, 67109120, 134217984]],
 [[56623360, 56623360, 56623360, 56623360, 56623360, 56623360], [56623360, 56623360, 56623360, 56623360, 56623360, 56623360],
  [56623360, 56623360, 56623360, 56623360, 56623360, 56623360], [56623360, 56623360, 56623360, 56623360, 56623360, 56623360],
  [56623360, 56623360, 56623360, 56623360, 56623360, 56623360], [56623360, 56623360, 56623360, 56623360, 56623360, 56623360],
  [56402176, 56402176, 56402176, 56402176, 55738624, 55738624], [56623360, 56623360, 56623360, 56623360, 56623360, 56623360],
  [56402176, 56402176, 56402176, 55738624, 55738624, 84934912],
  [56623360, 56623360, 56623360, 56623360, 56623360, 113246464],
  [56623360, 56623360, 56623360, 56623360, 113246464, 226492672]]]
# per descriptor of DESCS: workspace bytes, input-gradient scratch bytes, src_dist of the two-source blocks in plan order, and
# the SHA-256 of the whole list of seunet_net_conv_info records (json, sorted keys)
NETS = [[11276056832, 76546048, [-54525952, -33554432, -591396864, -268435456, -536870912],
  '1eb632db322912bbff11131616c8a8ddd66b7d0c25136c83cd2e14c5e76a18e0'],
 [11276056832, 76546048, [-54525952, -33554432, -591396864, -268435456, -536870912],
  '1eb632db322912bbff11131616c8a8ddd66b7d0c25136c83cd2e14c5e76a18e0'],
 [22218887424, 76546048, [-109051904, -67108864, -1182793728, -536870912, -1073741824],
  '1e5263cd71424243089227c970caf64ad70da9a55cd563a8399bbb7c8013b639'],
 [413430016, 2392064, [-1703936, -1048576, -18481152, -8388608, -16777216],
  'e184170a7bbfbebb078e11b1c529c228c010c8c4453dcff3751084916c1d9a2c'],
 [413430016, 2392064, [-1703936, -1048576, -18481152, -8388608, -16777216],
  'e184170a7bbfbebb078e11b1c529c228c010c8c4453dcff3751084916c1d9a2c'],
 [761383168, 2392064, [-3407872, -2097152, -36962304, -16777216, -33554432],
  '60beae079441c96519dca98a6c4edce2dfcfaa48cf235986324ccc304a624e9d'],
 [151843584, 598016, [-425984, -262144, -4620288, -2097152, -4194304],
  '68a80dbdb2504a362ce68d9c6a7f0052765e959da7255140b48503e10a23e4a8'],
 [10866605568, 37376000, [-53248000, -32768000, -577536000, -262144000, -524288000],
  '0f293a64f182d921a4671023afdb1feaa321d68a63f6f0f16180d1eed152bde0'],
 [21652321024, 74752000, [-106496000, -65536000, -1155072000, -524288000, -1048576000],
  'f466d12cc2e080ee080ff0161ea60bc0d912cbfc0d91d39806ed5ee6345d4bf5'],
 [21652321024, 74752000, [-106496000, -65536000, -1155072000, -524288000, -1048576000],
  'f466d12cc2e080ee080ff0161ea60bc0d912cbfc0d91d39806ed5ee6345d4bf5'],
 [450763264, 3588096, [-1703936, -1048576, -18481152, -8388608, -16777216],
  'a957b6c63b4e24b6d935dc3735ce4fd73ed61c3606c6ac620518001df0c2fc46'],
 [12478484992, 114819072, [-54525952, -33554432, -591396864, -268435456, -536870912],
  '12f56e7a96362311917c8f8b429ac2f3df6640d51e5e348c842200c1c7fc6713']]

# seunet_head_bwd_tmp_floats per shape, recorded from the library before the size query and the launcher shared one layout
HEAD_BWD_TMP_FLOATS = [3268, 3314, 9420, 61672, 79476, 275708, 393664, 197056, 3146944, 12587200, 12291392]
# The form of the x2 up-sampling, written down from the conditions of the launchers as they stood before the cuts existed.
# (n, c, d, h, w) of the coarse tensor -> (forward 16-bit, forward f32, backward 16-bit, backward f32).
#   forward:  march for C = 32 / 64 / 128 with every extent >= 2 and 2 * 3 * 68 * C * sizeof(T) <= 112 KB of LDS (128 channels
#             in f32 would need 208 896 B); else tiled while 4 * 68 * C * 4 B <= 144 KB (C <= 128: 136 channels need 147 968 B);
#             else gather
#   backward: march in 16-bit storage for C = 32 / 64 / 128 with every extent >= 4; else tiled for C <= 128 and W >= 2; else gather
UP2_FORMS = {
    (1, 32, 5, 7, 70): ("march", "march", "march", "tiled"),
    (2, 64, 3, 4, 33): ("march", "march", "tiled", "tiled"),
    (1, 8, 1, 1, 2): ("tiled", "tiled", "tiled", "tiled"),
    (1, 16, 2, 9, 64): ("tiled", "tiled", "tiled", "tiled"),
    (1, 128, 2, 3, 5): ("march", "tiled", "tiled", "tiled"),
    (2, 64, 9, 4, 33): ("march", "march", "march", "tiled"),
    (1, 128, 4, 6, 20): ("march", "tiled", "march", "tiled"),
    (1, 32, 40, 9, 17): ("march", "march", "march", "tiled"),
    (1, 32, 33, 16, 16): ("march", "march", "march", "tiled"),
    (1, 64, 4, 4, 4): ("march", "march", "march", "tiled"),
    # the smallest shapes that reach the gather kernels: more than 128 channels (both directions), coarse W = 1 (backward)
    (1, 136, 2, 3, 3): ("gather", "gather", "gather", "gather"),
    (1, 8, 2, 3, 1): ("tiled", "tiled", "gather", "gather"),
}
UP2_FORM_NAMES = ["gather", "tiled", "march"]


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    _lib.load()
    return _lib


def stream_slots(L):
    lib = L.load()
    return [[lib.seunet_conv3d_stream_slots(dil, L.Dims(*s)) for dil in DILS] for s in SHAPES]


def march_slots(L):
    lib = L.load()
    return [[[lib.seunet_conv3d_march_slots(dil, ci, co, L.Dims(*s)) for ci, co in MARCH_CH] for dil in DILS] for s in SHAPES]


def wgrad_stream_bytes(L):
    lib = L.load()
    return [[[lib.seunet_conv3d_wgrad_stream_workspace_bytes(xc, yc, dil, L.Dims(*s)) for xc, yc in WS_CH] for dil in DILS]
            for s in SHAPES]


def wgrad_bytes(L):
    lib = L.load()
    return [[[lib.seunet_conv3d_wgrad_workspace_bytes(t, ci, co) for co in WG_COUT] for ci in WG_CIN] for t in WG_TAPS]


def net(L, desc):
    from seunet_amd.SE_UNet import conv_plan, make_desc
    batch, inch, d, width, dtype = desc
    nd = make_desc(batch, inch, 1, d, d, d, width, L.dtype_code(dtype), 0, 0.01)
    lib = L.load()
    plan = conv_plan(nd)
    digest = hashlib.sha256(json.dumps(plan, sort_keys=True).encode()).hexdigest()
    return [lib.seunet_net_workspace_bytes(C.byref(nd)), lib.seunet_net_input_grad_bytes(C.byref(nd)),
            [c["src_dist"] for c in plan if len(c["src_c"]) == 2], digest], plan


def test_tables_cover_every_branch_of_the_cuts():
    planes = lambda s, dil: -(-s[1] // dil)
    assert any(planes(s, 1) < 8 for s in SHAPES) and any(planes(s, 2) < 8 <= planes(s, 1) for s in SHAPES)
    assert (1, 80, 8, 64) in SHAPES                                       # one patch row: the planes / 8 cap binds
    assert any(s[1] % 2 == 1 for s in SHAPES)                             # unequal parity classes at dilation 2
    assert any(s[2] % 8 and s[3] % 32 for s in SHAPES) and any(s[2] % 4 for s in SHAPES)
    assert (1, 128, 128, 128) in SHAPES and (4, 128, 128, 128) in SHAPES
    assert {(32, 32), (64, 64), (64, 32)} <= set(MARCH_CH)


def test_conv_stream_slots(L):
    assert stream_slots(L) == STREAM_SLOTS


def test_conv_march_slots(L):
    assert march_slots(L) == MARCH_SLOTS


def test_wgrad_stream_workspace_bytes(L):
    assert wgrad_stream_bytes(L) == WGRAD_STREAM_BYTES


def test_wgrad_workspace_bytes(L):
    assert wgrad_bytes(L) == WGRAD_BYTES


@pytest.mark.parametrize("i", range(len(DESCS)), ids=["-".join(str(v) for v in d) for d in DESCS])
def test_network_arena_and_conv_records(L, i):
    got, plan = net(L, DESCS[i])
    assert got[:3] == NETS[i][:3], plan
    assert got[3] == NETS[i][3], json.dumps(plan, sort_keys=True, indent=1)


def upsample2_form(L, dtype, c, dims, backward):
    lib = L.load()
    f = lib.seunet_debug_upsample2_form                      # diagnostic export, not in the public header
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int, L.Dims, C.c_int]
    return UP2_FORM_NAMES[f(L.dtype_code(dtype), c, L.Dims(*dims), int(backward))]


def test_upsample2_forms_of_the_tested_shapes(L):
    forms = {f for row in UP2_FORMS.values() for f in row}
    assert forms == set(UP2_FORM_NAMES)                      # every form of both directions is reached
    assert {row[0] for row in UP2_FORMS.values()} == forms and {row[2] for row in UP2_FORMS.values()} == forms
    for (n, c, d, h, w), want in UP2_FORMS.items():
        got = tuple(upsample2_form(L, dt, c, (n, d, h, w), bwd) for bwd in (False, True) for dt in ("bf16", "fp32"))
        assert got == want, (n, c, d, h, w)
        for bwd in (False, True):                            # both 16-bit storage types take the same route
            assert upsample2_form(L, "fp16", c, (n, d, h, w), bwd) == want[2 * bwd], (n, c, d, h, w, bwd)


@pytest.mark.parametrize("desc", DESCS, ids=lambda d: "-".join(str(v) for v in d))
def test_upsample2_forms_of_the_network(L, desc):
    """up0 / up1 / up2 up-sample levels 3 / 2 / 1 with 64 / 64 / 32 channels per unit of width: the forward marches in every
    storage type (at most 128 channels in 16 bits, 64 in f32), the backward marches in 16-bit storage (every coarse extent of these
    descriptors is >= 4) and is tiled in f32."""
    batch, _, d, width, dtype = desc
    for level, c in ((3, 64 * width), (2, 64 * width), (1, 32 * width)):
        dims = (batch, d >> level, d >> level, d >> level)
        assert d >> level >= 4 and c * (4 if dtype == "fp32" else 2) <= 256
        assert upsample2_form(L, dtype, c, dims, False) == "march", (level, c, dims)
        assert upsample2_form(L, dtype, c, dims, True) == ("tiled" if dtype == "fp32" else "march"), (level, c, dims)


def test_head_bwd_tmp_floats(L):
    lib = L.load()
    assert [lib.seunet_head_bwd_tmp_floats(L.Dims(*s)) for s in SHAPES] == HEAD_BWD_TMP_FLOATS
