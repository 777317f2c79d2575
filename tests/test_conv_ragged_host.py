"""The ragged per-layer convolution cases test what they name (host only, no GPU).

tests/test_conv_layers_ragged_gpu.py runs every routed pass of the plans of tests/conv_ragged_cases.py bitwise.  Its worth lies in
WHICH kernel each layer runs on and in how the extents meet that kernel's tiles; both are decided on the host (``Plan::route``,
``march_level``, ``wgrad_kernel`` in csrc/net.cpp and the cut functions of the kernels), so both are proved here, where a
re-route or a moved tile fails a test on a CPU-only build instead of quietly emptying a GPU case.

Tile sizes restated from the sources (the cuts that have a query are asked through it):
  x block of every kernel: 32 columns (MA_TX, WM_TX)
  marching forward / data gradient (conv_march.hip, march_cfg): patches of RY = RYW * (4 / NGW) rows, where NGW = 4 when the
    destination channels are a multiple of 64, else 2; RYW = 8 (32 source channels) or 4 (64) for NGW = 4, and 4 -- 2 for 64
    source channels at dilation 2 -- for NGW = 2: 8 or 4 rows
  marching weight gradient (wgrad_march.hip): patches of WM_RY = 4 rows; at most 256 workgroups over all (ci, co) combos
  whole-GEMM 1x1x1 weight gradient (wgrad_1x1.hip): chunks of 128 voxels of the flat (sample, voxel) index for 128 -> 64 channels
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ragged_cases as R  # noqa: E402

PASSES = ("fwd", "dgrad", "wgrad")
cdiv = lambda a, b: -(-a // b)


@pytest.fixture(scope="module")
def CFGS():
    return R.configs()


@pytest.fixture(scope="module")
def lib():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    return _lib


def layers(cfg, dtype=None):
    """The records of the layers a configuration runs (its LAYERS), in plan order."""
    return [cfg.PLANS[dtype or cfg.dtypes[0]][n] for n in cfg.LAYERS]


def march_rows(src_c, dst_c, dil):
    """Rows of a marching patch for a pass from src_c to dst_c effective channels (march_cfg, mode 0 / 1)."""
    ngw = 4 if dst_c % 64 == 0 else 2
    ks = src_c // 32
    ryw = (8 if ks == 1 else 4) if ngw == 4 else (2 if ks == 2 and dil == 2 else 4)
    return ryw * (4 // ngw)


def march_channels(c, p):
    """(source, destination) effective channels of the marched pass p of layer c."""
    cin = sum(c["src_c"])
    return (cin, c["cout"]) if p == "fwd" else (c["cout"], cin)


# ---------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["A", "A2", "B"])
def test_every_layer_is_routed_to_the_kernel_named_for_it(CFGS, key):
    cfg, routing = CFGS[key]
    assert sorted(routing) == sorted(cfg.PLANS[cfg.dtypes[0]]) and len(routing) == 24
    assert not R.misrouted(cfg, routing), R.misrouted(cfg, routing)


def test_configurations_are_the_stated_ones(CFGS):
    (a, _), (a2, _), (b, _) = CFGS["A"], CFGS["A2"], CFGS["B"]
    assert (a.batch, a.extent, a.width, a.dtypes, a.levels) == (1, (72, 56, 88), 1, ("bf16", "fp16"), None)
    assert (a2.batch, a2.extent, a2.width, a2.dtypes, a2.levels) == (1, (72, 56, 88), 2, ("bf16",), None)
    assert (b.batch, b.extent, b.width, b.dtypes, b.levels) == (2, (104, 152, 136), 1, ("bf16", "fp16"), (1, 2, 3))
    assert len(a.LAYERS) == len(a2.LAYERS) == 24 and len(b.LAYERS) == 18
    assert sorted(n for n in b.PLANS["bf16"] if n not in b.LAYERS) == sorted(["ec1", "ec2", "ec3", "ec33", "dc5", "dc6"])
    assert len(b.PLANS["bf16"]) == 24                                   # PLANS stays whole
    for cfg in (a, a2, b):
        d, h, w = cfg.extent
        for dt in cfg.dtypes:
            for c in cfg.PLANS[dt].values():
                assert c["dims"] == (cfg.batch, d >> c["level"], h >> c["level"], w >> c["level"]), c
        # the case lists follow LAYERS: one case per (layer, storage type), dc5 twice (two layouts); ec1 has no data gradient
        n5 = int("dc5" in cfg.LAYERS)
        assert len(cfg.CASES) == (len(cfg.LAYERS) + n5) * len(cfg.dtypes)
        assert {c[0] for c in cfg.CASES} == set(cfg.LAYERS) and {c[0] for c in cfg.DGRAD_CASES} == set(cfg.LAYERS) - {"ec1"}


def test_what_the_plans_route_is_not_vacuous(CFGS):
    (a, _), (a2, _), (b, _) = CFGS["A"], CFGS["A2"], CFGS["B"]
    nine = {(k, p) for k in ("Stream", "March", "Tiled") for p in PASSES}
    assert nine <= a.ROUTED and nine <= a2.ROUTED
    run_b = {(c[p], p) for dt in b.dtypes for c in layers(b, dt) for p in PASSES if c[p]}
    assert run_b == {(k, p) for k in ("March", "Tiled") for p in PASSES} | {("Wgrad1x1", "wgrad")}


# ---------------------------------------------------------------------------------------------------
# the tails
# ---------------------------------------------------------------------------------------------------
def test_levels_sit_where_the_routing_thresholds_put_them(CFGS):
    """march_level: W >= 32 and (voxels >= 48^3, or dilation 2 and voxels >= 32^3); wgrad_kernel: every dilation-2 layer."""
    vox = lambda ext, l: (ext[0] >> l) * (ext[1] >> l) * (ext[2] >> l)
    assert vox(R.EXT_A, 0) == 354816 >= 48 ** 3 and R.EXT_A[2] == 88 == 2 * 32 + 24           # A marches at level 0
    assert 32 ** 3 <= vox(R.EXT_A, 1) == 44352 < 48 ** 3 and R.EXT_A[2] >> 1 == 44             # A level 1 between the thresholds
    assert vox(R.EXT_A, 2) == 5544 < 32 ** 3 and R.EXT_A[2] >> 2 == 22 < 32
    assert vox(R.EXT_B, 1) == 268736 >= 48 ** 3 and R.EXT_B[2] >> 1 == 68 == 2 * 32 + 4
    assert 32 ** 3 <= vox(R.EXT_B, 2) == 33592 < 48 ** 3 and R.EXT_B[2] >> 2 == 34 >= 32
    for ext in (R.EXT_A, R.EXT_B):
        assert all(e % 8 == 0 for e in ext)                                                    # what Plan::init asks
        assert all(e >> 3 & 1 for e in ext), ext                                               # level 3: every extent odd


@pytest.mark.parametrize("key", ["A", "A2", "B"])
def test_every_marched_or_streamed_layer_has_an_x_tail_and_unequal_axes(CFGS, key):
    cfg, _ = CFGS[key]
    seen = 0
    for c in layers(cfg):
        _, d, h, w = c["dims"]
        assert len({d, h, w}) == 3, c["dims"]                                                  # pairwise different on every level
        if any(c[p] in ("March", "Stream") for p in PASSES):
            assert w % 32 != 0, (c["name"], c["dims"])
            seen += 1
    assert seen >= 6


def test_x_and_y_tails_are_the_named_ones(CFGS):
    (a, _), (a2, _), (b, _) = CFGS["A"], CFGS["A2"], CFGS["B"]
    pa, pa2, pb = a.PLANS["bf16"], a2.PLANS["bf16"], b.PLANS["bf16"]
    # A: x tails 24 / 12, H = 3 * 8 + 4 under the 8-row patches of the 32-channel marching layers of level 1
    assert pa["dc5"]["dims"][3] % 32 == 24 and pa["ec5"]["dims"][3] % 32 == 12
    for n in ("ec5", "ec6"):
        assert march_rows(*march_channels(pa[n], "fwd"), 2) == 8 and pa[n]["dims"][2] == 28 == 3 * 8 + 4
    # A2: the 4-row patches of the 64-channel layers meet H = 28 evenly, the 8-row ones of ec3 -> 64 meet H = 56 evenly:
    # what A2 adds is the x tail of 24 on March at full resolution and the 256-channel weight gradients
    assert march_rows(*march_channels(pa2["ec3"], "fwd"), 2) == 8 and march_rows(*march_channels(pa2["ec5"], "fwd"), 2) == 4
    assert pa2["ec3"]["dims"][3] % 32 == 24 and pa2["dc1"]["cin"] == pa2["dc3"]["cin"] == 256
    # B level 1: x tail 4, H % 8 == 4 under 8-row patches (forward of all four marched layers)
    for n in ("ec4", "ec5", "ec6", "dc4"):
        c = pb[n]
        assert c["dims"] == (2, 52, 76, 68) and c["dims"][3] % 32 == 4 and c["dims"][2] % 8 == 4
        assert march_rows(*march_channels(c, "fwd"), c["dilation"]) == 8, n
    assert {march_rows(*march_channels(pb[n], "dgrad"), pb[n]["dilation"]) for n in ("ec4", "ec5", "ec6", "dc4", "dc3")} == {4, 8}
    # B level 2: x tail 2, H % 4 == 2 under the 4-row patches of 64 -> 64 channels, and 13 planes per parity class
    for n in ("ec8", "ec9"):
        c = pb[n]
        assert c["dims"] == (2, 26, 38, 34) and c["dims"][3] % 32 == 2 and c["dims"][2] % 4 == 2 and c["dilation"] == 2
        assert march_rows(*march_channels(c, "fwd"), 2) == march_rows(*march_channels(c, "dgrad"), 2) == 4
        assert c["dims"][1] % 2 == 0 and (c["dims"][1] // 2) % 2 == 1 and c["dims"][1] // 2 == 13
    # every marching weight gradient works on 4-row patches: H % 4 == 2 on A's and B's level 2
    assert pa["ec8"]["dims"][2] % 4 == 2 and pb["ec8"]["dims"][2] % 4 == 2


def test_marching_weight_gradient_with_one_partial_x_block(CFGS):
    for key in ("A", "A2"):
        cfg, _ = CFGS[key]
        for dt in cfg.dtypes:
            for n in ("ec8", "ec9"):
                c = cfg.PLANS[dt][n]
                assert c["wgrad"] == "March" and c["dilation"] == 2 and c["dims"][3] == 22 < 32 and cdiv(c["dims"][3], 32) == 1
                assert c["fwd"] == c["dgrad"] == "Tiled"                  # march_level asks W >= 32; wgrad_kernel does not


def test_whole_gemm_weight_gradient_chunks_straddle_the_samples(CFGS):
    """ec63 of B: 128 -> 64 channels, 8 combos of 32 x 32, so wgrad_kernel asks N * voxels >= 500 000; wgrad_1x1_cfg gives that
    channel pair chunks of 128 voxels of the flat index ((128 + 64) * 2 * 128 = 48 KB per stage, three stages in 159 KB)."""
    b, _ = CFGS["B"]
    for dt in b.dtypes:
        c = b.PLANS[dt]["ec63"]
        n, d, h, w = c["dims"]
        assert (c["cin"], c["cout"], c["taps"], c["src_c"]) == (128, 64, 1, [64, 32, 32]) and c["wgrad"] == "Wgrad1x1"
        assert cdiv(c["cin"], 32) * cdiv(c["cout"], 32) == 8 and n * d * h * w == 537472 >= 500000
        assert (d * h * w) % 128 == 64                                     # the second sample starts in the middle of a chunk
        assert (n * d * h * w) % 128 == 0                                  # ... and the flat index ends on a chunk border
    a, _ = CFGS["A"]
    assert a.PLANS["bf16"]["ec63"]["wgrad"] == "Tiled"                     # 44 352 voxels: below the threshold


def test_whole_gemm_weight_gradient_with_a_ragged_last_chunk(CFGS):
    """Extents that are multiples of 8 give a level-1 sample a multiple of 4 * 4 * 4 = 64 voxels, so two samples are always a
    multiple of the 128-voxel chunk; C runs ec63 on three samples of 64 mod 128 voxels."""
    c3, routing = CFGS["C"]
    assert (c3.batch, c3.extent, c3.width, c3.dtypes, c3.levels) == (3, R.EXT_B, 1, ("bf16", "fp16"), (1,))
    assert not R.misrouted(c3, routing)
    for dt in c3.dtypes:
        c = c3.PLANS[dt]["ec63"]
        n, d, h, w = c["dims"]
        assert c["wgrad"] == "Wgrad1x1" and (c["cin"], c["cout"]) == (128, 64) and "ec63" in c3.LAYERS
        assert (d * h * w) % 128 == 64 and (n * d * h * w) % 128 == 64 and n * d * h * w == 806208 < 1 << 24


# ---------------------------------------------------------------------------------------------------
# exactness and layout
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["A", "A2", "B"])
def test_sums_stay_exact_in_f32(CFGS, key):
    cfg, _ = CFGS[key]
    for dt in cfg.dtypes:
        for c in layers(cfg, dt):
            n, d, h, w = c["dims"]
            assert n * d * h * w < 1 << 24, c                              # weight gradient: operands in {-1, 0, 1}
            assert n * d * h * w <= 537472
            assert c["taps"] * sum(c["src_c"]) * 9 + 3 <= 62211 and c["taps"] * c["cout"] * 9 + 3 <= 62211, c
            assert 62211 + 3 < 65504                                       # `+=` in fp16 storage does not overflow


@pytest.mark.parametrize("key", ["A", "A2", "B"])
def test_two_source_layers_sit_at_the_arena_distance(CFGS, key):
    cfg, _ = CFGS[key]
    paired = [c for dt in cfg.dtypes for c in layers(cfg, dt) if len(c["src_c"]) == 2]
    assert {c["name"] for c in paired} == {"dc1", "dc22", "dc3", "dc42", "dc5"} & set(cfg.LAYERS) and len(paired) >= 4
    for c in paired:
        n, d, h, w = c["dims"]
        nbytes = [n * d * h * w * ch * 2 for ch in c["src_c"]]
        dist = c["src_dist"]
        assert dist != 0 and dist % 256 == 0, c                           # conv_layer_cases.place_pair's precondition
        assert dist >= nbytes[0] or -dist >= nbytes[1], c                 # the sources do not overlap
    for c in (c for dt in cfg.dtypes for c in layers(cfg, dt) if len(c["src_c"]) != 2):
        assert c["src_dist"] == 0


def test_source_distances_differ_from_the_cubic_plans(CFGS):
    """A non-cubic arena puts the second source somewhere a cube of the suite does not: none of these distances is one of the
    128^3 (batch 1 / 4 / 16) or 160^3 plans'."""
    import conv_layer_cases as L
    cubes = set()
    for batch, extent, width in ((1, 128, 1), (4, 128, 1), (16, 128, 1), (2, 160, 2)):
        cubes |= {c["src_dist"] for c in L.plan_of("bf16", batch, extent, width) if len(c["src_c"]) == 2}
    for key in ("A", "A2", "B"):
        cfg, _ = CFGS[key]
        ours = {c["src_dist"] for c in layers(cfg) if len(c["src_c"]) == 2}
        assert ours and not ours & cubes, (key, ours & cubes)


# ---------------------------------------------------------------------------------------------------
# the cuts of the marched layers
# ---------------------------------------------------------------------------------------------------
def march_segments(lib, c, p):
    """z segments per parity class of the marched forward / data gradient p of layer c, from seunet_conv3d_march_slots
    (= y patches * x blocks * segments * dilation; the data gradient's overwrite mode shares the forward's cut function)."""
    src, dst = march_channels(c, p)
    _, d, h, w = c["dims"]
    slots = lib.load().seunet_conv3d_march_slots(c["dilation"], src, dst, lib.Dims(*c["dims"]))
    per_seg = cdiv(h, march_rows(src, dst, c["dilation"])) * cdiv(w, 32) * c["dilation"]
    assert slots > 0 and slots % per_seg == 0, (c["name"], p, slots, per_seg)
    return slots // per_seg


def wgrad_march_slabs(c):
    """Slabs (persistent workgroups) per (ci, co) combo of the marching weight gradient of layer c.  No query takes the shape
    (seunet_conv3d_wgrad_workspace_bytes bounds it by channels alone), so this restates wm_channels / wm_cut of wgrad_march.hip."""
    n, d, h, w = c["dims"]
    cin, cout, dil = c["cin"], c["cout"], c["dilation"]
    ncb, nob = (4, 2) if cin % 64 == 0 else ((2, 4) if cout % 64 == 0 else (2, 2))
    combos = (cin // (16 * ncb)) * (cout // (16 * nob))
    gmax = max(1, 256 // combos)
    per_seg, planes, nseg = n * dil * cdiv(h, 4) * cdiv(w, 32), cdiv(d, dil), 1
    while per_seg * nseg < gmax and planes // (nseg * 2) >= 8:
        nseg *= 2
    return min(per_seg * nseg, gmax), nseg


@pytest.mark.parametrize("key", ["A", "B"])
def test_marched_layers_are_cut_into_several_segments_or_slabs(CFGS, lib, key):
    cfg, _ = CFGS[key]
    marched = 0
    for dt in cfg.dtypes:
        for c in layers(cfg, dt):
            if "March" not in (c["fwd"], c["dgrad"], c["wgrad"]):
                continue
            marched += 1
            segs = {p: march_segments(lib, c, p) for p in ("fwd", "dgrad") if c[p] == "March"}
            slabs, wseg = wgrad_march_slabs(c) if c["wgrad"] == "March" else (0, 0)
            assert any(s > 1 for s in segs.values()) or slabs > 1, (c["name"], segs, slabs)
            if c["fwd"] == "March":                                        # every marched forward has a z seam
                assert segs["fwd"] > 1, (c["name"], segs)
            if c["wgrad"] == "March":                                      # every marched weight gradient sums several slabs
                assert slabs > 1, (c["name"], slabs)
    assert marched == {"A": 5, "B": 7}[key] * len(cfg.dtypes)


def test_batch_2_moves_the_marching_cut(CFGS, lib):
    """march_zsteps counts the workgroups of the whole launch: B's level-1 layers are cut differently at batch 2 than one
    sample of the same extents would be."""
    b, _ = CFGS["B"]
    moved = []
    for n in ("ec4", "ec5", "ec6", "dc4"):
        c = b.PLANS["bf16"][n]
        one = dict(c, dims=(1,) + tuple(c["dims"][1:]))
        moved.append(march_segments(lib, c, "fwd") != march_segments(lib, one, "fwd"))
    assert any(moved), moved
