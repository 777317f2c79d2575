"""The plan's kernel routing as ``seunet_net_conv_info`` / ``SE_UNet.conv_plan`` reports it (host only, no GPU).

Two kinds of checks: self-consistency of every routed kernel with the predicate of that kernel and with the parameter registry,
for a spread of descriptors; and the routing DESIGN.md (section 3, and the "kernel selection by measurement" notes) and the
comments of ``Plan::route`` / ``wgrad_kernel`` promise for the benchmarked configuration, written down here from those texts."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    _lib.load()
    return _lib


def plan(L, batch, inch, d, width, dtype, impl=0):
    from seunet_amd.SE_UNet import conv_plan, make_desc, registry
    desc = make_desc(batch, inch, 1, d, d, d, width, L.dtype_code(dtype), impl, 0.01)
    return conv_plan(desc), dict(registry(desc))


DESCS = [(4, 2, 128, 1, dt) for dt in ("bf16", "fp16", "fp32")] + [(1, 2, 64, 1, dt) for dt in ("bf16", "fp16", "fp32")] + [
    (2, 2, 32, 1, "bf16"), (1, 2, 160, 2, "bf16"), (2, 2, 160, 2, "bf16"), (2, 2, 160, 2, "fp16"), (1, 3, 64, 1, "bf16"), (4, 3, 128, 1, "fp16")]
GATED = ["ec1", "ec2", "ec3", "ec4", "ec5", "ec6", "ec7", "ec8", "ec9", "ec10", "ec11", "ec12", "dc1", "dc2", "dc3", "dc4", "dc5", "dc6"]
CAT = ["ec33", "ec63", "ec93", "ec123", "dc22", "dc42"]


@pytest.mark.parametrize("desc", DESCS, ids=lambda d: "-".join(str(v) for v in d))
def test_every_routed_kernel_is_one_its_predicate_admits(L, desc):
    batch, inch, d, width, dtype = desc
    p, reg = plan(L, batch, inch, d, width, dtype)
    lib, code = L.load(), L.dtype_code(dtype)
    ia = L.int_array
    assert sorted(c["name"] for c in p) == sorted(GATED + CAT)          # 18 gated 3x3x3 + 6 aggregation 1x1x1; dc62 is dead
    for c in p:
        name, dil, src_c, cout = c["name"], c["dilation"], c["src_c"], c["cout"]
        what = f"{name} of {desc}: {c}"
        assert c["taps"] == (27 if name in GATED else 1), what
        assert c["dims"] == (batch, d >> c["level"], d >> c["level"], d >> c["level"]), what
        # channel counts against the parameter registry's weight shapes
        k = 3 if c["taps"] == 27 else 1
        assert reg[name + ".conv1.weight"] == (cout, c["cin"], k, k, k), what
        assert c["cin"] == (inch if name == "ec1" else sum(src_c)), what
        assert c["src_is_input"] == ([True] if name == "ec1" else [False] * len(src_c)), what
        assert c["need_dgrad"] == (name != "ec1"), what
        assert (c["src_dist"] != 0) == (len(src_c) == 2) and c["src_dist"] % 256 == 0, what
        if c["x_name"]:
            assert reg[c["x_name"] + ".conv1.weight"] == (cout, inch, 1, 1, 1), what
            assert c["x_materialised"] == (inch > 2), what                 # <= 2 channels: recomputed by the epilogue
        # each pass against the predicate of the kernel it is routed to
        assert c["fwd"] in ("Tiled", "Stream", "March") and c["dgrad"] in (None, "Tiled", "Stream", "March"), what
        assert c["wgrad"] in ("Tiled", "Stream", "March", "Wgrad1x1"), what
        if dtype == "fp32":                                                # the other kernels are 16-bit only
            assert (c["fwd"], c["dgrad"] or "Tiled", c["wgrad"]) == ("Tiled",) * 3, what
        if c["taps"] == 1:
            assert c["fwd"] == "Tiled" and c["dgrad"] == "Tiled" and c["wgrad"] in ("Tiled", "Wgrad1x1"), what
        else:
            assert c["wgrad"] != "Wgrad1x1", what
        if c["fwd"] == "Stream":
            assert len(src_c) == 1 and lib.seunet_conv3d_stream_supported(code, dil, src_c[0], cout), what
        if c["dgrad"] == "Stream":
            assert len(src_c) == 1 and lib.seunet_conv3d_stream_supported(code, dil, cout, src_c[0]), what
        if c["wgrad"] == "Stream":
            assert len(src_c) == 1 and lib.seunet_conv3d_wgrad_stream_supported(code, dil, src_c[0], cout), what
        if c["fwd"] == "March":
            assert lib.seunet_conv3d_march_supported(code, dil, len(src_c), ia(src_c), 1, ia([cout])), what
        if c["dgrad"] == "March":
            assert lib.seunet_conv3d_march_supported(code, dil, 1, ia([cout]), len(src_c), ia(src_c)), what
        if c["wgrad"] == "March":                                          # wgrad_march_cfg: no public predicate; its conditions
            vox = (d >> c["level"]) ** 3
            assert dtype != "fp32" and c["cin"] % 32 == 0 and cout % 32 == 0 and len(src_c) <= 2 and len(set(src_c)) == 1, what
            assert abs(c["src_dist"]) + vox * src_c[0] * 2 < 0xFFFFFFFF and vox * cout * 2 < 0xFFFFFFFF, what
        for key in ("x_fwd", "x_wgrad"):
            assert c[key] == ("Tiled" if c["x_name"] and inch > 2 else None), what   # (in_channel x cout is one combo: never 1x1x1 whole-GEMM)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_naive_descriptor_routes_everything_to_the_naive_kernels(L, dtype):
    for inch in (2, 3):
        p, _ = plan(L, 1, inch, 64, 1, dtype, impl=L.CONV_NAIVE)
        for c in p:
            assert c["fwd"] == "Naive" and c["wgrad"] == "Naive" and c["dgrad"] in (None, "Naive"), c
            if c["x_name"]:
                assert c["x_materialised"] and c["x_fwd"] == "Naive" and c["x_wgrad"] == "Naive", c


def test_conv_info_index_range_and_bad_descriptor(L):
    from seunet_amd.SE_UNet import conv_plan, make_desc
    lib = L.load()
    desc = make_desc(1, 2, 1, 64, 64, 64, 1, L.BF16, 0, 0.01)
    info = L.ConvInfo()
    assert lib.seunet_net_conv_info(C.byref(desc), 23, C.byref(info)) == 0 and info.name == b"dc6"
    assert lib.seunet_net_conv_info(C.byref(desc), 24, C.byref(info)) != 0 and "past the last" in L.last_error()
    assert lib.seunet_net_conv_info(C.byref(desc), -1, C.byref(info)) != 0
    bad = make_desc(1, 2, 1, 100, 64, 64, 1, L.BF16, 0, 0.01)
    assert lib.seunet_net_conv_info(C.byref(bad), 0, C.byref(info)) != 0 and "multiples of 8" in L.last_error()
    with pytest.raises(RuntimeError, match="multiples of 8"):
        conv_plan(bad)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_documented_routing_of_the_benchmark_configuration(L, dtype):
    """4 x 2 x 128^3, width 1, 16-bit storage: what DESIGN.md section 3 and the comments of Plan::route / wgrad_kernel state."""
    p, _ = plan(L, 4, 2, 128, 1, dtype)
    by = {c["name"]: c for c in p}
    passes = lambda n: (by[n]["fwd"], by[n]["dgrad"], by[n]["wgrad"])
    # "small-channel 3x3x3 layers with one source tensor (ec1 / ec2 / ec3 / dc6 at width 1) run on the streaming kernel", all passes
    assert passes("ec1") == ("Stream", None, "Stream")            # (no data gradient towards the network input)
    for n in ("ec2", "ec3", "dc6"):
        assert passes(n) == ("Stream", "Stream", "Stream"), (n, passes(n))
    # conv_march: "ec4, ec5, ec6, dc4, dc5 forward; data gradients of ec4, ec5, ec6, dc3, dc4, dc5"; wgrad_march: "same layers
    # (weight gradients of ec4, ec5, ec6, dc3, dc4, dc5)"; "128-channel inputs (dc1, dc3 forward)" stay on the tiled kernel
    for n in ("ec4", "ec5", "ec6", "dc4", "dc5"):
        assert passes(n) == ("March", "March", "March"), (n, passes(n))
    assert passes("dc3") == ("Tiled", "March", "March")
    # "the dilation-2 layers at 32^3 (ec8, ec9) moved from the tiled to the marching kernels in all three directions"
    for n in ("ec8", "ec9"):
        assert by[n]["dilation"] == 2 and by[n]["dims"][1:] == (32, 32, 32)
        assert passes(n) == ("March", "March", "March"), (n, passes(n))
    # "dilation 1 at 32^3 is a tie and stayed"; the 16^3 level is on the tiled kernel (none of its layers has dilation 2)
    for n in ("ec7", "dc1", "dc2", "ec10", "ec11", "ec12"):
        assert by[n]["dilation"] == 1 and by[n]["dims"][1] in (32, 16)
        assert passes(n) == ("Tiled", "Tiled", "Tiled"), (n, passes(n))
    # wgrad_kernel: the whole-GEMM 1x1x1 kernel pays with 16 or more 32 x 32 (ci, co) combos, or 8 or more on 500 000 voxels:
    # ec63 (128 -> 64: 8 combos, 4 x 64^3 voxels) takes it; "not dc42 (2 combos) nor dc22 (8 combos but 131 k voxels)"; ec93 at
    # this width is 192 -> 64 = 12 combos on 131 k voxels, on dc22's side of the rule
    assert by["ec63"]["wgrad"] == "Wgrad1x1"
    for n in ("ec93", "dc22", "dc42", "ec33", "ec123"):
        assert by[n]["wgrad"] == "Tiled", (n, by[n]["wgrad"])
    # dc5's two sources are placed next to each other (one 32-bit descriptor reaches both); dc3's and dc1's are not
    one = 4 * 128 ** 3 * 32 * 2
    assert abs(by["dc5"]["src_dist"]) == one
    assert abs(by["dc3"]["src_dist"]) > 4 * 64 ** 3 * 64 * 2 and abs(by["dc1"]["src_dist"]) > 4 * 32 ** 3 * 64 * 2


def test_documented_routing_that_depends_on_width_and_batch(L):
    """wgrad_kernel: "256-channel inputs (dc1 ...)" take the marching weight gradient on a coarse level -- that is dc1 at width 2
    (2 x 128 channels); at width 1 it has 128 input channels, the tie that "stays where it was".  The whole-GEMM 1x1x1 kernel's
    ``combos >= 8 && N * voxels >= 500000`` clause: ec63 (8 combos) takes it at 4 x 64^3 and not at 1 x 64^3; ec93 has 12 combos
    on at most 131 k voxels per 128^3 sample of a batch of 4 (tiled)."""
    by2 = {c["name"]: c for c in plan(L, 4, 2, 128, 2, "bf16")[0]}
    assert by2["dc1"]["cin"] == 256 and by2["dc1"]["dims"][1:] == (32, 32, 32) and by2["dc1"]["wgrad"] == "March"
    assert by2["dc1"]["fwd"] == "Tiled"
    by1 = {c["name"]: c for c in plan(L, 4, 2, 128, 1, "bf16")[0]}
    assert by1["dc1"]["cin"] == 128 and by1["dc1"]["wgrad"] == "Tiled"
    one = {c["name"]: c for c in plan(L, 1, 2, 128, 1, "bf16")[0]}
    assert one["ec63"]["wgrad"] == "Tiled" and one["ec93"]["wgrad"] == "Tiled"
    # beyond 4 GB between the two sources "the weight gradient of those two layers takes the tiled kernel" (dc3 at width 2, batch 16)
    big = {c["name"]: c for c in plan(L, 16, 2, 128, 2, "bf16")[0]}
    assert abs(big["dc3"]["src_dist"]) >= 1 << 32 and big["dc3"]["wgrad"] == "Tiled"
    assert {c["name"]: c for c in plan(L, 4, 2, 128, 2, "bf16")[0]}["dc3"]["wgrad"] == "March"    # (the same layer within reach)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_documented_routing_of_config4(L, dtype):
    """2 x 2 x 160^3, width 2, 16-bit storage (BASELINE.json configs[4]): the routing table of DESIGN.md's "... at the second
    configuration" subsection, which tests/test_conv_layers_config4_gpu.py runs pass by pass."""
    p, _ = plan(L, 2, 2, 160, 2, dtype)
    by = {c["name"]: c for c in p}
    passes = lambda n: (by[n]["fwd"], by[n]["dgrad"], by[n]["wgrad"])
    shape = lambda n: (by[n]["dims"][1], by[n]["src_c"], by[n]["cout"], by[n]["dilation"])
    assert all(c["dims"] == (2,) + (160 >> c["level"],) * 3 for c in p)
    # the 16- and 32-channel layers at full resolution stream, as ec1 / ec2 do at width 1
    assert passes("ec1") == ("Stream", None, "Stream") and passes("ec2") == ("Stream", "Stream", "Stream")
    # 160^3: 32 -> 64 (dilation 2) and 64 -> 32 march in all three directions; dc5's 128 input channels keep its forward tiled
    assert shape("ec3") == (160, [32], 64, 2) and passes("ec3") == ("March", "March", "March")
    assert shape("dc6") == (160, [64], 32, 1) and passes("dc6") == ("March", "March", "March")
    assert shape("dc5") == (160, [64, 64], 64, 1) and passes("dc5") == ("Tiled", "March", "March")
    # 80^3
    for n in ("ec4", "ec5"):
        assert shape(n)[:3] == (80, [64], 64) and passes(n) == ("March", "March", "March"), (n, passes(n))
    assert shape("ec6") == (80, [64], 128, 2) and passes("ec6") == ("March", "Tiled", "March")
    assert shape("dc4") == (80, [128], 64, 1) and passes("dc4") == ("Tiled", "March", "March")
    assert shape("dc3") == (80, [128, 128], 128, 1) and passes("dc3") == ("Tiled", "Tiled", "March")
    # 40^3: 128 -> 128 with dilation 2, and dc1's 256 input channels: tiled but for the marching weight gradient
    for n in ("ec8", "ec9"):
        assert shape(n) == (40, [128], 128, 2) and passes(n) == ("Tiled", "Tiled", "March"), (n, passes(n))
    assert shape("dc1") == (40, [128, 128], 128, 1) and passes("dc1") == ("Tiled", "Tiled", "March")
    # ec63, 1x1x1 256 -> 128 at 80^3: a form wgrad_1x1.hip does not instantiate
    assert (by["ec63"]["cin"], by["ec63"]["cout"], by["ec63"]["taps"]) == (256, 128, 1) and passes("ec63") == ("Tiled", "Tiled", "Tiled")
    # the epilogue kernels' partial records per sample: the cap of 256 on levels 0 - 2, the floor branch (8000 // 128) on level 3
    lib = L.load()
    assert [lib.seunet_epilogue_slots(L.Dims(2, 160 >> l, 160 >> l, 160 >> l)) for l in range(4)] == [256, 256, 256, 62]
    assert {c["cout"] for c in p} == {16, 32, 64, 128}
