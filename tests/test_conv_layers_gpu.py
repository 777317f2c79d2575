"""Every convolution pass of the network's plan, at the layer's own shape and on the kernel the plan routes it to, BITWISE
(method, exactness argument and helpers: tests/conv_layer_cases.py).

The cases are generated from ``SE_UNet.conv_plan`` for the benchmarked configuration (4 x 2 x 128^3, width 1) in bf16 and fp16
storage, so a layer that is added or re-routed later is covered without editing this file.  Two smaller plans ride along:
1 x 2 x 128^3 (bf16, all three passes: the segment seams of the marching kernels and the statistic partial count move with the
batch) and the forward of the two-source layers at the source distances of the 16 x 2 x 128^3 inference plan (2^31 bytes and
more: the range a signed 32-bit offset does not reach).  The 160^3 width-2 configuration has its own module,
tests/test_conv_layers_config4_gpu.py."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_layer_cases as L  # noqa: E402
from conv_layer_cases import DTYPES, assert_same, check_wgrad, ints, rounded, shared, sources, storage, wgrad_data  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH, EXTENT = 4, 128
CFG = L.Config(BATCH, EXTENT, 1)
PLANS, LAYERS, CASES, DGRAD_CASES, _ROUTED, _ids = CFG.PLANS, CFG.LAYERS, CFG.CASES, CFG.DGRAD_CASES, CFG.ROUTED, L.ids
# a plan that silently routed everything to one kernel would make the cases below pass vacuously
assert len(LAYERS) == 24 and all(list(PLANS[dt]) == LAYERS for dt in DTYPES), LAYERS
assert {k for k, _ in _ROUTED} >= {"Stream", "March", "Tiled", "Wgrad1x1"}, sorted(_ROUTED)
assert {("Stream", p) for p in ("fwd", "dgrad", "wgrad")} | {("March", p) for p in ("fwd", "dgrad", "wgrad")} <= _ROUTED, sorted(_ROUTED)

# 1 x 2 x 128^3: march_zsteps / ws_zsteps cut a sample's planes differently than at batch 4, seunet_epilogue_slots is 256
# instead of 192 at every level but the last, and ec63's weight gradient leaves the whole-GEMM kernel for the tiled one
ONE = L.Config(1, EXTENT, 1, dtypes=("bf16",))
assert ONE.LAYERS == LAYERS and ONE.passes("ec63")[2] == "Tiled" and PLANS["bf16"]["ec63"]["wgrad"] == "Wgrad1x1"
assert {("Stream", p) for p in ("fwd", "dgrad", "wgrad")} | {("March", p) for p in ("fwd", "dgrad", "wgrad")} <= ONE.ROUTED, sorted(ONE.ROUTED)

# 16 x 2 x 128^3 (auto_batch's cap): dc5's sources are exactly 2^31 bytes apart and dc3's 2 365 587 456, inside [2^31, 2^32)
# where a signed 32-bit byte offset breaks and test_two_sources_more_than_4gb_apart (>= 2^32) does not look
BIG = L.Config(16, EXTENT, 1)
PAIRED = [n for n in LAYERS if len(BIG.PLANS["bf16"][n]["src_c"]) == 2]
assert PAIRED == ["dc1", "dc22", "dc3", "dc42", "dc5"], PAIRED
assert abs(BIG.PLANS["bf16"]["dc5"]["src_dist"]) == 1 << 31 and abs(BIG.PLANS["bf16"]["dc3"]["src_dist"]) == 2365587456
assert abs(PLANS["bf16"]["dc5"]["src_dist"]) < 1 << 31


@pytest.fixture(scope="module")
def S():
    return L.ops_or_skip()


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_and_statistics(S, case):
    L.forward_case(S, CFG, case)


@pytest.mark.parametrize("case", DGRAD_CASES, ids=_ids)
def test_data_gradient(S, case):
    """Overwrite, ``+=`` and a null first destination: see ``conv_layer_cases.dgrad_case``."""
    L.dgrad_case(S, CFG, case)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_weight_gradient(S, case):
    L.wgrad_case(S, CFG, case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_gradient_of_a_256_channel_input_on_a_coarse_level(S, dtype):
    """wgrad_kernel's third clause (cin >= 256 takes the marching kernel below 48^3) is met by dc1 at width 2 only: 2 x 128
    channels on 4 x 32^3, its sources at the distance that plan gives them."""
    c = {e["name"]: e for e in L.plan_of(dtype, BATCH, EXTENT, 2)}["dc1"]
    assert c["cin"] == 256 and c["dims"] == (BATCH, 32, 32, 32) and c["wgrad"] == "March", c
    x, dy, ref = shared(("wgrad", "dc1 at width 2"), lambda: wgrad_data(c, 3500))
    srcs = sources(S, x, c, dtype, "plan")
    check_wgrad(S, c, srcs, S.to_cl(dy.float(), dtype), ref, f"dc1 at width 2, weight gradient on March ({dtype})")


# ---------------------------------------------------------------------------------------------------
# two marching sources 4 GB apart
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_sources_more_than_4gb_apart(S, dtype):
    """launch_conv_march leaves the one-descriptor addressing when its two forward sources span 2^32 bytes or more, and
    wgrad_march_cfg refuses such a pair, so that the weight gradient falls back to the tiled kernel (the plan relies on both for
    dc1 / dc3 at large batches).  A dc5-shaped layer whose 32-channel sources sit at the two ends of one 4 GB + 64 MB allocation."""
    lib = S._lib
    shape, c_src, cout = (1, 16, 40, 64), 32, 32
    total = (1 << 32) + (64 << 20)
    try:
        buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:                    # (torch.cuda.OutOfMemoryError is one)
        pytest.skip(f"could not allocate {total} bytes on the GPU: {str(e).splitlines()[0]}")
    n, d, h, w = shape
    nb = n * d * h * w * c_src * 2
    cl = (n, d, h, w, c_src)
    far = [buf[:nb].view(storage(dtype)).view(cl), buf[total - nb:].view(storage(dtype)).view(cl)]
    assert far[1].data_ptr() - far[0].data_ptr() >= 1 << 32

    def fill(x_i8):
        near = [S.to_cl(x_i8[:, :c_src].float(), dtype), S.to_cl(x_i8[:, c_src:].float(), dtype)]
        for f, s in zip(far, near):
            f.copy_(s)
        return near

    x = ints((n, 2 * c_src, d, h, w), -3, 3, 4000)
    wt = ints((cout, 2 * c_src, 3, 3, 3), -3, 3, 4001).float()
    b = ints((cout,), -3, 3, 4002).float()
    near = fill(x)
    ref = F.conv3d(x.cpu().float(), wt.cpu(), b.cpu(), padding=1)
    (raw_far,), part_far, slots = S.conv3d_march(far, wt, b, 1, want_stats=True)
    (raw_near,), part_near, _ = S.conv3d_march(near, wt, b, 1, want_stats=True)
    assert_same(S.from_cl(raw_far), rounded(ref, dtype), f"forward, sources 4 GB apart ({dtype})")
    assert_same(raw_far, raw_near, f"forward, sources 4 GB apart against adjacent sources ({dtype})")
    assert torch.equal(part_far, part_near)

    x = ints((n, 2 * c_src, d, h, w), -1, 1, 4003)
    dy = ints((n, cout, d, h, w), -1, 1, 4004)
    fill(x)
    dy_cl = S.to_cl(dy.float(), dtype)
    ref = torch.nn.grad.conv3d_weight(x.cpu().float(), (cout, 2 * c_src, 3, 3, 3), dy.cpu().float(), padding=1)
    dw = S.conv3d_wgrad(far, dy_cl, 2 * c_src, cout, 27, 1, lib.CONV_MFMA)
    assert_same(dw.cpu(), ref, f"weight gradient, sources 4 GB apart ({dtype})", axes=("co", "ci", "tap"))
    assert_same(S.conv3d_wgrad(far, dy_cl, 2 * c_src, cout, 27, 1, lib.CONV_TILED), dw, "routed call against the tiled kernel",
                axes=("co", "ci", "tap"))
    with pytest.raises(RuntimeError, match="wgrad_march"):
        S.conv3d_wgrad(far, dy_cl, 2 * c_src, cout, 27, 1, lib.CONV_MARCH)


# ---------------------------------------------------------------------------------------------------
# the plan of one sample, and the source distances of the plan of sixteen
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ONE.CASES, ids=_ids)
def test_batch_1_forward_and_statistics(S, case):
    L.forward_case(S, ONE, case)


@pytest.mark.parametrize("case", ONE.DGRAD_CASES, ids=_ids)
def test_batch_1_data_gradient(S, case):
    L.dgrad_case(S, ONE, case)


@pytest.mark.parametrize("case", ONE.CASES, ids=_ids)
def test_batch_1_weight_gradient(S, case):
    L.wgrad_case(S, ONE, case)


@pytest.mark.parametrize("case", [(n, dt) for n in PAIRED for dt in DTYPES], ids=_ids)
def test_batch_16_forward_of_the_two_source_layers(S, case):
    """Samples 0, 8 and 15 of the 16 x 128^3 forward: the first, one in the middle and the last (every sample of dc5's second
    source lies 2^31 bytes or more past the first source's base; its last ends at 2^32)."""
    L.forward_samples_case(S, BIG, case[0], case[1], (0, 8, 15))
