"""Every convolution pass of the plan of BASELINE.json's configs[4] -- 2x channel width, 160^3 patches, 16-bit storage -- at
the layer's own shape and on the kernel the plan routes it to, BITWISE (method and helpers: tests/conv_layer_cases.py).

Kernel routing and work decomposition depend on the descriptor, and this one meets combinations the benchmarked 4 x 2 x 128^3
width-1 plan does not: marching kernels at full resolution on 160-voxel rows (five 32-voxel x tiles) and on 80-voxel rows
(2 1/2 tiles) with 64 -> 128 and 128 -> 64 channels, 256-input-channel marching weight gradients at 80^3 and at 40^3 (ragged
40-voxel rows), tiled kernels at 20^3 and 40^3 with 128 channels, and segment seams of ``march_zsteps`` for N = 2.

The exactness argument with this plan's numbers: operands in {-3..3} and at most 256 input channels under 27 taps give
|sum| <= 27 * 256 * 9 + 3 = 62 211 < 2^24 for the forward and the data gradient (exact in f32 in any order), and 62 211 + 3 for
``+=`` stays below 65 504, so fp16 storage does not overflow; the weight gradient's operands are in {-1, 0, 1} and its sums are
bounded by N * voxels = 2 * 160^3 = 8 192 000 < 2^24.  The statistics keep the bars of the benchmark module (mean atol 2e-5, rstd
rtol 2e-4 against float64 statistics of the exact result).

Batch 2 is the batch of ``scripts/bench_configs.py`` and of ``test_config4_shape_160_width2_properties``."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_layer_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH, EXTENT, WIDTH = 2, 160, 2
CFG = L.Config(BATCH, EXTENT, WIDTH)
# the routing of this configuration (fwd, dgrad, wgrad), the same in bf16 and fp16: a later re-route shows up as an edit here
ROUTING = {
    "ec1": ("Stream", None, "Stream"), "ec2": ("Stream", "Stream", "Stream"),
    "ec3": ("March", "March", "March"), "dc6": ("March", "March", "March"),           # 160^3, 32 -> 64 dilation 2 / 64 -> 32
    "dc5": ("Tiled", "March", "March"),                                               # 160^3, [64, 64] -> 64
    "ec4": ("March", "March", "March"), "ec5": ("March", "March", "March"),           # 80^3, 64 -> 64
    "ec6": ("March", "Tiled", "March"),                                               # 80^3, 64 -> 128, dilation 2
    "dc4": ("Tiled", "March", "March"),                                               # 80^3, 128 -> 64
    "dc3": ("Tiled", "Tiled", "March"),                                               # 80^3, [128, 128] -> 128
    "ec8": ("Tiled", "Tiled", "March"), "ec9": ("Tiled", "Tiled", "March"),           # 40^3, 128 -> 128, dilation 2
    "dc1": ("Tiled", "Tiled", "March"),                                               # 40^3, [128, 128] -> 128
    "ec63": ("Tiled", "Tiled", "Tiled"),                                              # 80^3, 1x1x1, 256 -> 128
}
for _dt in L.DTYPES:
    for _n, _want in ROUTING.items():
        assert CFG.passes(_n, _dt) == _want, (_n, _dt, CFG.passes(_n, _dt), _want)
_P = CFG.PLANS["bf16"]
assert len(CFG.LAYERS) == 24 and all(list(CFG.PLANS[dt]) == CFG.LAYERS for dt in L.DTYPES), CFG.LAYERS
assert all(c["dims"] == (BATCH, EXTENT >> c["level"], EXTENT >> c["level"], EXTENT >> c["level"]) for c in _P.values())
assert (_P["ec3"]["src_c"], _P["ec3"]["cout"], _P["ec3"]["dilation"]) == ([32], 64, 2) and (_P["dc6"]["src_c"], _P["dc6"]["cout"]) == ([64], 32)
assert (_P["dc5"]["src_c"], _P["dc5"]["cout"]) == ([64, 64], 64) and (_P["ec6"]["src_c"], _P["ec6"]["cout"], _P["ec6"]["dilation"]) == ([64], 128, 2)
assert (_P["dc4"]["src_c"], _P["dc4"]["cout"]) == ([128], 64) and (_P["dc3"]["src_c"], _P["dc1"]["src_c"]) == ([128, 128], [128, 128])
assert (_P["ec63"]["cin"], _P["ec63"]["cout"], _P["ec63"]["taps"]) == (256, 128, 1)
# not vacuous: what this plan adds to the benchmark's set of (kernel, pass, shape) combinations is really routed
assert any(c["fwd"] == "March" and c["cout"] == 128 for c in _P.values())
assert any(c["wgrad"] == "March" and c["cin"] == 256 and c["dims"][1] == 80 for c in _P.values())
assert any(c["wgrad"] == "March" and c["cin"] == 256 and c["dims"][1] == 40 for c in _P.values())
assert any(c["fwd"] == "March" and c["dims"][1] == 160 for c in _P.values()) and _P["ec6"]["dgrad"] == "Tiled"
assert {("March", "fwd"), ("March", "dgrad"), ("March", "wgrad"), ("Tiled", "fwd"), ("Tiled", "dgrad"), ("Tiled", "wgrad"),
        ("Stream", "fwd"), ("Stream", "dgrad"), ("Stream", "wgrad")} <= CFG.ROUTED, sorted(CFG.ROUTED)


@pytest.fixture(scope="module")
def S():
    return L.ops_or_skip()


@pytest.mark.parametrize("case", CFG.CASES, ids=L.ids)
def test_forward_and_statistics(S, case):
    L.forward_case(S, CFG, case)


@pytest.mark.parametrize("case", CFG.DGRAD_CASES, ids=L.ids)
def test_data_gradient(S, case):
    """Overwrite, ``+=`` and a null first destination: see ``conv_layer_cases.dgrad_case``."""
    L.dgrad_case(S, CFG, case)


@pytest.mark.parametrize("case", CFG.CASES, ids=L.ids)
def test_weight_gradient(S, case):
    L.wgrad_case(S, CFG, case)
