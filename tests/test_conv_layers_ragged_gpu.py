"""Every convolution pass of three NON-CUBIC plans whose extents leave every tile of the kernel family ragged, at the layer's
own shape and on the kernel the plan routes it to, BITWISE (method and helpers: tests/conv_layer_cases.py; the configurations,
their routing and what each level reaches: tests/conv_ragged_cases.py; the host-side proof that the cases test what they name:
tests/test_conv_ragged_host.py).

The other layer modules run cubes (128^3, 160^3) that are multiples of every tile: no x tail, no y tail, equal axes, an even
plane count per dilation-2 parity class, and the cuts (z segments, slabs, ``march_zsteps``) of those shapes only.  Here:

  A   1 x 2 x (72, 56, 88), width 1, bf16 and fp16: x tails of 24, 12 and 22 columns, H = 3 * 8 + 4 on the marching level,
      a marching weight gradient with W = 22 < 32, odd extents (9, 7, 11) on level 3
  A2  the same extents at width 2, bf16: ec3 / dc6 on the marching kernel at full resolution with a 24-column x tail,
      256-input-channel marching weight gradients on ragged rows
  B   2 x 2 x (104, 152, 136), width 1, bf16 and fp16, levels 1 to 3: x tails of 4 and 2 columns, H = 9 * 8 + 4 and
      9 * 4 + 2, 13 planes per parity class, the whole-GEMM 1x1x1 weight gradient on 268 736 voxels per sample (no multiple of
      its 128-voxel chunk), two-source layers at the source distance a non-cubic arena gives them
  C   3 x 2 x (104, 152, 136), the weight gradient of ec63 alone: the whole-GEMM kernel chunks the flat (sample, voxel) index,
      which at batch 2 is always a multiple of 128; three samples leave its last chunk half empty

Values are compared bitwise with a float32 ``F.conv3d`` of exact small integers; the InstanceNorm statistics keep the bars of
the benchmark module (mean atol 2e-5, rstd rtol 2e-4 against float64 statistics of the exact result)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_layer_cases as L  # noqa: E402
import conv_ragged_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu

(A, _RA), (A2, _RA2), (B, _RB), (C3, _RC) = (R.configs()[k] for k in ("A", "A2", "B", "C"))
# the routing these cases are named for, the same in bf16 and fp16 (a plan that silently routed everything to one kernel would
# make the cases below pass vacuously)
for _cfg, _want in ((A, _RA), (A2, _RA2), (B, _RB)):
    assert not R.misrouted(_cfg, _want), R.misrouted(_cfg, _want)
    assert len(_cfg.PLANS[_cfg.dtypes[0]]) == 24 and all(list(_cfg.PLANS[dt]) == list(_cfg.PLANS[_cfg.dtypes[0]]) for dt in _cfg.dtypes)
_ALL9 = {(k, p) for k in ("Stream", "March", "Tiled") for p in ("fwd", "dgrad", "wgrad")}
assert _ALL9 <= A.ROUTED and _ALL9 <= A2.ROUTED, (sorted(A.ROUTED), sorted(A2.ROUTED))
# (B.ROUTED describes the whole plan; what B runs is its levels 1 to 3, where nothing streams)
_B_RUN = {(c[p], p) for dt in B.dtypes for n, c in B.PLANS[dt].items() if n in B.LAYERS for p in ("fwd", "dgrad", "wgrad") if c[p]}
assert _B_RUN == {(k, p) for k in ("March", "Tiled") for p in ("fwd", "dgrad", "wgrad")} | {("Wgrad1x1", "wgrad")}, sorted(_B_RUN)
assert _B_RUN < B.ROUTED and all(c["level"] in (1, 2, 3) for n, c in B.PLANS["bf16"].items() if n in B.LAYERS)
assert len(A.LAYERS) == 24 and len(A2.LAYERS) == 24 and len(B.LAYERS) == 18 and "dc5" not in B.LAYERS and "ec1" not in B.LAYERS
_PA, _PA2, _PB = A.PLANS["bf16"], A2.PLANS["bf16"], B.PLANS["bf16"]
assert _PA["dc5"]["dims"] == (1, 72, 56, 88) and A.passes("dc5") == ("March",) * 3
assert _PA["ec5"]["dims"] == (1, 36, 28, 44) and A.passes("ec5") == A.passes("ec6") == ("March",) * 3 and A.passes("ec4") == ("Tiled",) * 3
assert _PA["ec8"]["dims"] == (1, 18, 14, 22) and A.passes("ec8") == A.passes("ec9") == ("Tiled", "Tiled", "March")
assert _PA["ec10"]["dims"] == (1, 9, 7, 11)
assert A2.passes("ec3") == A2.passes("dc6") == ("March",) * 3 and A2.passes("dc5") == ("Tiled", "March", "March")
assert (_PA2["ec3"]["src_c"], _PA2["ec3"]["cout"], _PA2["dc1"]["cin"], _PA2["dc3"]["cin"]) == ([32], 64, 256, 256)
assert _PB["ec4"]["dims"] == (2, 52, 76, 68) and all(B.passes(n) == ("March",) * 3 for n in ("ec4", "ec5", "ec6", "dc4", "ec8", "ec9"))
assert B.passes("dc3") == ("Tiled", "March", "March") and B.passes("ec63")[2] == "Wgrad1x1" and A.passes("ec63")[2] == "Tiled"
assert _PB["ec8"]["dims"] == (2, 26, 38, 34) and _PB["ec10"]["dims"] == (2, 13, 19, 17)
_EC63 = [c for c in C3.CASES if c[0] == "ec63"]
assert len(_EC63) == 2 and all(C3.PLANS[dt]["ec63"]["dims"] == (3, 52, 76, 68) and C3.passes("ec63", dt)[2] == "Wgrad1x1" for dt in C3.dtypes)
assert (2 * 52 * 76 * 68) % 128 == 0 and (3 * 52 * 76 * 68) % 128 == 64 and 3 * 52 * 76 * 68 < 1 << 24


@pytest.fixture(scope="module")
def S():
    return L.ops_or_skip()


@pytest.mark.parametrize("case", A.CASES, ids=L.ids)
def test_a_forward_and_statistics(S, case):
    L.forward_case(S, A, case)


@pytest.mark.parametrize("case", A.DGRAD_CASES, ids=L.ids)
def test_a_data_gradient(S, case):
    """Overwrite, ``+=`` and a null first destination: see ``conv_layer_cases.dgrad_case``."""
    L.dgrad_case(S, A, case)


@pytest.mark.parametrize("case", A.CASES, ids=L.ids)
def test_a_weight_gradient(S, case):
    """Routed, forced and a second run: see ``conv_layer_cases.check_wgrad``."""
    L.wgrad_case(S, A, case)


@pytest.mark.parametrize("case", A2.CASES, ids=L.ids)
def test_a2_forward_and_statistics(S, case):
    L.forward_case(S, A2, case)


@pytest.mark.parametrize("case", A2.DGRAD_CASES, ids=L.ids)
def test_a2_data_gradient(S, case):
    L.dgrad_case(S, A2, case)


@pytest.mark.parametrize("case", A2.CASES, ids=L.ids)
def test_a2_weight_gradient(S, case):
    L.wgrad_case(S, A2, case)


@pytest.mark.parametrize("case", B.CASES, ids=L.ids)
def test_b_forward_and_statistics(S, case):
    L.forward_case(S, B, case)


@pytest.mark.parametrize("case", B.DGRAD_CASES, ids=L.ids)
def test_b_data_gradient(S, case):
    L.dgrad_case(S, B, case)


@pytest.mark.parametrize("case", B.CASES, ids=L.ids)
def test_b_weight_gradient(S, case):
    L.wgrad_case(S, B, case)


@pytest.mark.parametrize("case", _EC63, ids=L.ids)
def test_c_whole_gemm_weight_gradient_with_a_ragged_last_chunk(S, case):
    """ec63 at 3 x (52, 76, 68): 806 208 = 6 298 * 128 + 64 voxels of the flat index (tests/conv_ragged_cases.py, C)."""
    L.wgrad_case(S, C3, case)
