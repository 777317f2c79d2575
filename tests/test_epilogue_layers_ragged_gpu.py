"""Every epilogue, pooling, up-sampling and head pass of a training step at NON-CUBIC shapes whose extents leave the slot counts,
z segments and tiles of those kernels ragged, against the float64 restatement (tests/epilogue_ref.py) under the DERIVED bounds of
the benchmark module, and bitwise wherever the operation only selects or rounds once (method, tolerances and case functions:
tests/epilogue_layer_cases.py; the configurations and what each reaches: tests/epilogue_ragged_cases.py; the host-side proof that
the cases test what they name: tests/test_epilogue_ragged_host.py).  The extents are those of the ragged convolution module
(tests/test_conv_layers_ragged_gpu.py): the same volumes get both halves of a step tested.

The other epilogue modules run cubes (128^3, 160^3): a kernel that takes H's stride, scale or extent where W's or D's is meant
gives the right answer there, every z segment of the up-sampling kernels is full, and ``epi_partials`` takes the wave-quantised
branch with a count the batch divides (128^3) or the cap and the floor branch (160^3).  Here:

  A   1 x 2 x (72, 56, 88), width 1, bf16 and fp16 (fp32 on levels 2 and 3): every case list, both heads' passes, the
      block-by-block forward.  Slots 256 / 256 / 43 / 5, level 3 = (9, 7, 11), up-sampling from D = 9 / 18 / 36 (last segments of
      1 / 2 / 4 coarse planes), heads' row form with a partial y block, backward x pass on the table walk for its tap count
  A2  the same extents at width 2, bf16: gate, aggregation and up-sampling cases on 128-channel lanes
  B   2 x 2 x (104, 152, 136), width 1, levels 1 to 3: up-sampling from (13, 19, 17), (26, 38, 34), (52, 76, 68) (8-plane segments,
      the last half empty), batch 2 below the quantisation threshold
  B heads  1 x (40, 24, 136) with 4 levels (two passes of a wave over the row; the backward's register fast path with level-1
      entries in the second slot) and 1 x (16, 40, 20) with 3 levels (the per-voxel forward)
  C   5 x 2 x (24, 40, 56), level 0, bf16, gate and aggregation cases: 153 slots per sample, 765 per launch

and the heads refuse extents that 2^(levels - 1) does not divide (W = 28 with 4 levels would lose 3 of 27 taps in the backward's x
pass).  No tolerance is new: every K and L is the function of the channel count, the slot count and the extents that the cubes use,
per axis where a cube could use one number for three."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_layer_cases as E  # noqa: E402
import epilogue_ragged_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu

A, A2, B, C5 = (R.configs()[k] for k in ("A", "A2", "B", "C"))
# what each configuration is there for (a moved threshold would make the cases below pass vacuously)
for _key, _cfg in R.configs().items():
    assert R.facts(_cfg) == R.EXPECT[_key], (_key, R.facts(_cfg))
assert len(A.PLAN_LIST) == 24 and len(A.GATED) == len(A2.GATED) == 18 and len(A.AGG) == len(A2.AGG) == 6
assert {b["C"] for b in A.BLOCKS.values()} == {8, 16, 32, 64} and {b["C"] for b in A2.BLOCKS.values()} == {16, 32, 64, 128}
assert {b["gates"] for b in A.BLOCKS.values() if b["gated"]} == {1, 2}
assert [A.SLOTS[l] for l in range(4)] == [256, 256, 43, 5] and [B.SLOTS[l] for l in (1, 2, 3)] == [256, 256, 32] and C5.SLOTS[0] == 153
assert A.BLOCKS["ec10"]["dims"] == (1, 9, 7, 11) and B.BLOCKS["ec10"]["dims"] == (2, 13, 19, 17)
assert all(R.last_trip(c.BLOCKS[n]["dims"], c.BLOCKS[n]["C"]) for c in (A, A2, B, C5) for n in c.GATED + c.AGG)
assert [(c, d[1:]) for _, c, d in A.UPS] == [(64, (9, 7, 11)), (64, (18, 14, 22)), (32, (36, 28, 44))]
assert [(c, d[1:]) for _, c, d in A2.UPS] == [(128, (9, 7, 11)), (128, (18, 14, 22)), (64, (36, 28, 44))]
assert [(c, d[1:]) for _, c, d in B.UPS] == [(64, (13, 19, 17)), (64, (26, 38, 34)), (32, (52, 76, 68))]
assert len(A.POOLS) == 3 and len(A.POOLS_X) == 2 and len(B.POOLS) == 2 and len(B.POOLS_X) == 1
assert {B.BLOCKS[n]["level"] for n in B.GATED + B.AGG} == {1, 2, 3} and {C5.BLOCKS[n]["level"] for n in C5.GATED + C5.AGG} == {0}
assert len(C5.GATED) == 5 and C5.AGG_X == ["ec33"] and not C5.AGG1_CASES, (C5.GATED, C5.AGG)
assert R.head_x_path(88, 4)[:2] == (77, False) and R.head_x_path(136, 4) == (119, True, [1, 2, 3])
_HEAD_IDS = ["x".join(map(str, s.extent)) + f"-{nl}" for s, nl in R.HEADS_B]


@pytest.fixture(scope="module")
def S():
    return E.ops_or_skip()


# ---- A ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.GATE_CASES, ids=E.ids)
def test_a_gate_stats_and_forward(S, case):
    E.gate_stats_and_forward(S, A, case)


@pytest.mark.parametrize("case", A.GATE_CASES, ids=E.ids)
def test_a_gate_backward(S, case):
    E.gate_backward(S, A, case)


@pytest.mark.parametrize("case", A.X_CASES, ids=E.ids)
def test_a_aggregation_x_pool_forward_and_backward(S, case):
    E.aggregation_x_pool_forward_and_backward(S, A, case)


@pytest.mark.parametrize("case", A.AGG1_CASES, ids=E.ids)
def test_a_aggregation_one_branch(S, case):
    E.aggregation_one_branch(S, A, case)


@pytest.mark.parametrize("case", A.POOL_FWD_CASES, ids=E.ids)
def test_a_maxpool_forward(S, case):
    E.maxpool_forward(S, case)


@pytest.mark.parametrize("case", A.POOL_BWD_CASES, ids=E.ids)
def test_a_maxpool_backward(S, case):
    E.maxpool_backward(S, case)


@pytest.mark.parametrize("case", A.UP_CASES, ids=E.ids)
def test_a_upsample_forward(S, case):
    E.upsample_forward(S, case)


@pytest.mark.parametrize("case", A.UP_BWD_CASES, ids=E.ids)
def test_a_upsample_backward(S, case):
    E.upsample_backward(S, case)


@pytest.mark.parametrize("nlevels", R.HEAD_A)
def test_a_head_forward(S, nlevels):
    E.head_forward(S, A, nlevels)


@pytest.mark.parametrize("nlevels", R.HEAD_A)
def test_a_head_backward(S, nlevels):
    E.head_backward(S, A, nlevels)


@pytest.mark.parametrize("dtype", ("bf16", "fp16"))
def test_a_network_forward_block_by_block(S, dtype):
    E.network_forward_block_by_block(S, A, dtype)


# ---- A2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A2.GATE_CASES, ids=E.ids)
def test_a2_gate_stats_and_forward(S, case):
    E.gate_stats_and_forward(S, A2, case)


@pytest.mark.parametrize("case", A2.GATE_CASES, ids=E.ids)
def test_a2_gate_backward(S, case):
    E.gate_backward(S, A2, case)


@pytest.mark.parametrize("case", A2.X_CASES, ids=E.ids)
def test_a2_aggregation_x_pool_forward_and_backward(S, case):
    E.aggregation_x_pool_forward_and_backward(S, A2, case)


@pytest.mark.parametrize("case", A2.AGG1_CASES, ids=E.ids)
def test_a2_aggregation_one_branch(S, case):
    E.aggregation_one_branch(S, A2, case)


@pytest.mark.parametrize("case", A2.UP_CASES, ids=E.ids)
def test_a2_upsample_forward(S, case):
    E.upsample_forward(S, case)


@pytest.mark.parametrize("case", A2.UP_BWD_CASES, ids=E.ids)
def test_a2_upsample_backward(S, case):
    E.upsample_backward(S, case)


# ---- B ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.GATE_CASES, ids=E.ids)
def test_b_gate_stats_and_forward(S, case):
    E.gate_stats_and_forward(S, B, case)


@pytest.mark.parametrize("case", B.GATE_CASES, ids=E.ids)
def test_b_gate_backward(S, case):
    E.gate_backward(S, B, case)


@pytest.mark.parametrize("case", B.X_CASES, ids=E.ids)
def test_b_aggregation_x_pool_forward_and_backward(S, case):
    E.aggregation_x_pool_forward_and_backward(S, B, case)


@pytest.mark.parametrize("case", B.AGG1_CASES, ids=E.ids)
def test_b_aggregation_one_branch(S, case):
    E.aggregation_one_branch(S, B, case)


@pytest.mark.parametrize("case", B.POOL_FWD_CASES, ids=E.ids)
def test_b_maxpool_forward(S, case):
    E.maxpool_forward(S, case)


@pytest.mark.parametrize("case", B.POOL_BWD_CASES, ids=E.ids)
def test_b_maxpool_backward(S, case):
    E.maxpool_backward(S, case)


@pytest.mark.parametrize("case", B.UP_CASES, ids=E.ids)
def test_b_upsample_forward(S, case):
    E.upsample_forward(S, case)


@pytest.mark.parametrize("case", B.UP_BWD_CASES, ids=E.ids)
def test_b_upsample_backward(S, case):
    E.upsample_backward(S, case)


@pytest.mark.parametrize("shape,nlevels", R.HEADS_B, ids=_HEAD_IDS)
def test_b_head_forward(S, shape, nlevels):
    E.head_forward(S, shape, nlevels)


@pytest.mark.parametrize("shape,nlevels", R.HEADS_B, ids=_HEAD_IDS)
def test_b_head_backward(S, shape, nlevels):
    E.head_backward(S, shape, nlevels)


# ---- C ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C5.GATE_CASES, ids=E.ids)
def test_c_gate_stats_and_forward(S, case):
    E.gate_stats_and_forward(S, C5, case)


@pytest.mark.parametrize("case", C5.GATE_CASES, ids=E.ids)
def test_c_gate_backward(S, case):
    E.gate_backward(S, C5, case)


@pytest.mark.parametrize("case", C5.X_CASES, ids=E.ids)
def test_c_aggregation_x_pool_forward_and_backward(S, case):
    """(Level 0 has one aggregation block, ec33, and it has the x-branch: no one-branch case.)"""
    E.aggregation_x_pool_forward_and_backward(S, C5, case)


# ---- extents the levels do not divide -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", R.HEADS_REFUSED, ids=lambda e: "x".join(map(str, e)))
def test_heads_refuse_extents_the_levels_do_not_divide(S, ext):
    """4 levels ask for multiples of 8.  At W = 28 level 3 has 28 >> 3 = 3 columns whose middle one has 27 taps along x, three more
    than a table row of the backward's x pass holds: both passes return an error before they launch anything, and the level
    gradients keep what they held.  With 3 levels the same extents are multiples of 4 and are served."""
    from seunet_amd import _lib
    lib = _lib.load()
    d, h, w = ext
    assert any(e % 8 for e in ext) and all(e % 4 == 0 for e in ext)
    maps = [torch.zeros((1, d >> l, h >> l, w >> l), device="cuda") for l in range(4)]
    bias = torch.zeros(1, device="cuda")
    with pytest.raises(RuntimeError, match=r"head_fwd: extents \(\d+, \d+, \d+\) must be multiples of 8 for 4 levels"):
        S.head_fwd(maps, bias)
    g = torch.ones((1, 1, d, h, w), device="cuda")
    with pytest.raises(RuntimeError, match=r"head_bwd: extents \(\d+, \d+, \d+\) must be multiples of 8 for 4 levels"):
        S.head_bwd(g, 4)
    # nothing is launched: the outputs keep their fill
    dims = _lib.Dims(1, d, h, w)
    levels = [None] + [torch.full_like(m, 123.0) for m in maps[1:]]
    tmp = torch.full((lib.seunet_head_bwd_tmp_floats(dims),), 123.0, device="cuda")
    gb = torch.full((1,), 123.0, device="cuda")
    status = lib.seunet_head_bwd(g.data_ptr(), _lib.ptr_array(levels), 4, tmp.data_ptr(), gb.data_ptr(), dims, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert status != 0 and "must be multiples of 8" in _lib.last_error()
    assert all(bool((t == 123.0).all()) for t in levels[1:] + [tmp, gb])
    pred = torch.full((1, 1, d, h, w), 123.0, device="cuda")
    status = lib.seunet_head_fwd(_lib.ptr_array(maps), 4, bias.data_ptr(), pred.data_ptr(), dims, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert status != 0 and bool((pred == 123.0).all())
    # three levels: served, under the bounds of every other head case
    E.head_forward(S, R.HeadShape(1, ext), 3)
    E.head_backward(S, R.HeadShape(1, ext), 3)
