"""Every epilogue, pooling, up-sampling and head pass of a training step, at the shape and storage type the benchmark runs it
with, against a float64 restatement (tests/epilogue_ref.py) under DERIVED bounds -- and bitwise wherever the operation only
selects or rounds once.  Method, tolerances and case functions: tests/epilogue_layer_cases.py.

The cases are generated from ``SE_UNet.conv_plan`` for the benchmarked configuration (4 x 2 x 128^3, width 1) and from the
module's own blocks, so a block that is added later is covered without editing this file; the extents that are not powers of
two (np2-*) run here as well.  The 160^3 width-2 configuration has its own module, tests/test_epilogue_layers_config4_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_layer_cases as E  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH, EXTENT = 4, 128
CFG = E.Config(BATCH, EXTENT, 1)
PLAN_LIST, NET, SLOTS, PLAN, BLOCKS = CFG.PLAN_LIST, CFG.NET, CFG.SLOTS, CFG.PLAN, CFG.BLOCKS
GATED, AGG, AGG_X, AGG_1, UPS, POOLS, POOLS_X = CFG.GATED, CFG.AGG, CFG.AGG_X, CFG.AGG_1, CFG.UPS, CFG.POOLS, CFG.POOLS_X
assert len(PLAN_LIST) == 24 and len(GATED) == 18 and len(AGG) == 6, (GATED, AGG)
assert {b["C"] for b in BLOCKS.values()} == {8, 16, 32, 64} and {b["level"] for b in BLOCKS.values()} == {0, 1, 2, 3}
assert {b["gates"] for n, b in BLOCKS.items() if b["gated"]} == {1, 2}
assert all(BLOCKS[n]["pool"] for n in AGG_X) and len(AGG_X) == 3 and len(AGG_1) == 3, (AGG_X, AGG_1)
assert sorted(BLOCKS[n]["slot"] for n in GATED if BLOCKS[n]["head"] == 0) == list(range(12))
assert sorted(BLOCKS[n]["slot"] for n in GATED if BLOCKS[n]["head"] == 1) == list(range(6))
# the wave-quantised branch of the slot count is the one these cases run
assert [SLOTS[l] for l in range(4)] == [192, 192, 192, 32], SLOTS
assert [(c, d[1]) for _, c, d in UPS] == [(64, 16), (64, 32), (32, 64)], UPS
assert len(POOLS) == 3 and len(POOLS_X) == 2
X_CASES = CFG.X_CASES + E.NONPOW2_CASES


@pytest.fixture(scope="module")
def S():
    return E.ops_or_skip()


@pytest.mark.parametrize("case", CFG.GATE_CASES, ids=E.ids)
def test_gate_stats_and_forward(S, case):
    E.gate_stats_and_forward(S, CFG, case)


@pytest.mark.parametrize("case", CFG.GATE_CASES, ids=E.ids)
def test_gate_backward(S, case):
    E.gate_backward(S, CFG, case)


@pytest.mark.parametrize("case", X_CASES, ids=E.ids)
def test_aggregation_x_pool_forward_and_backward(S, case):
    E.aggregation_x_pool_forward_and_backward(S, CFG, case)


@pytest.mark.parametrize("case", CFG.AGG1_CASES, ids=E.ids)
def test_aggregation_one_branch(S, case):
    E.aggregation_one_branch(S, CFG, case)


@pytest.mark.parametrize("case", CFG.POOL_FWD_CASES, ids=E.ids)
def test_maxpool_forward(S, case):
    E.maxpool_forward(S, case)


@pytest.mark.parametrize("case", CFG.POOL_BWD_CASES, ids=E.ids)
def test_maxpool_backward(S, case):
    E.maxpool_backward(S, case)


@pytest.mark.parametrize("case", CFG.UP_CASES, ids=E.ids)
def test_upsample_forward(S, case):
    E.upsample_forward(S, case)


@pytest.mark.parametrize("case", CFG.UP_BWD_CASES, ids=E.ids)
def test_upsample_backward(S, case):
    E.upsample_backward(S, case)


@pytest.mark.parametrize("nlevels", (4, 3))
def test_head_forward(S, nlevels):
    E.head_forward(S, CFG, nlevels)


@pytest.mark.parametrize("nlevels", (4, 3))
def test_head_backward(S, nlevels):
    E.head_backward(S, CFG, nlevels)


@pytest.mark.parametrize("dtype", ("bf16", "fp16"))
def test_network_forward_block_by_block(S, dtype):
    E.network_forward_block_by_block(S, CFG, dtype)
