"""Every epilogue, pooling, up-sampling and head pass of a training step of BASELINE.json's configs[4] -- 2 x 2 x 160^3, 2x
channel width -- against the float64 restatement (tests/epilogue_ref.py) under the DERIVED bounds of the benchmark module, and
bitwise wherever the operation only selects or rounds once.  Method, tolerances and case functions:
tests/epilogue_layer_cases.py; every K and L there is a function of lg = log2(C / 8), of the slot count and of the extents.

What this configuration adds: 128-channel gated and aggregation blocks (16 lanes per voxel), extents 160 / 80 / 40 / 20 that
are not multiples of 32, and the two branches of ``seunet_epilogue_slots`` the benchmark shapes do not reach -- the cap of 256
records per sample (levels 0 to 2) and the floor branch with a ragged split (level 3: 8000 voxels over 62 records, 16 voxels per
block and trip at 128 channels: the last trip of a block is partly empty)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_layer_cases as E  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH, EXTENT, WIDTH = 2, 160, 2
CFG = E.Config(BATCH, EXTENT, WIDTH)
BLOCKS = CFG.BLOCKS
assert len(CFG.PLAN_LIST) == 24 and len(CFG.GATED) == 18 and len(CFG.AGG) == 6, (CFG.GATED, CFG.AGG)
assert {b["C"] for b in BLOCKS.values()} == {16, 32, 64, 128} and {b["level"] for b in BLOCKS.values()} == {0, 1, 2, 3}
assert {(b["C"], b["gates"]) for b in BLOCKS.values() if b["gated"]} == {(16, 1), (32, 1), (64, 1), (64, 2), (128, 2)}
assert all(b["dims"] == (BATCH, EXTENT >> b["level"], EXTENT >> b["level"], EXTENT >> b["level"]) for b in BLOCKS.values())
assert all(BLOCKS[n]["pool"] for n in CFG.AGG_X) and len(CFG.AGG_X) == 3 and len(CFG.AGG_1) == 3, (CFG.AGG_X, CFG.AGG_1)
assert sorted(BLOCKS[n]["slot"] for n in CFG.GATED if BLOCKS[n]["head"] == 0) == list(range(12))
assert sorted(BLOCKS[n]["slot"] for n in CFG.GATED if BLOCKS[n]["head"] == 1) == list(range(6))
# the cap (256 records) on levels 0 - 2, the floor branch (8000 // 128 = 62, not a divisor of 8000) on level 3
assert [CFG.SLOTS[l] for l in range(4)] == [256, 256, 256, 62], CFG.SLOTS
assert 8000 % 62 != 0 and E.thread_chain((BATCH, 20, 20, 20), 128) == 9 and 62 * 16 * 9 > 8000 > 62 * 16 * 8
assert [(c, d[1]) for _, c, d in CFG.UPS] == [(128, 20), (128, 40), (64, 80)], CFG.UPS
assert [(c, d[1]) for _, c, d in CFG.POOLS] == [(64, 160), (128, 80), (128, 40)] and len(CFG.POOLS_X) == 2, (CFG.POOLS, CFG.POOLS_X)
X_CASES = CFG.X_CASES


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
