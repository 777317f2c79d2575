"""The ragged epilogue / resampling / head cases test what they name (host only, no GPU).

tests/test_epilogue_layers_ragged_gpu.py runs the case functions of tests/epilogue_layer_cases.py on the non-cubic configurations
of tests/epilogue_ragged_cases.py.  Its worth lies in WHICH branch of ``epi_partials`` a level takes, in how the extents meet the z
segments and tiles of the up-sampling kernels, and in which path the heads' kernels take; all of that is decided on the host (the
launch cuts) or follows from the extents alone, so it is proved here, where a moved threshold fails a test on a CPU-only build
instead of quietly emptying a GPU case.

Restated from the sources (the cuts that have a query are asked through it):
  pass A of every epilogue (csrc/epilogue.h): 256 threads, C / 8 lanes per voxel, so 256 / (C / 8) voxels per block and trip; a block
    strides over the sample by slots x that many voxels
  forward march (csrc/resample.hip): UFM_ZSF = 16 fine planes per z segment, 4096 / C fine columns per block
  backward march: ZS = 8 coarse planes per segment when D >= 32, else 4; TY = 128 / C coarse rows and UM_TX = 16 coarse columns
    per block
  heads (csrc/heads.hip): the row form of the forward (W % 8 == 0) cuts a plane into blocks of 4 waves x 4 rows; the x pass of the
    backward keeps HB_K = 24 weights per table entry and has a register fast path for <= 128 entries with <= HB_KA = 8 taps in a
    lane's first entry
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_ragged_cases as R  # noqa: E402

cdiv = lambda a, b: -(-a // b)


@pytest.fixture(scope="module")
def CFGS():
    return R.configs()


def test_configurations_are_the_stated_ones(CFGS):
    a, a2, b, c = (CFGS[k] for k in ("A", "A2", "B", "C"))
    assert (a.batch, a.extent, a.width, a.levels, a.dtypes) == (1, (72, 56, 88), 1, None, None)
    assert (a2.batch, a2.extent, a2.width, a2.levels, a2.dtypes) == (1, (72, 56, 88), 2, None, ("bf16",))
    assert (b.batch, b.extent, b.width, b.levels, b.dtypes) == (2, (104, 152, 136), 1, (1, 2, 3), None)
    assert (c.batch, c.extent, c.width, c.levels, c.dtypes) == (5, (24, 40, 56), 1, (0,), ("bf16",))
    for cfg in (a, a2, b, c):
        d, h, w = cfg.extent
        assert len(cfg.PLAN_LIST) == len(cfg.BLOCKS) == 24                       # PLAN and BLOCKS stay whole
        for blk in cfg.BLOCKS.values():
            assert blk["dims"] == (cfg.batch, d >> blk["level"], h >> blk["level"], w >> blk["level"]), blk
            assert len(set(blk["dims"][1:])) == 3                               # pairwise different extents on every level
    # the case lists follow `levels` and `dtypes`
    assert len(a.GATED) == len(a2.GATED) == 18 and len(a.AGG_X) == len(a.AGG_1) == 3 and len(a.UPS) == len(a.POOLS) == 3 and len(a.POOLS_X) == 2
    assert {dt for _, dt in a.GATE_CASES} == {"bf16", "fp16", "fp32"} and {dt for _, dt in a2.GATE_CASES} == {"bf16"}
    assert {dt for _, dt in a.GATE_CASES if a.BLOCKS[_]["level"] < 2} == {"bf16", "fp16"}
    assert {b.BLOCKS[n]["level"] for n in b.GATED + b.AGG} == {1, 2, 3} and {c.BLOCKS[n]["level"] for n in c.GATED + c.AGG} == {0}
    assert len(b.GATED) + len(b.AGG) == 18 and len(c.GATED) + len(c.AGG) == 6 and {dt for _, dt in c.GATE_CASES} == {"bf16"}
    # B: the three up-samplings read levels 3, 2 and 1; the pools read levels 1 and 2, the packed input's pool level 1
    assert [d[1:] for _, _, d in b.UPS] == [(13, 19, 17), (26, 38, 34), (52, 76, 68)]
    assert [d[1:] for _, _, d in b.POOLS] == [(52, 76, 68), (26, 38, 34)] and [d[1:] for _, _, d in b.POOLS_X] == [(52, 76, 68)]
    assert not c.UPS and [d[1:] for _, _, d in c.POOLS] == [(24, 40, 56)] == [d[1:] for _, _, d in c.POOLS_X]
    assert all(e % 8 == 0 and e >> 3 & 1 for e in R.EXT_A + R.EXT_B + R.EXT_C)     # Plan::init's multiples of 8; level 3 odd


def test_cubes_collect_what_they_did(CFGS):
    """An int extent is the cube of it, and without filters every list is whole."""
    import epilogue_layer_cases as E
    cfg = E.Config(2, 32, 1)
    assert cfg.extent == (32, 32, 32) and cfg.key == (2, 32, 1) and cfg.levels is None and cfg.dtypes is None
    assert len(cfg.GATED) == 18 and len(cfg.AGG_X) == 3 and len(cfg.AGG_1) == 3 and len(cfg.UPS) == 3
    assert len(cfg.POOLS) == 3 and len(cfg.POOLS_X) == 2
    assert len(cfg.POOL_FWD_CASES) == 10 and len(cfg.POOL_BWD_CASES) == 12 and len(cfg.UP_CASES) == 6 and len(cfg.UP_BWD_CASES) == 12
    assert [d[1] for _, _, d in cfg.UPS] == [4, 8, 16] and [d[1] for _, _, d in cfg.POOLS_X] == [32, 16]


@pytest.mark.parametrize("key", ["A", "A2", "B", "C"])
def test_facts_are_the_listed_ones(CFGS, key):
    assert R.facts(CFGS[key]) == R.EXPECT[key]


def test_slot_counts_reach_every_branch(CFGS):
    from seunet_amd import _lib
    lib = _lib.load()
    for cfg in CFGS.values():                                   # the restatement is the library's
        for blk in cfg.BLOCKS.values():
            assert R.slots(blk["dims"]) == lib.seunet_epilogue_slots(_lib.Dims(*blk["dims"])) == cfg.SLOTS[blk["level"]], blk
    a, b, c = CFGS["A"], CFGS["B"], CFGS["C"]
    # A: the plain cap (V / 128 > 256 and N p = 256 < 768) twice, V / 128 with a remainder, a handful of records
    assert [a.SLOTS[l] for l in range(4)] == [256, 256, 43, 5]
    assert 354816 // 128 > 256 and 44352 // 128 > 256 and 5544 == 43 * 128 + 40 and 693 == 5 * 128 + 53
    # B: batch 2 stays below the threshold: 2 * 256 = 512 < 768
    assert [b.SLOTS[l] for l in (1, 2, 3)] == [256, 256, 32] and b.batch * 256 < 768 and 13 * 19 * 17 == 32 * 128 + 103
    # C: 5 * 256 = 1280 >= 768 is quantised to one round of 768, which 5 does not divide: 153 per sample, 765 in all
    assert c.SLOTS[0] == 153 and c.batch * 256 >= 768 and 768 // 5 == 153 and 5 * 153 == 765 < 768
    # none of them is the branch the benchmark module runs (a multiple of 768 per launch)
    for cfg in (a, b, c):
        assert all((cfg.batch * cfg.SLOTS[blk["level"]]) % 768 for n, blk in cfg.BLOCKS.items() if n in cfg.GATED + cfg.AGG)


@pytest.mark.parametrize("key", ["A", "A2", "B", "C"])
def test_last_trip_of_pass_a_is_partly_empty(CFGS, key):
    """V mod (slots x 256 / (C / 8)) != 0 for every block the configuration runs: some blocks make one trip less than the
    others, and thread_chain (ceil of the quotient) is the longer count."""
    import epilogue_layer_cases as E
    cfg = CFGS[key]
    seen = set()
    for n in cfg.GATED + cfg.AGG:
        blk = cfg.BLOCKS[n]
        V, per = blk["dims"][1] * blk["dims"][2] * blk["dims"][3], cfg.SLOTS[blk["level"]] * (256 // (blk["C"] // 8))
        assert R.last_trip(blk["dims"], blk["C"]) == V % per != 0, (n, blk)
        assert E.thread_chain(blk["dims"], blk["C"]) == cdiv(V, per) == V // per + 1
        seen.add((blk["level"], blk["C"]))
    want = {"A": {(0, 8), (0, 16), (0, 32), (1, 32), (1, 64), (2, 64), (3, 64)},
            "A2": {(0, 16), (0, 32), (0, 64), (1, 64), (1, 128), (2, 128), (3, 128)},
            "B": {(1, 32), (1, 64), (2, 64), (3, 64)}, "C": {(0, 8), (0, 16), (0, 32)}}[key]
    assert seen == want, sorted(seen)


@pytest.mark.parametrize("key", ["A", "A2", "B"])
def test_up_sampling_marches_on_ragged_segments_and_tiles(CFGS, key):
    cfg = CFGS[key]
    ragged_y = 0
    for c, (d, h, w), ffwd, fbwd, (fseg, flast), (zs, bseg, blast) in R.facts(cfg)["ups"]:
        assert (ffwd, fbwd) == ("march", "march")
        assert len({d, h, w}) == 3
        # backward: several z segments, the last one short
        assert zs == (8 if d >= 32 else 4) and bseg == cdiv(d, zs) > 1 and 0 < blast < zs and (bseg - 1) * zs + blast == d
        # forward: several segments of 16 fine planes, the last one short
        assert fseg == cdiv(2 * d, 16) > 1 and 0 < flast < 16 and (fseg - 1) * 16 + flast == 2 * d
        # x tiles ragged in both directions: 16 coarse columns (backward), 4096 / C fine columns (forward)
        assert w % R.UM_TX != 0 and (2 * w) % (4096 // c) != 0
        ragged_y += h % (128 // c) != 0
    assert len(cfg.UPS) == 3
    # y tiles: TY = 128 / C coarse rows; ragged where TY > 1 meets an odd H (level 3); at 128 channels TY is 1
    assert ragged_y == (0 if key == "A2" else 1)
    assert {128 // c for _, c, _ in cfg.UPS} == ({1, 2} if key == "A2" else {2, 4})


def test_last_segments_are_the_named_ones():
    got = {d: R.segments(d, 8 if d >= 32 else 4)[1] for d in (36, 52, 26, 18, 9, 13)}
    assert got == {36: 4, 52: 4, 26: 2, 18: 2, 9: 1, 13: 1}
    assert all(R.segments(d, 8 if d >= 32 else 4)[1] == (8 if d >= 32 else 4) for d in (16, 32, 64, 20, 40, 80))   # the cubes: full


def test_heads_take_the_named_paths():
    # forward: the row form wherever W % 8 == 0, with a partial y block; the per-voxel form at W = 20
    for H, W in ((R.EXT_A[1], R.EXT_A[2]), R.HEADS_B[0][0].extent[1:]):
        assert W % 8 == 0 and W <= 2048
        nblk, last = R.head_y_blocks(H)
        assert nblk == cdiv(H, 16) and 0 < last < 16, (H, nblk, last)
    assert R.EXT_A[1] == 3 * 16 + 8 and R.head_y_blocks(128) == (8, 16) and R.head_y_blocks(160) == (10, 16)
    assert R.HEADS_B[0][0].extent[2] == 136 > 128                  # a wave passes over the row twice
    assert R.HEADS_B[1][0].extent[2] % 8 == 4 and R.HEADS_B[1][1] == 3
    for shape, nl in R.HEADS_B + [(R.HeadShape(1, R.EXT_A), n) for n in R.HEAD_A]:
        assert all(e % (1 << (nl - 1)) == 0 for e in shape.extent) and len(set(shape.extent)) == 3
    # backward, x pass: the cubes run the fast path (128) and the table walk for want of registers (160: 140 entries)
    assert R.head_x_path(128, 4) == (112, True, [2, 3]) and R.head_x_path(160, 4)[:2] == (140, False)
    # W = 88: few enough entries, but a lane's first entry can be a level-2 row, whose table entry counts up to 11 taps (9 that
    # can carry weight and the zero ones up to the end of its range): refused, the table walk runs
    for nl, nent in ((4, 77), (3, 66)):
        assert R.head_x_path(88, nl)[:2] == (nent, False)
        cnt = list(R.head_x_taps(88, nl)[0]) + list(R.head_x_taps(88, nl)[1])
        assert max(cnt[:44]) <= R.HB_KA < max(cnt[44:64]) == 11
    # W = 136: the fast path, with level-1 entries (64 .. 67) in the second slot next to levels 2 and 3
    assert R.head_x_path(136, 4) == (119, True, [1, 2, 3])
    # (the fast path needs 64 level-1 entries in front: W = 128 .. 146; W = 20 walks the table like W = 88)
    assert R.head_x_path(20, 3)[:2] == (15, False)
    assert [W for W in range(16, 257, 8) if R.head_x_path(W, 4)[1]] == [128, 136, 144]


def test_head_rows_never_exceed_the_table():
    """Every width that 2^l divides gives an output of level l at most 6 / 12 / 23 taps (l = 1 / 2 / 3): HB_K = 24 holds them.
    A width that 8 does not divide can exceed it with 4 levels -- W = 28: 27 taps -- which is why launch_head_bwd refuses it."""
    worst = {1: (0, 0), 2: (0, 0), 3: (0, 0)}
    for W in range(8, 1025, 8):
        for l, t in enumerate(R.head_x_taps(W, 4), 1):
            assert int(t.max()) <= R.HB_K, (W, l, int(t.max()))
            worst[l] = max(worst[l], (int(t.max()), -W))
    assert worst[3] == (23, -24) and worst[1][0] == 6 and worst[2][0] <= 12
    # widths that are multiples of 4 only are valid with 3 levels (20: the 12-tap maximum of level 2) ...
    for W in range(4, 1025, 4):
        t1, t2 = R.head_x_taps(W, 3)
        assert int(t1.max()) <= 6 and int(t2.max()) <= 12, W
    assert int(R.head_x_taps(20, 3)[1].max()) == 12
    # ... and not with 4
    assert int(R.head_x_taps(28, 4)[2].max()) == 27 > R.HB_K and 28 >> 3 == 3
