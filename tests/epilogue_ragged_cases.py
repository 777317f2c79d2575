"""The non-cubic configurations of the ragged epilogue / resampling / head tests, and what each is there to reach.  Shared by
tests/test_epilogue_layers_ragged_gpu.py (which runs the case functions of tests/epilogue_layer_cases.py on them, under the
derived bounds of tests/epilogue_ref.py) and tests/test_epilogue_ragged_host.py (which proves, without a GPU, that the extents
meet the slot counts, z segments, tiles and head paths each case is named for).  The extents are those of
tests/conv_ragged_cases.py, so the same volumes get both halves of a training step tested.

The cubes of the other epilogue modules (4 x 2 x 128^3 at width 1, 2 x 2 x 160^3 at width 2) cannot tell H's stride, scale or extent
from W's or D's, run one or two branches of ``epi_partials`` each, and fill every z segment of the up-sampling kernels.  Here:

  A   1 x 2 x (72, 56, 88), width 1, bf16 and fp16 (fp32 storage on levels 2 and 3), all 24 blocks, every case list, the
        block-by-block forward in bf16 and fp16, both heads' passes with 4 and 3 levels
        slots 256 / 256 / 43 / 5: the plain cap at batch 1 (N p < 768) twice, V / 128 with a remainder (5 544 = 43 * 128 + 40),
        and five records for 693 voxels; the last grid-stride trip of pass A is partly empty for every channel count
        level 3 is (9, 7, 11): every extent odd; up-sampling from D = 9 / 18 / 36 leaves the last z segment of the backward
        march with 1 / 2 / 4 planes (of 4 / 4 / 8) and the forward's last segment with 2 / 4 / 8 fine planes of 16
        heads at W = 88: the row form with H = 56 = 3 * 16 + 8 (a partial y block); the backward's x pass has 77 table entries
        but a lane's first entry can be a level-2 row of up to 11 taps (> HB_KA = 8), so the register fast path is refused and
        the table walk runs
  A2  the same extents at width 2, bf16: gate, aggregation and up-sampling cases.  128-channel lanes (16 lanes per voxel, one
        coarse row per block in the backward march) at ragged extents
  B   2 x 2 x (104, 152, 136), width 1, bf16 and fp16, levels 1 to 3 (level 0 adds nothing over A and is the expensive part)
        up-sampling from (13, 19, 17), (26, 38, 34), (52, 76, 68): 8-plane segments with a half-empty last one (52 = 6 * 8 + 4),
        every extent odd on level 3; slots 256 / 256 / 32 at batch 2, still below the 768 threshold
  B heads  1 x (40, 24, 136) with 4 levels: W = 136 > 128, so a wave passes over the row twice in the forward, and the backward's
        register fast path runs (119 entries) with level-1 entries in a lane's second slot.  1 x (16, 40, 20) with 3 levels:
        W % 8 == 4, the per-voxel forward
  C   5 x 2 x (24, 40, 56), width 1, bf16, level 0, gate and aggregation cases: 5 * 256 records exceed 768, and the quantised
        count 768 / 5 = 153 is one the batch does not divide (N p = 765)

No extent had to move from the ones first proposed: the facts below hold as listed (EXPECT, asserted at import by the GPU module
and tested by the host module)."""
import ctypes as C
import math
from collections import namedtuple

import epilogue_layer_cases as E
from conv_ragged_cases import EXT_A, EXT_B  # noqa: F401

EXT_C = (24, 40, 56)
HeadShape = namedtuple("HeadShape", "batch extent")           # what head_forward / head_backward read of a configuration
HEAD_A = [4, 3]                                                # levels of the two heads, on A's extents
HEADS_B = [(HeadShape(1, (40, 24, 136)), 4), (HeadShape(1, (16, 40, 20)), 3)]
# extents with one axis that 2^3 does not divide (28 = 3 * 8 + 4): refused with 4 levels
HEADS_REFUSED = [(8, 8, 28), (8, 28, 8), (28, 8, 8)]

_made = {}


def configs():
    """{"A": Config, "A2": ..., "B": ..., "C": ...}, built once per process (the plans come from the library)."""
    if not _made:
        _made["A"] = E.Config(1, EXT_A, 1)
        _made["A2"] = E.Config(1, EXT_A, 2, dtypes=("bf16",))
        _made["B"] = E.Config(2, EXT_B, 1, levels=(1, 2, 3))
        _made["C"] = E.Config(5, EXT_C, 1, levels=(0,), dtypes=("bf16",))
    return _made


# ---- the cuts, restated from the sources (csrc/epilogue.hip, csrc/resample.hip, csrc/heads.hip) ------------------------------------
def slots(dims):
    """epi_partials: V / 128 records per sample, at least 1, at most 256; once N records reach 768 = 3 x 256 workgroups, the
    launch's count is rounded down to a multiple of 768 and divided by the batch."""
    n, d, h, w = dims
    p = min(max(d * h * w // 128, 1), 256)
    if n * p >= 768:
        q = (n * p // 768) * 768 // n
        if q >= 1:
            p = q
    return p


def last_trip(dims, c):
    """Voxels the last grid-stride trip of pass A holds, over all blocks of a sample: V mod (slots x voxels per block and trip);
    0 = every trip is full."""
    n, d, h, w = dims
    return (d * h * w) % (slots(dims) * (256 // (c // 8)))


def segments(planes, per):
    """(segments, planes of the last one) of `planes` cut into runs of `per`."""
    nseg = -(-planes // per)
    return nseg, planes - (nseg - 1) * per


def up_bwd_cut(c, dims):
    """upsample2_bwd_cut, march form: (coarse rows per block TY, coarse planes per segment ZS)."""
    return 128 // c, 8 if dims[1] >= 32 else 4


UFM_ZSF, UM_TX = 16, 16          # fine planes per z segment of the forward march; coarse columns per block of the backward march
FORMS = ("gather", "tiled", "march")


def up_form(dtype, c, dims, backward):
    from seunet_amd import _lib
    f = _lib.load().seunet_debug_upsample2_form              # diagnostic export, not in the public header
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int, _lib.Dims, C.c_int]
    return FORMS[f(_lib.dtype_code(dtype), c, _lib.Dims(*dims), int(backward))]


def facts(cfg):
    """What a configuration's case lists reach: the slot count of every level it runs, and per up-sampling case (channels, coarse
    extents, forward form, backward form, (segments, fine planes of the last) of the forward, (ZS, segments, coarse planes of the
    last) of the backward)."""
    lv = sorted({cfg.BLOCKS[n]["level"] for n in cfg.GATED + cfg.AGG})
    ups = []
    for _, c, dims in cfg.UPS:
        forms = {(up_form(dt, c, dims, False), up_form(dt, c, dims, True)) for dt in ("bf16", "fp16")}
        assert len(forms) == 1, forms                           # both 16-bit storage types take the same route
        _, zs = up_bwd_cut(c, dims)
        ups.append((c, tuple(dims[1:])) + forms.pop() + (segments(2 * dims[1], UFM_ZSF), (zs,) + segments(dims[1], zs)))
    return {"slots": [cfg.SLOTS[l] for l in lv], "ups": ups}


EXPECT = {
    "A": {"slots": [256, 256, 43, 5],
          "ups": [(64, (9, 7, 11), "march", "march", (2, 2), (4, 3, 1)), (64, (18, 14, 22), "march", "march", (3, 4), (4, 5, 2)),
                  (32, (36, 28, 44), "march", "march", (5, 8), (8, 5, 4))]},
    "A2": {"slots": [256, 256, 43, 5],
           "ups": [(128, (9, 7, 11), "march", "march", (2, 2), (4, 3, 1)), (128, (18, 14, 22), "march", "march", (3, 4), (4, 5, 2)),
                   (64, (36, 28, 44), "march", "march", (5, 8), (8, 5, 4))]},
    "B": {"slots": [256, 256, 32],
          "ups": [(64, (13, 19, 17), "march", "march", (2, 10), (4, 4, 1)), (64, (26, 38, 34), "march", "march", (4, 4), (4, 7, 2)),
                  (32, (52, 76, 68), "march", "march", (7, 8), (8, 7, 4))]},
    "C": {"slots": [153], "ups": []},
}


# ---- the x pass of the heads' backward (head_bwd_x_multi_kernel), in numpy float32 ---------------------------------------------------
HB_K, HB_KA = 24, 8


def head_x_taps(W, nlevels):
    """Per coarse level l = 1 .. nlevels - 1 the tap count of every output of that level along x: ac_scale / ac_range /
    ac_weight of csrc/trilinear.h in float32, counted as the kernel's table does -- from the first non-zero weight of the range to
    its end."""
    import numpy as np
    f = np.float32
    out = []
    o = np.arange(W)
    for l in range(1, nlevels):
        Wl = W >> l
        i = np.arange(Wl)[:, None]
        rs = f(Wl - 1) / f(W - 1) if W > 1 else f(0)
        if rs <= 0:
            lo, hi = np.zeros((Wl, 1), dtype=np.int64), np.full((Wl, 1), W - 1)
        else:
            lo = np.floor((i - 1).astype(f) / rs).astype(np.int64) - 1
            hi = np.ceil((i + 1).astype(f) / rs).astype(np.int64) + 1
        lo, hi = np.maximum(lo, 0), np.minimum(hi, W - 1)
        src = rs * o.astype(f)                                   # (float32 product)
        i0 = np.minimum(src.astype(np.int64), Wl - 1)
        i1 = i0 + (i0 < Wl - 1)
        lam = src - i0.astype(f)
        w = np.where(i0[None, :] == i, f(1) - lam[None, :], f(0)) + np.where(i1[None, :] == i, lam[None, :], f(0))
        in_range = (o[None, :] >= lo) & (o[None, :] <= hi)
        started = np.maximum.accumulate(in_range & (w != 0), axis=1)
        out.append((started & in_range).sum(1))
    return out


def head_x_path(W, nlevels):
    """(table entries, whether the register fast path runs, levels of the entries a lane's second slot holds): the fast path asks
    for at most 128 entries, at most HB_KA taps in every lane's first entry (entry = lane) and HB_K in its second (lane + 64)."""
    import numpy as np
    taps = head_x_taps(W, nlevels)
    cnt = np.concatenate(taps)
    level = np.concatenate([np.full(len(t), l + 1) for l, t in enumerate(taps)])
    nent = len(cnt)
    fast = nent <= 128 and bool((cnt[:64] <= HB_KA).all()) and bool((cnt[64:128] <= HB_K).all())
    return nent, fast, sorted(set(level[64:128].tolist()))


def head_y_blocks(H):
    """(y blocks per plane of head_fwd_rows_kernel -- 4 waves x 4 rows --, rows of the last block)."""
    return segments(H, 16)


assert math.prod(EXT_A) == 354816 and math.prod(EXT_C) == 53760
