"""The non-cubic configurations of the ragged per-layer convolution tests, and what each is there to reach.  Shared by
tests/test_conv_layers_ragged_gpu.py (which runs every routed pass of them bitwise, with the machinery of
tests/conv_layer_cases.py) and tests/test_conv_ragged_host.py (which proves, without a GPU, that the plans route the layers to the
kernels named here and that the extents leave the tiles ragged in the way each case is named for).

``Plan::init`` takes any extents that are multiples of 8 per axis, independently; the cubes of the other layer modules (128^3,
160^3) are multiples of every tile of the kernel family -- the 32-voxel x block of all five kernels, the 8 x 32 streaming patches,
the 4- and 8-row marching patches, the 4 x 32 weight-gradient patches, the tiled 2 x 4 x 32 -- have equal axes and an even plane
count per dilation-2 parity class.  These do not:

  A   1 x 2 x (72, 56, 88), width 1, bf16 and fp16, all 24 layers
        level 0 (72, 56, 88), 354 816 voxels, W = 2 * 32 + 24: ec1 / ec2 / ec3 / dc6 stream, dc5 marches in all three passes
        level 1 (36, 28, 44), 44 352 voxels, between 32^3 and 48^3: only the dilation-2 layers ec5 / ec6 march (x tail 12,
                H = 3 * 8 + 4); ec4 / dc4 / dc3 are tiled
        level 2 (18, 14, 22): forward and data gradient tiled; the weight gradient of ec8 / ec9 marches on W = 22 < 32, one
                partial x block (wgrad_kernel sends every dilation-2 layer there whatever W is)
        level 3 (9, 7, 11): tiled, every extent odd
  A2  the same extents at width 2, bf16: ec3 and dc6 leave the streaming kernel for the marching one; dc5's forward is tiled
        while its gradients march; dc1 / dc3 take the 256-input-channel marching weight gradient on ragged rows
  B   2 x 2 x (104, 152, 136), width 1, bf16 and fp16, levels 1 to 3 (level 0 adds nothing over A and is the expensive part)
        level 1 (52, 76, 68), 268 736 voxels >= 48^3: ec4 / ec5 / ec6 / dc4 march in all passes, dc3 in its two gradients; x
                tail 4, H = 9 * 8 + 4; batch 2 moves march_zsteps; ec63 sees 2 * 268 736 = 537 472 >= 500 000 voxels and takes the
                whole-GEMM Wgrad1x1 on a per-sample voxel count that is no multiple of 128
        level 2 (26, 38, 34), 33 592 voxels >= 32^3, W = 34: ec8 / ec9 march in all three passes; x tail 2, H = 9 * 4 + 2, 13
                planes per parity class
        level 3 (13, 19, 17): tiled, every extent odd
  C   3 x 2 x (104, 152, 136), width 1, bf16 and fp16, the weight gradient of ec63 alone (added to the proposed set).  Wgrad1x1
        chunks the FLAT (sample, voxel) index, and extents that are multiples of 8 make a level-1 sample a multiple of 64
        voxels, so at batch 2 the flat count is always a multiple of the 128-voxel chunk (B: 537 472 = 4 199 * 128): in B a chunk
        straddles the two samples, but the last chunk is full.  With three samples of 268 736 = 2 099 * 128 + 64 voxels the flat
        count is 806 208 = 6 298 * 128 + 64: the last chunk is half empty, the case the chunk tail of wgrad_1x1.hip is there for.
        Sums are at most 806 208 < 2^24.

No extent had to move from the ones first proposed: the plans route as listed (ROUTING below, asserted at import by the GPU
module and tested by the host module).

Exactness (tests/conv_layer_cases.py): forward and data-gradient sums stay <= 27 * 256 * 9 + 3 = 62 211; weight-gradient sums are
at most N * voxels <= 537 472 (C: 806 208) < 2^24."""
import conv_layer_cases as L

EXT_A, EXT_B = (72, 56, 88), (104, 152, 136)

T3, M3, S3 = ("Tiled",) * 3, ("March",) * 3, ("Stream",) * 3
# (fwd, dgrad, wgrad) of every layer, the same in bf16 and fp16: a later re-route shows up as an edit here
_COARSE = {n: T3 for n in ("ec7", "ec93", "ec10", "ec11", "ec12", "ec123", "dc1", "dc2", "dc22")}
_POINTWISE_FINE = {n: T3 for n in ("ec33", "ec63", "dc42")}
ROUTING_A = dict(_COARSE, **_POINTWISE_FINE, **{
    "ec1": ("Stream", None, "Stream"), "ec2": S3, "ec3": S3, "dc6": S3,               # (72, 56, 88), 8 / 16 / 32 channels
    "dc5": M3,                                                                       # (72, 56, 88), [32, 32] -> 32
    "ec4": T3, "ec5": M3, "ec6": M3, "dc4": T3, "dc3": T3,                            # (36, 28, 44): dilation 2 marches, dilation 1 does not
    "ec8": ("Tiled", "Tiled", "March"), "ec9": ("Tiled", "Tiled", "March"),           # (18, 14, 22): W < 32
})
ROUTING_A2 = dict(ROUTING_A, **{
    "ec3": M3, "dc6": M3,                                                             # 32 -> 64 dilation 2 / 64 -> 32
    "dc5": ("Tiled", "March", "March"),                                               # [64, 64] -> 64
    "ec6": ("March", "Tiled", "March"),                                               # 64 -> 128: the data gradient has 128 sources
    "dc3": ("Tiled", "Tiled", "March"), "dc1": ("Tiled", "Tiled", "March"),           # 256 input channels below 48^3
})
ROUTING_B = dict(ROUTING_A, **{
    "ec4": M3, "dc4": M3, "dc3": ("Tiled", "March", "March"),                         # (52, 76, 68) >= 48^3
    "ec63": ("Tiled", "Tiled", "Wgrad1x1"),                                           # 2 * 268 736 >= 500 000 voxels
    "ec8": M3, "ec9": M3,                                                             # (26, 38, 34) >= 32^3, W >= 32
})

_made = {}


def configs():
    """{"A": (Config, routing), "A2": ..., "B": ..., "C": ...}, built once per process (the plans come from the library)."""
    if not _made:
        _made["A"] = (L.Config(1, EXT_A, 1), ROUTING_A)
        _made["A2"] = (L.Config(1, EXT_A, 2, dtypes=("bf16",)), ROUTING_A2)
        _made["B"] = (L.Config(2, EXT_B, 1, levels=(1, 2, 3)), ROUTING_B)
        _made["C"] = (L.Config(3, EXT_B, 1, levels=(1,)), ROUTING_B)
    return _made


def misrouted(cfg, routing):
    """[(layer, storage type, the plan's (fwd, dgrad, wgrad), the expected one)] of every layer the plan routes elsewhere."""
    return [(n, dt, cfg.passes(n, dt), routing.get(n)) for dt in cfg.dtypes for n in cfg.PLANS[dt] if cfg.passes(n, dt) != routing.get(n)]
