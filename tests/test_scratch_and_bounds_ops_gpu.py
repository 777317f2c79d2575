"""The per-op wrappers of ``seunet_amd.ops`` and one whole network step over dirty scratch memory, with red zones around every
buffer (tests/guarded_alloc.py).

Each operation runs three times -- scratch and outputs pre-filled with 0x00, with 0xFF and with seeded random bytes, inputs
copied into red-zoned buffers -- and must (a) leave every red zone as it was and (b) give the same bits all three times.
What the values should be is asserted against float64 in tests/test_ops_gpu.py for these very calls; this file adds the fills
and the zones.  Shapes are that file's ragged ones, (2, 6, 9, 40) and (1, 5, 8, 31); the 2x2x2 pooling kernels take even
extents only (the launchers refuse others), so they run at the even neighbours (2, 6, 10, 40) and (1, 4, 8, 30)."""
import pytest
import torch

import guarded_alloc as G
from guarded_alloc import check, guard, guarded_allocations, same_bits, three_fills
from test_launch_cut_host import UP2_FORMS
from test_ops_gpu import MARCH_FWD, STREAM_FWD, gen, rnd

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
SHAPES = [(2, 6, 9, 40), (1, 5, 8, 31)]
EVEN = [(2, 6, 10, 40), (1, 4, 8, 30)]
DT = ["fp32", "bf16", "fp16"]
DT16 = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    from seunet_amd import _lib, ops
    _lib.load()
    return ops


def dev(t):
    """A host tensor on the device, inside a red-zoned buffer of the active context."""
    return guard(t.cuda())


def cl(S, t, dtype):
    """Channels-last device tensor of the storage type (packed by the library from a guarded source), itself guarded."""
    return guard(S.to_cl(dev(t), dtype))


# ---- positive controls: torch ops only ------------------------------------------------------------------------------
def test_control_an_unwritten_buffer_is_flagged_by_the_fills(S):
    with pytest.raises(AssertionError, match="fill 0x00 against fill 0xFF"):
        three_fills(lambda: torch.empty(1000, dtype=torch.int32, device="cuda").sum(), "control")


def test_control_a_write_past_the_payload_is_flagged_by_check(S):
    with guarded_allocations(0xFF, 7) as g:
        t = torch.empty(1000, dtype=torch.float32, device="cuda")
        t.fill_(1.0)
        assert check() == 1
        r = g.records[0]
        past = r.base[r.off + G.RED_ZONE:].view(torch.float32)       # the test's own buffer, seen from the payload's first byte
        assert past.data_ptr() == t.data_ptr()
        past[1000] = 1.0                                              # one element past the payload
        with pytest.raises(AssertionError, match=r"back zone, .* first at payload offset 400\d, last at payload offset 400\d"):
            check()


# ---- layout ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", SHAPES)
def test_layout_pack_and_unpack(S, dtype, shape):
    n, d, h, w = shape

    def op():
        c = S.to_cl(dev(gen(n, 5, d, h, w, seed=1)), dtype)
        wide = S.to_cl(dev(gen(n, 13, d, h, w, seed=2)), dtype, c_pad=24)
        return c, wide, S.from_cl(c), S.from_cl(wide, 13)
    three_fills(op, "layout")


# ---- convolutions -----------------------------------------------------------------------------------------------------
def _srcs(S, x, split, dtype):
    out, o = [], 0
    for c in split:
        out.append(cl(S, x[:, o:o + c], dtype))
        o += c
    return out


TILED = [([8], 2, 8, 1, 3), ([16], 16, 32, 2, 3), ([32, 32], 64, 32, 1, 3), ([32, 8, 16], 56, 32, 1, 1)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", TILED)
def test_conv_forward_with_statistics(S, dtype, impl, shape, case):
    split, cin, cout, dil, k = case
    n, d, h, w = shape

    def op():
        x = rnd(dtype, gen(n, sum(split), d, h, w, seed=2))
        x[:, cin:] = 0
        wt = dev(rnd(dtype, gen(cout, cin, k, k, k, seed=3, scale=(k ** 3 * cin) ** -0.5)))
        (raw,), part, slots = S.conv3d(_srcs(S, x, split, dtype), wt, dev(gen(cout, seed=4, scale=0.1)), dil, impl, cin=cin,
                                       want_stats=True)
        return raw, part, slots, S.stats_finalize(part, slots, d * h * w)
    three_fills(op, "conv tiled / naive fwd")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", STREAM_FWD[:4])
def test_conv_stream_forward_with_statistics(S, shape, case):
    src_c, cin, cout, dil = case
    n, d, h, w = shape

    def op():
        x = rnd("bf16", gen(n, src_c, d, h, w, seed=2))
        x[:, cin:] = 0
        wt = dev(rnd("bf16", gen(cout, cin, 3, 3, 3, seed=3, scale=(27 * cin) ** -0.5)))
        raw, part, slots = S.conv3d_stream(cl(S, x, "bf16"), wt, dev(gen(cout, seed=4, scale=0.1)), dil, want_stats=True)
        return raw, part, slots, S.stats_finalize(part, slots, d * h * w)
    three_fills(op, "conv stream fwd")


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", [MARCH_FWD[2], MARCH_FWD[0], MARCH_FWD[7], MARCH_FWD[9]])
def test_conv_march_forward_with_statistics(S, dtype, shape, case):
    split, cout, dil = case
    n, d, h, w = shape
    cin = sum(split)

    def op():
        x = rnd(dtype, gen(n, cin, d, h, w, seed=2))
        wt = dev(rnd(dtype, gen(cout, cin, 3, 3, 3, seed=3, scale=(27 * cin) ** -0.5)))
        (raw,), part, slots = S.conv3d_march(_srcs(S, x, split, dtype), wt, dev(gen(cout, seed=4, scale=0.1)), dil, want_stats=True)
        return raw, part, slots, S.stats_finalize(part, slots, d * h * w)
    three_fills(op, "conv march fwd")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", [([32, 32], 32, 1, 3), ([16], 32, 2, 3), ([8, 16], 32, 1, 3), ([32, 8, 16], 32, 1, 1)])
def test_conv_data_gradient_tiled(S, dtype, acc, shape, case):
    """Overwrite form: the library's own destinations (torch.empty).  Accumulate form: every destination holds an earlier
    gradient and sits in a guarded buffer."""
    split, cout, dil, k = case
    n, d, h, w = shape
    cin = sum(split)

    def op():
        wt = dev(rnd(dtype, gen(cout, cin, k, k, k, seed=7, scale=(k ** 3 * cin) ** -0.5)))
        dy = cl(S, rnd(dtype, gen(n, cout, d, h, w, seed=8)), dtype)
        if acc:
            dsts = [cl(S, rnd(dtype, gen(n, c, d, h, w, seed=9 + i)), dtype) for i, c in enumerate(split)]
            out, _, _ = S.conv3d([dy], wt, None, dil, 0, transpose_flip=True, dsts=dsts, accumulate=[1] * len(split))
        else:
            out, _, _ = S.conv3d([dy], wt, None, dil, 0, transpose_flip=True, dst_channels=list(split))
        return out
    three_fills(op, "conv tiled dgrad")


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", [(16, 8, 8, 1), (32, 16, 16, 2), (16, 32, 32, 1), (16, 8, 16, 1)])
def test_conv_data_gradient_stream(S, acc, shape, case):
    dyc, dxc, dst_c, dil = case
    n, d, h, w = shape

    def op():
        wt = dev(rnd("bf16", gen(dyc, dxc, 3, 3, 3, seed=5, scale=(27 * dxc) ** -0.5)))
        dy = cl(S, rnd("bf16", gen(n, dyc, d, h, w, seed=6)), "bf16")
        dst = cl(S, rnd("bf16", gen(n, dst_c, d, h, w, seed=7)), "bf16") if acc else None
        got, _, _ = S.conv3d_stream(dy, wt, None, dil, transpose_flip=True, dst=dst, dst_channels=dst_c, accumulate=acc)
        return got
    three_fills(op, "conv stream dgrad")


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", [(32, [32, 32], 1), (64, [32], 2), (32, [32], 1), (64, [64, 64], 1)])
def test_conv_data_gradient_march(S, dtype, acc, shape, case):
    dyc, split, dil = case
    n, d, h, w = shape
    dxc = sum(split)

    def op():
        wt = dev(rnd(dtype, gen(dyc, dxc, 3, 3, 3, seed=5, scale=(27 * dxc) ** -0.5)))
        dy = cl(S, rnd(dtype, gen(n, dyc, d, h, w, seed=6)), dtype)
        if acc:
            dsts = [cl(S, rnd(dtype, gen(n, c, d, h, w, seed=7 + i)), dtype) for i, c in enumerate(split)]
            got, _, _ = S.conv3d_march([dy], wt, None, dil, transpose_flip=True, dsts=dsts, accumulate=[1] * len(split))
        else:
            got, _, _ = S.conv3d_march([dy], wt, None, dil, transpose_flip=True, dst_channels=list(split))
        return got
    three_fills(op, "conv march dgrad")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", [([8], 2, 8, 1, 27), ([16], 16, 32, 2, 27), ([32, 32], 64, 32, 1, 27), ([32, 8, 16], 56, 32, 1, 1),
                                  ([8], 2, 32, 1, 1)])
def test_conv_weight_gradient_tiled(S, dtype, impl, shape, case):
    split, cin, cout, dil, taps = case
    n, d, h, w = shape

    def op():
        x = rnd(dtype, gen(n, sum(split), d, h, w, seed=10))
        x[:, cin:] = 0
        dy = cl(S, rnd(dtype, gen(n, cout, d, h, w, seed=11)), dtype)
        return S.conv3d_wgrad(_srcs(S, x, split, dtype), dy, cin, cout, taps, dil, impl)
    three_fills(op, "wgrad tiled / naive")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", [(8, 2, 8, 1), (8, 8, 16, 1), (16, 16, 32, 2), (32, 32, 16, 1)])
def test_conv_weight_gradient_stream(S, shape, case):
    x_c, cin, cout, dil = case
    n, d, h, w = shape

    def op():
        x = rnd("bf16", gen(n, x_c, d, h, w, seed=8))
        x[:, cin:] = 0
        return S.conv3d_wgrad_stream(cl(S, x, "bf16"), cl(S, rnd("bf16", gen(n, cout, d, h, w, seed=9)), "bf16"), cin, cout, dil)
    three_fills(op, "wgrad stream")


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", [([32], 32, 1, 27), ([32, 32], 32, 1, 27), ([32], 64, 2, 27), ([64], 64, 2, 27),
                                  ([32, 32], 32, 1, 1), ([64, 32, 32], 64, 1, 1), ([64, 64, 64], 128, 1, 1)])
def test_conv_weight_gradient_march_and_1x1(S, dtype, shape, case):
    """csrc/wgrad_march.hip (27 taps) and csrc/wgrad_1x1.hip (1 tap), forced as tests/test_ops_gpu.py forces them."""
    split, cout, dil, taps = case
    n, d, h, w = shape
    cin = sum(split)

    def op():
        x = rnd(dtype, gen(n, cin, d, h, w, seed=12))
        dy = cl(S, rnd(dtype, gen(n, cout, d, h, w, seed=13)), dtype)
        return S.conv3d_wgrad(_srcs(S, x, split, dtype), dy, cin, cout, taps, dil, S._lib.CONV_MARCH)
    three_fills(op, "wgrad march / 1x1")


# ---- statistics and epilogues ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", [8, 32, 128])
def test_channel_stats_and_finalize(S, dtype, shape, c):
    n, d, h, w = shape

    def op():
        part, slots = S.channel_stats(cl(S, rnd(dtype, gen(n, c, d, h, w, seed=12) * 2 + 0.3), dtype))
        return part, slots, S.stats_finalize(part, slots, d * h * w), S.stats_finalize(part, slots, d * h * w, 0.0, 1)
    three_fills(op, "statistics")


def _stats(S, raw_cl, vox):
    part, slots = S.channel_stats(raw_cl)
    return S.stats_finalize(part, slots, vox)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c,gates", [(8, 1), (32, 2), (128, 2)])
@pytest.mark.parametrize("fused", [False, True])
def test_gate_epilogue_with_side_output(S, dtype, shape, c, gates, fused):
    n, d, h, w = shape

    def op():
        raw = cl(S, rnd(dtype, gen(n, c, d, h, w, seed=12) * 2 + 0.3), dtype)
        w_se, w_side, b_side = dev(gen(1, c, 1, 1, 1, seed=13, scale=0.5)), dev(gen(2, c, 1, 1, 1, seed=15, scale=0.5)), dev(gen(2, seed=16, scale=0.1))
        w_se2 = dev(gen(1, c, 1, 1, 1, seed=14, scale=0.5)) if gates == 2 else None
        mean, rstd = _stats(S, raw, d * h * w)
        e, side = S.gate_epilogue_fwd(raw, mean, rstd, w_se, w_se2, w_side, b_side)
        out = S.gate_epilogue_bwd(raw, mean, rstd, w_se, w_se2, w_side, b_side, g_e=cl(S, rnd(dtype, gen(n, c, d, h, w, seed=17)), dtype),
                                  g_side=dev(gen(n, d, h, w, 2, seed=18)), fused_finalize=fused)
        return e, side, out
    three_fills(op, "gate epilogue")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", SHAPES)
def test_gate_epilogue_with_level_map(S, dtype, shape):
    n, d, h, w = shape
    c = 16

    def op():
        raw = cl(S, rnd(dtype, gen(n, c, d, h, w, seed=19)), dtype)
        w_se, w_side, b_side = dev(gen(1, c, 1, 1, 1, seed=20)), dev(gen(2, c, 1, 1, 1, seed=21)), dev(gen(2, seed=22))
        head_w = dev(gen(2, seed=23))
        drop = dev(torch.tensor([[0.0, 1.3, 9, 9], [0.7, 0.7, 9, 9]])[:n].contiguous())
        mean, rstd = _stats(S, raw, d * h * w)
        lvl = dev(torch.full((n, d, h, w), 5.0))
        e, _ = S.gate_epilogue_fwd(raw, mean, rstd, w_se, None, w_side, b_side, level_map=lvl, level_accumulate=1, head_w=head_w,
                                   drop=drop, drop_stride=4, want_side=False)
        out = S.gate_epilogue_bwd(raw, mean, rstd, w_se, None, w_side, b_side, g_level=dev(gen(n, d, h, w, seed=24)), head_w=head_w,
                                  drop=drop, drop_stride=4)
        return e, lvl, out
    three_fills(op, "gate epilogue")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("two", [False, True])
def test_cat_epilogue_plain(S, dtype, shape, two):
    n, d, h, w = shape
    c = 32

    def op():
        a = cl(S, rnd(dtype, gen(n, c, d, h, w, seed=25) + 0.2), dtype)
        sa = (a,) + _stats(S, a, d * h * w)
        sb = (None, None, None)
        if two:
            b = cl(S, rnd(dtype, gen(n, c, d, h, w, seed=26) * 3), dtype)
            sb = (b,) + _stats(S, b, d * h * w)
        return S.cat_epilogue_fwd(*sa, *sb), S.cat_epilogue_bwd(cl(S, rnd(dtype, gen(n, c, d, h, w, seed=27)), dtype), *sa, *sb)
    three_fills(op, "cat epilogue")


def _x_in(S, x, dtype):
    n, inch, d, h, w = x.shape
    xin = torch.zeros((n, d, h, w, 8), dtype=S._tdtype(S._lib.dtype_code(dtype)), device="cuda")
    xin[..., :inch] = x.permute(0, 2, 3, 4, 1).cuda().to(xin.dtype)
    return xin


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("inch,c", [(2, 32), (1, 64), (2, 128)])
def test_cat_epilogue_with_recomputed_x_branch(S, dtype, shape, inch, c):
    n, d, h, w = shape

    def op():
        xin = _x_in(S, rnd(dtype, gen(n, inch, d, h, w, seed=31) + 0.3), dtype)
        raw = cl(S, rnd(dtype, gen(n, c, d, h, w, seed=33) + 0.2), dtype)
        mean, rstd = _stats(S, raw, d * h * w)
        return S.cat_epilogue_x(cl(S, rnd(dtype, gen(n, c, d, h, w, seed=34)), dtype), raw, mean, rstd, xin,
                                dev(gen(c, inch, 1, 1, 1, seed=32) * 0.7), inch)
    three_fills(op, "cat epilogue")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", EVEN)
@pytest.mark.parametrize("c", [32, 128])
def test_cat_epilogue_pooled(S, dtype, shape, c):
    n, d, h, w = shape

    def op():
        xin = _x_in(S, rnd(dtype, gen(n, 2, d, h, w, seed=31) + 0.3), dtype)
        raw = cl(S, rnd(dtype, gen(n, c, d, h, w, seed=33) + 0.2), dtype)
        w2 = dev(gen(c, 2, 1, 1, 1, seed=32) * 0.7)
        mean, rstd = _stats(S, raw, d * h * w)
        mean2, rstd2, mom = S.xbranch_stats(xin, w2, 2)
        out, pooled, words = S.cat_epilogue_fwd_x_pool(raw, mean, rstd, xin, w2, 2, mean2, rstd2)
        res = S.cat_epilogue_bwd_x(cl(S, rnd(dtype, gen(n, c, d, h, w, seed=34)), dtype), raw, mean, rstd, xin, w2, 2, mean2, rstd2, mom,
                                   pool_argmax=words, pool_g=cl(S, rnd(dtype, gen(n, c, d // 2, h // 2, w // 2, seed=35)), dtype))
        return out, pooled, words, res
    three_fills(op, "cat epilogue")


# ---- pooling, up-sampling, heads --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", EVEN)
@pytest.mark.parametrize("c", [8, 24])
def test_maxpool_forward_backward(S, dtype, shape, c):
    n, d, h, w = shape

    def op():
        g0 = torch.Generator().manual_seed(50 + c)
        x = cl(S, torch.randint(0, 3, (n, c, d, h, w), generator=g0).float(), dtype)            # full of ties
        g = cl(S, rnd(dtype, gen(n, c, d // 2, h // 2, w // 2, seed=51)), dtype)
        prev = cl(S, rnd(dtype, gen(n, c, d, h, w, seed=30)), dtype)
        return S.maxpool_fwd(x), S.maxpool_bwd(x, g), S.maxpool_bwd(x, g, prev)
    three_fills(op, "maxpool")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [(n, 16, d, h, w) for n, d, h, w in SHAPES] + list(UP2_FORMS))
def test_upsample2_forward_backward(S, dtype, shape):
    """The two ragged shapes at 16 channels, and every shape of UP2_FORMS (each is the smallest that takes its combination of
    gather / tiled / marching forms; the smallest entry alone would leave the marching kernels out)."""
    n, c, d, h, w = shape

    def op():
        y = cl(S, rnd(dtype, gen(n, c, d, h, w, seed=41)), dtype)
        gu = cl(S, rnd(dtype, gen(n, c, 2 * d, 2 * h, 2 * w, seed=42)), dtype)
        init = cl(S, rnd(dtype, gen(n, c, d, h, w, seed=43)), dtype)
        return S.upsample2_fwd(y), S.upsample2_bwd(gu), S.upsample2_bwd(gu, g_in=init)
    three_fills(op, "upsample2")


@pytest.mark.parametrize("case", [(2, 16, 8, 24, 4), (1, 8, 8, 136, 4), (1, 8, 4, 20, 3)])
def test_heads_forward_backward(S, case):
    n, d, h, w, nl = case

    def op():
        maps = [dev(gen(n, d >> l, h >> l, w >> l, seed=33 + l)) for l in range(nl)]
        return S.head_fwd(maps, dev(gen(1, seed=40))), S.head_bwd(dev(gen(n, 1, d, h, w, seed=41)), nl)
    three_fills(op, "heads")


def test_side_upsample(S):
    def op():
        side = dev(gen(2, 3, 4, 5, 2, seed=42))
        return S.side_upsample(side, 4), S.side_upsample(side, 2), S.side_upsample(side, 1)
    three_fills(op, "side_upsample")


# ---- the whole network: forward, stage-1 loss, backward -------------------------------------------------------------------
@pytest.mark.parametrize("batch,size,dtype,input_grad", [(1, (40, 48, 56), "fp32", False), (1, (40, 48, 56), "bf16", False),
                                                         (1, (40, 48, 56), "fp16", False), (2, (32, 32, 32), "bf16", True)])
def test_one_network_step(S, batch, size, dtype, input_grad):
    """Arena, logits, gradient bucket and input gradient all come from torch.empty; input, label and every parameter are
    copied into guarded buffers."""
    import seunet_amd as A
    import seunet_oracle as orc
    b = orc.synthetic_batch(batch, size, 2, seed=13)
    sd = orc.deterministic_state_dict(2, 1, 1, seed=0)

    def op():
        m = A.SE_UNet(in_channel=2, n_classes=1, act_dtype=dtype, input_grad=input_grad)
        m.load_state_dict(sd)
        m = m.cuda().eval()
        for p in m.parameters():
            p.data = guard(p.data)
        x, lab = dev(b["image"]), dev(b["label"])
        if input_grad:
            x.requires_grad_(True)
        e, d = m(x)
        loss = A.fused_stage_loss(1, e, d, lab)
        loss.backward()
        grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        assert grads and bool(torch.isfinite(loss))
        return loss.detach(), e.detach(), d.detach(), grads, (x.grad if input_grad else None)
    res = three_fills(op, "network step")
    assert (res[4] is not None) == input_grad


def test_the_allocation_functions_are_restored(S):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
    print("\nguarded allocations verified, by family (operations, allocations):")
    for fam, (ops_n, allocs) in sorted(G.VERIFIED.items()):
        print(f"  {fam}: {ops_n} operations, {allocs} allocations")
