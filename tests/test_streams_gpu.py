"""Every operation family on a side stream, behind a producer that is still busy when the operation is called
(tests/side_stream.py).

The rest of the suite runs on the default stream, where work issued on stream 0 instead of the caller's stream, or a host read
that waits for the wrong stream, cannot be seen.  Here each family's inputs hold poison (another valid input) until a delayed
copy on a fresh non-blocking stream delivers the real data, and the operation is called under that stream while the delay is
pending.  Results must equal, bit for bit, the same call made beforehand on the default stream with the real inputs (which is
also the warm-up that keeps one-time kernel setup out of the delayed call) and, where the suite has an independent statement
that is cheap at these shapes (skeleton, mesh, morphometry, components and DTI oracles, scipy, the recorded fixtures, the AdamW
oracle), that statement.  What the values should be at large is asserted elsewhere for these very calls; this file adds the
stream, as tests/test_scratch_and_bounds_ops_gpu.py adds the fills.

Operations documented as not synchronising the host (conv / epilogue / loss wrappers, per_sample_loss, OnlineHardPool.add,
AdamW.step, predict_logits, SE_UNet forward and backward) must also return while the delay is still pending.

Delay: 50 ms (DELAY_MS of tests/side_stream.py), calibrated once per process from one timed ``_sleep``; on an MI355X a test then
takes the 50 ms it asks for (0.40 s each when the delay was set to 400 ms).  The longest host time from the delay's start to
the return of a call that must not wait was 5.9 ms (the second of the two interleaved network steps; a single network step:
3.0-4.1 ms; every per-op family under 1.2 ms), so both ``gate.query()`` asserts hold with room to spare.  One figure did not
fit: a network step's FIRST run on a stream grows torch's per-stream allocator pool, and at 40 x 48 x 56 those hipMalloc calls
took 145 ms of host time; the two-stream test therefore runs each step once undelayed on its stream before the delayed run.
The last test prints the figures of the run.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import side_stream as SS
from guarded_alloc import same_bits
from side_stream import Delayed, run_behind_delay, to_device
from test_launch_cut_host import UP2_FORMS
from test_ops_gpu import MARCH_FWD, STREAM_FWD, gen

import skeleton_oracle as so

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SHAPES = [(2, 6, 9, 40), (1, 5, 8, 31)]
EVEN = (2, 6, 10, 40)
POISON = 100                                   # seed offset of the poison inputs
WINDOW_CASES = {(48, 32, 64): (3, 0), (64, 32, 64): (4, 1)}        # volume -> (full batches, windows in the ragged last one) at batch 2


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


@pytest.fixture(scope="module")
def S(A):
    from seunet_amd import ops
    return ops


def serial(real, op):
    """``op`` on the default stream with the real inputs (fresh device copies): the expected bits, and the warm-up."""
    out = op(*[to_device(v) for v in real])
    torch.cuda.synchronize()
    return out


def both(real, poison, op, label, no_host_sync=False):
    """The default-stream result and the side-stream result of ``op``, after asserting that they are the same bits."""
    want = serial(real, op)
    got = run_behind_delay(lambda: real, lambda: poison, op, no_host_sync, label=label)
    same_bits(got, want, f"{label}: side stream against default stream")
    return got, want


def other(v):
    """Poison for a volume: the same volume turned round (still a valid mask, label map or scan of that shape)."""
    p = np.ascontiguousarray(v[::-1, ::-1, ::-1])
    return p if not np.array_equal(p, v) else np.ascontiguousarray(np.roll(v, 1, axis=-1))


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- positive controls: torch ops only ------------------------------------------------------------------------------
def test_control_work_on_the_default_stream_sees_the_poison(A):
    real, poison = [gen(1000, seed=1)], [gen(1000, seed=1 + POISON)]

    def op(x):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return x.clone()
    got = run_behind_delay(lambda: real, lambda: poison, op, no_host_sync=True, label="control")
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), poison[0]) and not torch.equal(got.cpu(), real[0])
    right = run_behind_delay(lambda: real, lambda: poison, lambda x: x.clone(), no_host_sync=True, label="control")
    assert torch.equal(right.cpu(), real[0])


def test_control_a_delay_of_zero_cycles_trips_the_gate(A):
    """Without a delay the gate has fired by the time the operation (here: one that waits for its stream) has returned, if not
    before it is called."""
    real, poison = [gen(1000, seed=2)], [gen(1000, seed=2 + POISON)]

    def op(x):
        torch.cuda.current_stream().synchronize()
        return x.clone()
    with pytest.raises(AssertionError, match=r"gate\.query\(\) is True"):
        run_behind_delay(lambda: real, lambda: poison, op, no_host_sync=True, cycles=0, label="control")


# ---- convolutions: forward, data gradient, weight gradient of one case per kernel family -----------------------------
def _conv_inputs(off, cin, cout, k):
    out = []
    for n, d, h, w in SHAPES:
        out += [gen(n, cin, d, h, w, seed=2 + off), gen(cout, cin, k, k, k, seed=3 + off, scale=(k ** 3 * cin) ** -0.5),
                gen(cout, seed=4 + off, scale=0.1), gen(n, cout, d, h, w, seed=8 + off)]
    return out


def _srcs(S, x, split, dtype):
    out, o = [], 0
    for c in split:
        out.append(S.to_cl(x[:, o:o + c], dtype))
        o += c
    return out


def _per_shape(fn):
    def op(*t):
        return [fn(*t[4 * i:4 * i + 4]) for i in range(len(SHAPES))]
    return op


@pytest.mark.parametrize("impl", [0, 1])
def test_conv_tiled(S, impl):
    split, cin, cout, dil = [16], 16, 32, 2

    def one(x, wt, b, dy):
        vox = x.shape[2] * x.shape[3] * x.shape[4]
        srcs, dyc = _srcs(S, x, split, "fp32"), S.to_cl(dy, "fp32")
        (raw,), part, slots = S.conv3d(srcs, wt, b, dil, impl, cin=cin, want_stats=True)
        dx, _, _ = S.conv3d([dyc], wt, None, dil, 0, transpose_flip=True, dst_channels=list(split))
        return raw, part, slots, S.stats_finalize(part, slots, vox), dx, S.conv3d_wgrad(srcs, dyc, cin, cout, 27, dil, impl)
    both(_conv_inputs(0, cin, cout, 3), _conv_inputs(POISON, cin, cout, 3), _per_shape(one), f"conv tiled impl {impl}", True)


def test_conv_stream(S):
    src_c, cin, cout, dil = STREAM_FWD[2]
    assert (src_c, cin, cout, dil) == (16, 16, 32, 2)

    def one(x, wt, b, dy):
        vox = x.shape[2] * x.shape[3] * x.shape[4]
        xc, dyc = S.to_cl(x, "bf16"), S.to_cl(dy, "bf16")
        raw, part, slots = S.conv3d_stream(xc, wt, b, dil, want_stats=True)
        dx, _, _ = S.conv3d_stream(dyc, wt, None, dil, transpose_flip=True, dst_channels=cin)
        return raw, part, slots, S.stats_finalize(part, slots, vox), dx, S.conv3d_wgrad_stream(xc, dyc, cin, cout, dil)
    both(_conv_inputs(0, cin, cout, 3), _conv_inputs(POISON, cin, cout, 3), _per_shape(one), "conv stream", True)


def test_conv_march(S):
    split, cout, dil = MARCH_FWD[0]
    cin = sum(split)
    assert (split, cout, dil) == ([32, 32], 32, 1)

    def one(x, wt, b, dy):
        vox = x.shape[2] * x.shape[3] * x.shape[4]
        srcs, dyc = _srcs(S, x, split, "bf16"), S.to_cl(dy, "bf16")
        (raw,), part, slots = S.conv3d_march(srcs, wt, b, dil, want_stats=True)
        dx, _, _ = S.conv3d_march([dyc], wt, None, dil, transpose_flip=True, dst_channels=list(split))
        return raw, part, slots, S.stats_finalize(part, slots, vox), dx, S.conv3d_wgrad(srcs, dyc, cin, cout, 27, dil, S._lib.CONV_MARCH)
    both(_conv_inputs(0, cin, cout, 3), _conv_inputs(POISON, cin, cout, 3), _per_shape(one), "conv march", True)


def test_conv_1x1x1(S):
    """The tiled kernels at one tap ([32, 8, 16] -> 32) and csrc/wgrad_1x1.hip, forced ([32, 32] -> 32: its first 64 channels)."""
    split, cin, cout = [32, 8, 16], 56, 32

    def one(x, wt, b, dy):
        srcs, dyc = _srcs(S, x[:, :cin], split, "bf16"), S.to_cl(dy, "bf16")
        w56 = wt[:, :cin].contiguous()
        (raw,), part, slots = S.conv3d(srcs, w56, b, 1, 0, cin=cin, want_stats=True)
        dx, _, _ = S.conv3d([dyc], w56, None, 1, 0, transpose_flip=True, dst_channels=list(split))
        return (raw, part, slots, dx, S.conv3d_wgrad(srcs, dyc, cin, cout, 1, 1, 0),
                S.conv3d_wgrad(_srcs(S, x, [32, 32], "bf16"), dyc, 64, cout, 1, 1, S._lib.CONV_MARCH))
    both(_conv_inputs(0, 64, cout, 1), _conv_inputs(POISON, 64, cout, 1), _per_shape(one), "conv 1x1x1", True)


# ---- epilogues, pooling, up-sampling, heads, losses: fp32 and one 16-bit storage mode ------------------------------------
def _stats(S, raw_cl, vox):
    part, slots = S.channel_stats(raw_cl)
    return S.stats_finalize(part, slots, vox)


def _gate_inputs(off, c):
    out = []
    for n, d, h, w in SHAPES:
        out += [gen(n, c, d, h, w, seed=12 + off) * 2 + 0.3, gen(1, c, 1, 1, 1, seed=13 + off, scale=0.5),
                gen(1, c, 1, 1, 1, seed=14 + off, scale=0.5), gen(2, c, 1, 1, 1, seed=15 + off, scale=0.5), gen(2, seed=16 + off, scale=0.1),
                gen(n, c, d, h, w, seed=17 + off), gen(n, d, h, w, 2, seed=18 + off)]
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gate_epilogue(S, dtype):
    def op(*t):
        out = []
        for i in range(len(SHAPES)):
            x, w_se, w_se2, w_side, b_side, g_e, g_side = t[7 * i:7 * i + 7]
            raw = S.to_cl(x, dtype)
            mean, rstd = _stats(S, raw, x.shape[2] * x.shape[3] * x.shape[4])
            e, side = S.gate_epilogue_fwd(raw, mean, rstd, w_se, w_se2, w_side, b_side)
            out.append((e, side, S.gate_epilogue_bwd(raw, mean, rstd, w_se, w_se2, w_side, b_side, g_e=S.to_cl(g_e, dtype), g_side=g_side)))
        return out
    both(_gate_inputs(0, 32), _gate_inputs(POISON, 32), op, f"gate epilogue {dtype}", True)


def _catx_inputs(off, c, inch):
    out = []
    for n, d, h, w in SHAPES:
        out += [gen(n, inch, d, h, w, seed=31 + off) + 0.3, gen(n, c, d, h, w, seed=33 + off) + 0.2, gen(n, c, d, h, w, seed=34 + off),
                gen(c, inch, 1, 1, 1, seed=32 + off) * 0.7]
    return out


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_cat_epilogue_with_recomputed_x_branch(S, dtype):
    c, inch = 32, 2
    td = S._tdtype(S._lib.dtype_code(dtype))

    def op(*t):
        out = []
        for i in range(len(SHAPES)):
            x, r, g, w2 = t[4 * i:4 * i + 4]
            n, _, d, h, w = x.shape
            xin = torch.zeros((n, d, h, w, 8), dtype=td, device="cuda")
            xin[..., :inch] = x.permute(0, 2, 3, 4, 1).to(td)
            raw = S.to_cl(r, dtype)
            mean, rstd = _stats(S, raw, d * h * w)
            out.append(S.cat_epilogue_x(S.to_cl(g, dtype), raw, mean, rstd, xin, w2, inch))
        return out
    both(_catx_inputs(0, c, inch), _catx_inputs(POISON, c, inch), op, f"cat epilogue x {dtype}", True)


def _resample_inputs(off):
    n, d, h, w = EVEN
    g0 = torch.Generator().manual_seed(50 + off)
    out = [torch.randint(0, 3, (n, 24, d, h, w), generator=g0).float(), gen(n, 24, d // 2, h // 2, w // 2, seed=51 + off),
           gen(n, 24, d, h, w, seed=30 + off)]
    for (n, d, h, w) in SHAPES:
        out += [gen(n, 16, d, h, w, seed=41 + off), gen(n, 16, 2 * d, 2 * h, 2 * w, seed=42 + off), gen(n, 16, d, h, w, seed=43 + off)]
    n, c, d, h, w = min(UP2_FORMS, key=lambda s: (UP2_FORMS[s] != ("march",) * 3 + ("tiled",), s[1] * s[2] * s[3] * s[4]))
    out += [gen(n, c, d, h, w, seed=41 + off), gen(n, c, 2 * d, 2 * h, 2 * w, seed=42 + off), gen(n, c, d, h, w, seed=43 + off)]
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_maxpool_and_upsample2(S, dtype):
    """Pooling at (2, 6, 10, 40) with ties; 2x up-sampling at the two ragged shapes and at the smallest UP2_FORMS shape that takes
    the marching kernels."""
    def op(x, g, prev, *ups):
        xc, gc = S.to_cl(x, dtype), S.to_cl(g, dtype)
        out = [S.maxpool_fwd(xc), S.maxpool_bwd(xc, gc), S.maxpool_bwd(xc, gc, S.to_cl(prev, dtype))]
        for i in range(0, len(ups), 3):
            gu = S.to_cl(ups[i + 1], dtype)
            out += [S.upsample2_fwd(S.to_cl(ups[i], dtype)), S.upsample2_bwd(gu), S.upsample2_bwd(gu, g_in=S.to_cl(ups[i + 2], dtype))]
        return out
    both(_resample_inputs(0), _resample_inputs(POISON), op, f"maxpool, upsample2 {dtype}", True)


HEAD_CASES = [(2, 16, 8, 24, 4), (1, 8, 4, 20, 3)]


def _head_inputs(off):
    out = []
    for n, d, h, w, nl in HEAD_CASES:
        out += [gen(n, d >> l, h >> l, w >> l, seed=33 + l + off) for l in range(nl)] + [gen(1, seed=40 + off), gen(n, 1, d, h, w, seed=41 + off)]
    return out


def test_heads(S):
    """The heads read and write f32 level maps in every storage mode: one run."""
    def op(*t):
        out, o = [], 0
        for n, d, h, w, nl in HEAD_CASES:
            maps, bias, g = list(t[o:o + nl]), t[o + nl], t[o + nl + 1]
            o += nl + 2
            out.append((S.head_fwd(maps, bias), S.head_bwd(g, nl)))
        return out
    both(_head_inputs(0), _head_inputs(POISON), op, "heads", True)


def _loss_inputs(seed):
    import test_loss_layers_gpu as TL
    out = []
    for n, d, h, w in SHAPES:
        shape = (n, 1, d, h, w)
        xe, t, w_, s = TL.shaped(shape, shape, seed=seed)
        out += [xe.clone(), xe * 0.5 + 0.1, t, w_, s]
    return out


@pytest.mark.parametrize("stage", (1, 3))
def test_fused_stage_loss(A, stage):
    """Forward and backward (the backward runs on autograd's thread, which looks the stream up again).  The logits of both heads
    are f32 in every storage mode: one run per stage."""
    def op(*t):
        out = []
        for i in range(len(SHAPES)):
            xe, xd, lab, w, s = t[5 * i:5 * i + 5]
            xe, xd = xe.detach().requires_grad_(), xd.detach().requires_grad_()
            loss = A.fused_stage_loss(stage, xe, xd, lab, w, s)
            loss.backward()
            out.append((loss.detach(), xe.grad, xd.grad))
        return out
    both(_loss_inputs(41), _loss_inputs(41 + POISON), op, f"stage {stage} loss", True)


# ---- the whole network ---------------------------------------------------------------------------------------------------
_MODELS = {}


def model(A, dtype, input_grad=False, tag=""):
    """One network per (storage mode, input_grad, tag), built on the default stream with the deterministic weights."""
    import seunet_oracle as orc
    key = (dtype, input_grad, tag)
    if key not in _MODELS:
        m = A.SE_UNet(in_channel=2, n_classes=1, act_dtype=dtype, input_grad=input_grad)
        m.load_state_dict(orc.deterministic_state_dict(2, 1, 1, seed=0))
        _MODELS[key] = m.cuda().eval()
        torch.cuda.synchronize()
    return _MODELS[key]


def batch(n, size, seed):
    import seunet_oracle as orc
    b = orc.synthetic_batch(n, size, 2, seed=seed)
    return [b["image"], b["label"]]


def step_op(A, m, input_grad=False):
    def op(x, lab):
        for p in m.parameters():
            p.grad = None
        x = x.detach()
        if input_grad:
            x.requires_grad_(True)
        e, d = m(x)
        loss = A.fused_stage_loss(1, e, d, lab)
        loss.backward()
        grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        assert len(grads) > 100
        return loss.detach(), e.detach(), d.detach(), grads, (x.grad if input_grad else None)
    return op


@pytest.mark.parametrize("dtype,input_grad", [("fp32", False), ("bf16", False), ("fp16", False), ("bf16", True)])
def test_network_step(A, dtype, input_grad):
    """Forward, stage-1 loss and backward at 2 x 2 x 32^3, all issued under the side stream: the logits, the loss and every
    parameter gradient (and the input gradient where asked for)."""
    m = model(A, dtype, input_grad)
    got, _ = both(batch(2, (32, 32, 32), 13), batch(2, (32, 32, 32), 13 + POISON), step_op(A, m, input_grad),
                  f"network step {dtype}{' input_grad' if input_grad else ''}", True)
    assert (got[4] is not None) == input_grad and bool(torch.isfinite(got[0]))


def test_predict_logits_twice(A):
    """The second call reuses the arena of the first."""
    m = model(A, "bf16")

    def op(x):
        first = m.predict_logits(x).clone()
        return first, m.predict_logits(x), len(m._arena)
    real, poison = batch(2, (32, 32, 32), 23)[:1], batch(2, (32, 32, 32), 23 + POISON)[:1]
    got, _ = both(real, poison, op, "predict_logits", True)
    assert got[2] == 1 and torch.equal(got[0], got[1])
    with torch.no_grad():
        assert torch.equal(got[0], m(real[0].cuda())[1])


def test_captured_forward_recorded_and_replayed(A):
    """The graph is recorded (first call) and replayed (second call) with the side stream current; the expected bits are the eager
    forward's on the default stream."""
    m = model(A, "bf16")
    real, poison = batch(2, (32, 32, 32), 31)[:1], batch(2, (32, 32, 32), 31 + POISON)[:1]
    with torch.no_grad():
        e0, e1 = m(real[0].cuda())
    torch.cuda.synchronize()

    def op(x):
        cap = A.CapturedForward(m, 2, (32, 32, 32))
        out = []
        for _ in range(2):
            cap.x.copy_(x)
            p0, p1 = cap()
            out.append((p0.clone(), p1.clone()))
        return out
    got = run_behind_delay(lambda: real, lambda: poison, op, label="CapturedForward")
    same_bits(got, [(e0, e1), (e0, e1)], "CapturedForward: replays on the side stream against the eager forward")


# ---- inference loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("size", list(WINDOW_CASES))
def test_sliding_window_predict(A, size, graph):
    """cube 32, step 16, batch 2: 48 x 32 x 64 is three full batches, 64 x 32 x 64 four full batches and a ragged last one (with
    ``graph`` the full batches replay the recorded graph and the ragged one runs eagerly)."""
    import seunet_oracle as orc
    n = len(A.window_table(size, 32, 16))
    assert (n // 2, n % 2) == WINDOW_CASES[size] and n >= 4
    m = model(A, "fp32")
    real = [orc.synthetic_batch(1, size, 2, seed=10)["image"]]
    poison = [orc.synthetic_batch(1, size, 2, seed=10 + POISON)["image"]]
    got, _ = both(real, poison, lambda x: A.sliding_window_predict(m, x, cube=32, step=16, batch=2, graph=graph),
                  f"window loop {size} graph={graph}")
    assert got.shape == size and got.dtype == np.float64 and 0.0 <= float(got.min()) < float(got.max()) <= 1.0


# ---- optimiser and mining ---------------------------------------------------------------------------------------------------
ADAMW_SHAPES = [(5,), (1,), (257, 9), (4, 4, 3, 3, 3), (2049,)]              # the ragged list of tests/test_optim_gpu.py


def _adamw_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g) * 0.1 for s in ADAMW_SHAPES]
    return init + [torch.randn(s, generator=g) * 1e-3 for _ in range(4) for s in ADAMW_SHAPES]


def test_adamw_four_steps(A):
    import adamw_oracle as ao
    k = len(ADAMW_SHAPES)

    def op(*t):
        params = [torch.nn.Parameter(v) for v in t[:k]]
        opt = A.AdamW(params, lr=1e-4)
        for s in range(4):
            for i, p in enumerate(params):
                p.grad = t[k * (s + 1) + i]
            opt.step()
        return [p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params]
    real = _adamw_inputs(7)
    (params, _, exp_avg_sq), _ = both(real, _adamw_inputs(7 + POISON), op, "AdamW", True)
    want = ao.run([v.numpy() for v in real[:k]], [[v.numpy() for v in real[k * (s + 1):k * (s + 2)]] for s in range(4)], [1e-4] * 4)
    for i, p in enumerate(params):
        np.testing.assert_allclose(host(p), want["params"][i], rtol=2e-7, atol=1e-9)
        np.testing.assert_allclose(host(exp_avg_sq[i]), want["exp_avg_sq"][i], rtol=2e-6, atol=3e-7 * float(np.abs(want["exp_avg_sq"][i]).max()))


def test_adamw_four_steps_gated_with_a_skip_at_step_two(A):
    """The gated step (``overflow_gate=``): the flag an overflowing backward would raise arrives with the other inputs, behind
    the delay (poison: another step is skipped), and the prepare kernel, its table and the flag's reset are on the caller's
    stream.  Against the oracle run on steps one, three and four."""
    import adamw_oracle as ao
    k = len(ADAMW_SHAPES)
    raised = lambda *steps: [torch.tensor([int(s in steps) for s in range(4)], dtype=torch.int32)]

    def op(*t):
        params = [torch.nn.Parameter(v) for v in t[:k]]
        flag = torch.zeros((), dtype=torch.int32, device="cuda")
        opt = A.AdamW(params, lr=1e-4, overflow_gate=flag)
        for s in range(4):
            for i, p in enumerate(params):
                p.grad = t[k * (s + 1) + i]
            flag.bitwise_or_(t[-1][s])
            opt.step()
        return ([p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params],
                [opt.state[p]["skipped"] for p in params], flag)
    real = _adamw_inputs(7) + raised(1)
    (params, exp_avg, exp_avg_sq, skipped, flag), _ = both(real, _adamw_inputs(7 + POISON) + raised(2), op, "AdamW gated", True)
    assert int(flag) == 0 and [float(v) for v in skipped] == [1.0] * k
    want = ao.run([v.numpy() for v in real[:k]], [[v.numpy() for v in real[k * (s + 1):k * (s + 2)]] for s in (0, 2, 3)], [1e-4] * 3)
    for i, p in enumerate(params):
        np.testing.assert_allclose(host(p), want["params"][i], rtol=2e-7, atol=1e-9)
        for got, key in ((exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            np.testing.assert_allclose(host(got[i]), want[key][i], rtol=2e-6, atol=3e-7 * float(np.abs(want[key][i]).max()))


def _psl_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    shape = (4, 1, 6, 9, 40)
    t = (torch.rand(shape, generator=g) < 0.1).float()
    return [torch.randn(shape, generator=g), t, 1 + torch.rand(shape, generator=g), t * (torch.rand(shape, generator=g) < 0.5).float()]


def test_per_sample_loss(A):
    def op(x, t, w, s):
        return A.per_sample_loss(x, t, w, apply_sigmoid=True), A.per_sample_loss(x, t, w, s, c_dice=0.5, c_gul=1.0, c_atr=0.5, apply_sigmoid=True)
    got, _ = both(_psl_inputs(1), _psl_inputs(1 + POISON), op, "per_sample_loss", True)
    assert got[0].shape == (4,) and bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())


POOL_SHAPE = (1, 4, 4)


def _pool_inputs(run, first_id):
    """The recorded key stream of a fixture run, with payloads whose first voxel names the sample (as test_online_pool_gpu.py)."""
    keys = np.load(os.path.join(GOLDEN, "online_pool_known.npz"))[f"run{run}_keys"]
    steps, B = keys.shape
    ids = first_id + torch.arange(steps * B, dtype=torch.float32).reshape(steps, B)
    data = torch.zeros((steps, B, 2) + POOL_SHAPE)
    data[:, :, 0, 0, 0, 0] = ids
    label = ((torch.arange(steps * B * 16).reshape((steps, B, 1) + POOL_SHAPE) + first_id) % 3 == 0).float()
    return [torch.from_numpy(keys), data, label, data[:, :, :1] + 0.5]


def test_online_pool_epoch(A):
    """One epoch on the recorded key stream of fixture run 7 (three tensors and a skeleton, 3 offers per step, 7 slots): offers and
    evictions without a host wait, then the replay pass, against tests/pool_oracle.py and the recorded survivors and replays.
    The poison is run 8's key stream with other payloads."""
    from pool_oracle import PoolOracle
    known = np.load(os.path.join(GOLDEN, "online_pool_known.npz"))
    run = 7
    three, B, K = (int(v) for v in known[f"run{run}_config"])
    assert three == 1 and tuple(known["run8_config"])[:2] == (three, B)
    real, poison = _pool_inputs(run, 0), _pool_inputs(8, 5000)
    steps = real[0].shape[0]
    rates = known["rates"].tolist()

    def offer(pool):
        def op(keys, data, label, weight):
            pool.clear()
            return [pool.add(keys[it], data[it], label[it], weight[it], skel=label[it]).clone() for it in range(steps)]
        return op

    def replay(pool):
        n = len(pool)
        alive = sorted(int(v) for v in pool.data[:n, 0, 0].tolist())
        batches = {}
        for k, rate in enumerate(rates):
            it = pool.replay(batch_size=1, rate=rate, generator=torch.Generator().manual_seed(100 + k))
            batches[k] = [(int(b["data"][0, 0, 0, 0, 0]), b["weight"].clone(), b["skel"].clone()) for b in it]
        return n, alive, batches

    def on_the_default_stream():
        pool = A.OnlineHardPool(K, cube=POOL_SHAPE, with_skel=True)
        return serial(real, offer(pool)), replay(pool)

    def on_a_side_stream():
        pool = A.OnlineHardPool(K, cube=POOL_SHAPE, with_skel=True)          # (its storage is made on the default stream)
        d = Delayed(lambda: real, lambda: poison, label="OnlineHardPool.add")
        try:
            slots = d.open().call(offer(pool), no_host_sync=True)
            return slots, d.call(lambda *_: replay(pool))
        finally:
            d.finish()
    want, got = on_the_default_stream(), on_a_side_stream()
    same_bits(got, want, "online pool: side stream against default stream")
    oracle = PoolOracle(K)
    for it in range(steps):
        assert got[0][it].tolist() == oracle.add(real[0][it].tolist(), list(range(it * B, (it + 1) * B))), it
    n, alive, batches = got[1]
    assert n == K and alive == sorted(int(v) for v in known[f"run{run}_survivors"][-1] if v >= 0)
    for k in range(len(rates)):
        assert sorted(b[0] for b in batches[k]) == sorted(known[f"run{run}_replay{k}"].tolist()), k
        assert all(float(b[1][0, 0, 0, 0, 0]) == b[0] + 0.5 for b in batches[k])


# ---- volume operations ---------------------------------------------------------------------------------------------------------
def volumes(real, op, label):
    """``op`` on numpy volumes behind the delay, the poison being the volumes turned round."""
    return both(real, [other(v) for v in real], op, label)[0]


def test_distance_transform(A):
    from scipy import ndimage
    v = np.load(os.path.join(GOLDEN, "prep_known.npz"))["edt1_vol"]            # (5, 40, 37): rows that cross a 64-voxel word
    sq, dist, ind = volumes([v], lambda t: A.distance_transform_edt(t, return_indices=True, return_sqdist=True), "EDT")
    ref_dist, ref_ind = ndimage.distance_transform_edt(v, return_indices=True)
    assert np.array_equal(host(ind), ref_ind.astype(np.int32)) and np.array_equal(host(dist).view(np.int64), ref_dist.view(np.int64))
    assert np.array_equal(host(sq).astype(np.int64), ((ref_ind.astype(np.int64) - np.indices(v.shape)) ** 2).sum(0))


def test_prep_weights_and_candidates(A):
    g, p = np.load(os.path.join(GOLDEN, "prep_known.npz")), "case0_"

    def op(label, skeleton, pred):
        w, br = A.break_weight(label, pred, skeleton)
        skel, small = A.hard_mining_candidates(label, skeleton, pred)
        cs = A.CandidateSet.from_mask(br)
        draws = [c.coords(k) for c in (skel, small, cs) for k in (0, len(c) // 2, len(c) - 1) if len(c)]
        return A.lib_weight(label), w, [c.to_numpy() for c in (skel, small, cs)], draws
    lib, w_br, sets, draws = volumes([g[p + "label"], g[p + "skeleton"], g[p + "pred"]], op, "prep")
    for cs, ref in zip(sets, (np.where(g[p + "loc_skeleton"]), np.where(g[p + "loc_small"]), tuple(g[p + "loc_break"].astype(np.int64)))):
        assert all(np.array_equal(a, b) for a, b in zip(cs, ref))
    assert len(draws) == 9
    assert np.array_equal(host(lib).view(np.int16), g[p + "lib"].view(np.int16)) and np.array_equal(host(w_br).view(np.int16), g[p + "w_br"].view(np.int16))


@pytest.mark.parametrize("name", ["tree", "noise"])
def test_skeletonize(A, name):
    v, want, passes = so.solved(name)
    got, got_passes = volumes([np.array(v)], lambda t: A.skeletonize_3d(t, return_passes=True), f"skeleton {name}")
    assert np.array_equal(host(got), want) and got_passes == passes


def _parse_case(i):
    z = np.load(os.path.join(GOLDEN, "parse_known.npz"))
    return {k[len(f"case{i}_"):]: z[k] for k in z.files if k.startswith(f"case{i}_")}


def test_tree_parsing(A):
    c = _parse_case(2)                                                          # (20, 24, 134): the smallest, rows of three words
    got, num = volumes([c["label"], c["skeleton"]], lambda lab, sk: A.tree_parsing(lab, sk, return_num=True), "tree_parsing")
    assert num == int(c["num"]) and np.array_equal(host(got), c["parsing"].astype(np.int32))


def test_airway_parse(A):
    z = np.load(os.path.join(GOLDEN, "topology_known.npz"))
    label = (z["case2_label"] != 0).astype(np.uint8)                            # (24, 26, 70)
    poison = (z["case3_label"] != 0).astype(np.uint8)                           # the other recorded tree of that shape
    got, _ = both([label], [poison], lambda t: A.airway_parse(t), "airway_parse")
    assert np.array_equal(host(got), z["case2_parsing"].astype(np.int32))


def test_morphology_and_fill_holes(A):
    from scipy import ndimage
    v = (np.random.default_rng(74).random((4, 5, 65)) < 0.5).astype(np.uint8)
    shell = so.make_case("shell")

    def op(t, s):
        return A.binary_dilation(t), A.binary_erosion(t), A.binary_erosion(t, border_value=1), A.binary_closing(t), A.binary_fill_holes(s)
    dil, er0, er1, clo, filled = volumes([v, shell], op, "morphology")
    assert np.array_equal(host(dil), ndimage.binary_dilation(v).astype(np.uint8))
    assert np.array_equal(host(er0), ndimage.binary_erosion(v).astype(np.uint8))
    assert np.array_equal(host(er1), ndimage.binary_erosion(v, border_value=1).astype(np.uint8))
    assert np.array_equal(host(clo), ndimage.binary_erosion(ndimage.binary_dilation(v), border_value=1).astype(np.uint8))
    assert np.array_equal(host(filled), ndimage.binary_fill_holes(shell).astype(np.uint8))


def test_largest_component_and_maximum_3d(A):
    import components_oracle as co
    from test_components_gpu import _volume
    shape = (9, 8, 65)
    v, p = _volume("blobs", shape, 31 * sum(shape) + 5), _volume("blobs", shape, 31 * sum(shape) + 5 + POISON)
    largest, maxi = both([v], [p], lambda t: (A.largest_component(t), A.maximum_3d(t)), "components")[0]
    np.testing.assert_array_equal(host(largest), co.largest_component(v))
    np.testing.assert_array_equal(host(maxi).astype(bool), co.maximum_3d(v))


def test_evaluation_case(A):
    import components_oracle as co
    real, poison = co.synthetic_tree((48, 40, 56), 7), co.synthetic_tree((48, 40, 56), 8)
    got = both(list(real), list(poison), lambda *t: tuple(A.evaluation_case(*t)), "evaluation_case")[0]
    assert got == tuple(co.evaluation_case(*real))


def test_double_threshold_iteration(A):
    import dti_oracle as do
    shape = (5, 7, 65)
    v, p = np.random.default_rng(77).random(shape), np.random.default_rng(77 + POISON).random(shape)
    got = both([v], [p], lambda t: [A.double_threshold_iteration(t, 0.62, 0.37, pred_dtype=pd) for pd in ("float64", "float32")], "double threshold")[0]
    for g, pd in zip(got, ("float64", "float32")):
        np.testing.assert_array_equal(host(g), do.double_threshold_iteration(v, 0.62, 0.37, pd).astype(np.uint8))


def test_preprocess_ct_and_cut_mask(A):
    """Fixture ``a`` (prepro mode: data cut, lung mask and the box read back) and its labelled mask ``e``; the poison is the scan
    and the mask turned round."""
    z = np.load(os.path.join(GOLDEN, "lung_known.npz"))
    assert np.array_equal(z["e_box"], z["a_box"])

    def op(ct, label):
        data_cut, lung_mask, box = A.preprocess_ct(ct)
        return data_cut, lung_mask, np.asarray(box), A.cut_mask(label, box)
    data_cut, lung_mask, box, cut = volumes([z["a_ct"], z["e_label"]], op, "preprocessing")
    assert np.array_equal(host(data_cut), z["a_data_cut"]) and np.array_equal(host(lung_mask), z["a_lung_mask"])
    assert np.array_equal(box, z["a_box"]) and np.array_equal(host(cut), z["e_mask_cut"])


def test_crop_batch(A):
    import pipeline_oracle as po
    from test_pipeline_gpu import _case
    shape, starts, codes = (70, 66, 100), [(3, 1, 36), (6, 2, 0)], [5, 10]
    real, poison = _case(5, shape), _case(5 + POISON, shape)
    got = both(list(real), list(poison), lambda img, label, w16, skel: A.crop_batch(img, starts, 64, label, w16, skel, codes, u=0.37), "pipeline")[0]
    want = po.crop_batch(real[0], starts, codes, 64, real[1], real[2], real[3], 0.37)
    for k in ("data", "label", "skel"):
        np.testing.assert_array_equal(host(got[k]), want[k], err_msg=k)


def test_mesh_extraction_smoothing_and_stl(A):
    import mesh_oracle as mo
    shape = (5, 6, 67)
    v = (np.random.default_rng(sum(shape)).random(shape) < 0.5).astype(np.uint8)
    v[1, 2, 63] = v[1, 2, 64] = 1
    centre, scale = (2.5, 3.0, 31.25), (0.07, 0.08, 0.125)

    def op(t):
        verts, faces = A.marching_cubes(t)
        smooth = A.smooth_mesh(verts, faces, n_iter=3)
        return verts, faces, smooth, A.stl_records(smooth, faces, centre, scale)
    verts, faces, smooth, stl = volumes([v], op, "mesh")
    wv, wf = mo.marching_cubes(v)
    ws = mo.smooth(wv, wf, 3, 0.2)
    assert np.array_equal(bits(host(verts)), bits(wv)) and np.array_equal(host(faces), wf)
    assert np.array_equal(bits(host(smooth)), bits(ws)) and np.array_equal(host(stl), mo.stl_records(ws, wf, centre, scale))


def test_label_meshes(A):
    import mesh_label_oracle as lo
    shape = (5, 6, 67)
    L = lo.random_labels(shape, 3, 0.5, sum(shape))
    L[1, 2, 63], L[1, 2, 64] = 1, 2
    got = volumes([L], lambda t: A.label_meshes(t), "label_meshes")
    res = lo.label_meshes(L)
    assert np.array_equal(got.vert_ptr, res[2]) and np.array_equal(got.face_ptr, res[3])
    assert np.array_equal(host(got.faces), res[1]) and np.array_equal(bits(host(got.verts)), bits(res[0]))


def test_branch_morphometry(A):
    import morphometry_oracle as mo
    from test_scratch_and_bounds_morphometry_gpu import NUM, SPACING, same, want
    parsing, skeleton, sqdist, rows = want((2, 3, 67))
    poison = [np.ascontiguousarray(np.roll(a, 7, axis=-1)) for a in (parsing, skeleton, sqdist)]
    got = both([parsing, skeleton, sqdist], poison, lambda p, s, q: A.branch_morphometry(p, s, SPACING, NUM, q), "morphometry")[0]
    same(got, rows)
    derived = mo.derived(rows, SPACING)
    for k in mo.FLOAT_COLUMNS:
        np.testing.assert_allclose(getattr(got, k), derived[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


# ---- two streams at once --------------------------------------------------------------------------------------------------------
def test_two_side_streams_at_once(A):
    """Two side streams, each behind a delay of its own, fed alternately from one host thread: skeletonize_3d on one and the
    distance transform on the other, then two network steps of different shapes whose launches interleave.  Each result must equal
    its serial result: device state shared behind the caller's back would show."""
    v, skel_want, passes = so.solved("tree")
    e = np.load(os.path.join(GOLDEN, "prep_known.npz"))["edt1_vol"]
    skel_op = lambda t: A.skeletonize_3d(t, return_passes=True)                 # noqa: E731
    edt_op = lambda t: A.distance_transform_edt(t, return_indices=True)        # noqa: E731
    want_s, want_e = serial([np.array(v)], skel_op), serial([e], edt_op)
    da = Delayed(lambda: [np.array(v)], lambda: [other(np.array(v))], label="two streams: skeleton")
    db = Delayed(lambda: [e], lambda: [other(e)], label="two streams: EDT")
    da.open(), db.open()
    db.assert_pending("after the other stream was opened")
    got_s, got_e = da.call(skel_op), db.call(edt_op)
    da.finish(), db.finish()
    same_bits(got_s, want_s, "skeleton beside the EDT")
    same_bits(got_e, want_e, "EDT beside the skeleton")
    assert np.array_equal(host(got_s[0]), skel_want) and got_s[1] == passes

    ma, mb = model(A, "bf16", tag="a"), model(A, "fp16", tag="b")
    ra, rb = batch(2, (32, 32, 32), 13), batch(1, (40, 48, 56), 14)
    want_a, want_b = serial(ra, step_op(A, ma)), serial(rb, step_op(A, mb))
    for m in (ma, mb):
        for p in m.parameters():
            p.grad = None
    da = Delayed(lambda: ra, lambda: batch(2, (32, 32, 32), 13 + POISON), label="two streams: step 32^3")
    db = Delayed(lambda: rb, lambda: batch(1, (40, 48, 56), 14 + POISON), label="two streams: step 40x48x56")
    # torch's allocator keeps a pool per stream: a step's first run on a stream grows that pool with hipMalloc calls, which at
    # 40 x 48 x 56 take longer on the host than the delay.  So each stream first runs its step once, undelayed.
    for d, m, r, w in ((da, ma, ra, want_a), (db, mb, rb, want_b)):
        with torch.cuda.stream(d.stream):
            same_bits(step_op(A, m)(*[to_device(v) for v in r]), w, f"{d.label}: undelayed on its stream")
        for p in m.parameters():
            p.grad = None
    torch.cuda.synchronize()
    da.open(), db.open()
    fa = da.call(lambda x, lab: ma(x) + (lab,), no_host_sync=True)
    fb = db.call(lambda x, lab: mb(x) + (lab,), no_host_sync=True)
    out = []
    for d, m, (pe, pd, lab) in ((da, ma, fa), (db, mb, fb)):
        def rest(*_):
            loss = A.fused_stage_loss(1, pe, pd, lab)
            loss.backward()
            return loss.detach(), pe.detach(), pd.detach(), {n: p.grad for n, p in m.named_parameters() if p.grad is not None}, None
        out.append(d.call(rest, no_host_sync=True))
    db.assert_pending("after all four calls were issued")
    da.finish(), db.finish()
    same_bits(out[0], want_a, "step at 32^3 beside the step at 40x48x56")
    same_bits(out[1], want_b, "step at 40x48x56 beside the step at 32^3")


# ---- first use of the library on a side stream -------------------------------------------------------------------------------------
def test_first_library_call_on_a_side_stream_in_a_fresh_process(A):
    """tests/side_stream_first_use.py in a child process: its first library calls are a marching and a 1x1x1 weight gradient under
    a side stream, so the per-device page of zeros those kernels pad through is made while another stream than the default one
    is current.  (A missing wait there cannot be made to fail deterministically; this runs the path at all.)"""
    cmd = [sys.executable, os.path.join(HERE, "side_stream_first_use.py")]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit("the first-use child process hung: nothing further is started on this GPU", returncode=1)
    if r.returncode < 0:
        pytest.exit(f"the first-use child process died on signal {-r.returncode}: nothing further is started on this GPU\n{r.stderr[-2000:]}",
                    returncode=1)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "first use OK" in r.stdout


def test_report_the_enqueue_times(A):
    print(f"\ndelay {SS.DELAY_MS} ms; host milliseconds from the delay's start to the return of each call that must not wait:")
    for k, v in sorted(SS.ENQUEUE_MS.items(), key=lambda kv: -kv[1]):
        print(f"  {v:8.2f}  {k}")
    assert all(v < SS.DELAY_MS for v in SS.ENQUEUE_MS.values())
