"""The machinery of the convolutions' number-range tests (tests/test_conv_range_gpu.py and the host module
tests/test_range_host.py; the epilogues' side is tests/range_epilogue_cases.py): every convolution pass at the two ends of its
storage type's range and on non-finite input.

fp16 training carries every activation gradient times a static loss scale of 65536 and drops a step when a parameter gradient
is not finite.  That is only correct if every backward pass (a) keeps fp16 subnormals -- operands and results below 2^-14 --
and (b) stores what leaves the range as +-inf and hands every inf / NaN it reads on to everything that value contributes to.

Convolutions: exact, by scaled integers.  The operands are the small integers of tests/conv_layer_cases.py; ONE of them -- the
one that stands for a gradient (dy; in the forward x and the bias) -- is multiplied by a power of two 2^s.  Every product and
partial sum is then an integer below 2^24 times 2^s, exact in f32 in any order (in f32's own subnormal range too: a subnormal
is an integer multiple of 2^-149, and 2^s is one), so the stored result is ``ldexp(integer reference, s)`` rounded ONCE to the
storage type.  The reference never convolves scaled operands on the CPU (a CPU library may flush on its own); the comparison
is on bit patterns, so that inf equals inf and a NaN cannot slip through ``==`` (all NaNs count as one pattern, and -0 as +0:
neither payload nor the sign of a zero reaches an optimiser step).

All operands are drawn with the CPU generator and converted to the storage type on the CPU, so the host module sees the very
tensors the GPU module runs, and no device kernel sits between the draw and the kernel under test."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_layer_cases as L  # noqa: E402

Q_EXP = {"fp16": -24, "bf16": -133}          # each type's smallest subnormal
MIN_NORMAL_EXP = {"fp16": -14, "bf16": -126}
FP16_INF_FROM = 65520.0                       # the first value that rounds to inf (65504 is the largest finite one)


# ---- case table ---------------------------------------------------------------------------------------------------------------
def layer(name, fwd, dgrad, wgrad, src_c, cin, cout, dilation, taps, dims):
    return {"name": name, "fwd": fwd, "dgrad": dgrad, "wgrad": wgrad, "src_c": list(src_c), "cin": cin, "cout": cout,
            "dilation": dilation, "taps": taps, "dims": tuple(dims)}


SMALL = (2, 6, 9, 40)       # ragged patches in y and x, more than one workgroup: the shape of tests/test_ops_gpu.py
# Every kernel FORCED, as tests/test_ops_gpu.py does (these volumes are far below the sizes at which the dispatcher would pick
# the marching and whole-GEMM kernels by itself).  A None pass is not run for that entry.
FWD_DGRAD = [
    layer("stream-2of8-8", "Stream", None, None, [8], 2, 8, 1, 27, SMALL),                 # ec1: runs no data gradient
    layer("stream-8-16", "Stream", "Stream", None, [8], 8, 16, 1, 27, SMALL),              # ec2
    layer("stream-16-32-d2", "Stream", "Stream", None, [16], 16, 32, 2, 27, SMALL),        # ec3
    layer("stream-32-16", "Stream", "Stream", None, [32], 32, 16, 1, 27, SMALL),           # dc6
    layer("march-32+32-32", "March", "March", None, [32, 32], 64, 32, 1, 27, SMALL),       # dc5: two sources / destinations
    layer("march-64-64-d2", "March", "March", None, [64], 64, 64, 2, 27, SMALL),           # ec8 / ec9
    layer("tiled-64-64", "Tiled", "Tiled", None, [64], 64, 64, 1, 27, SMALL),              # staged store path
    layer("tiled-16-32", "Tiled", "Tiled", None, [16], 16, 32, 1, 27, SMALL),              # direct store path (<= 16 channels)
    layer("tiled-1x1-32+8+16-32", "Tiled", "Tiled", None, [32, 8, 16], 56, 32, 1, 1, SMALL),
]
WGRAD = [
    layer("stream-2of8-8", None, None, "Stream", [8], 2, 8, 1, 27, SMALL),
    layer("stream-16-32-d2", None, None, "Stream", [16], 16, 32, 2, 27, SMALL),
    layer("stream-32-16", None, None, "Stream", [32], 32, 16, 1, 27, SMALL),
    # the marching weight gradient: n = 2, h = 6, w = 40 with its per-case depth (tests/test_ops_gpu.py)
    layer("march-32+32-32", None, None, "March", [32, 32], 64, 32, 1, 27, (2, 37, 6, 40)),
    layer("march-64-32", None, None, "March", [64], 64, 32, 1, 27, (2, 5, 6, 40)),
    layer("march-32-32-d2", None, None, "March", [32], 32, 32, 2, 27, (2, 6, 6, 40)),
    layer("tiled-16-32-d2", None, None, "Tiled", [16], 16, 32, 2, 27, (2, 5, 6, 40)),
    layer("tiled-1x1-32+8+16-32", None, None, "Tiled", [32, 8, 16], 56, 32, 1, 1, (2, 5, 6, 40)),
    # the 1x1x1 whole-GEMM kernel: the shapes of test_conv_weight_gradient_1x1
    layer("1x1-64+32+32-64", None, None, "Wgrad1x1", [64, 32, 32], 128, 64, 1, 1, (2, 5, 6, 40)),
    layer("1x1-64+64+64-128", None, None, "Wgrad1x1", [64, 64, 64], 192, 128, 1, 1, (1, 9, 8, 24)),
    layer("1x1-32+32-32", None, None, "Wgrad1x1", [32, 32], 64, 32, 1, 1, (2, 3, 5, 7)),
    layer("1x1-64+64-64", None, None, "Wgrad1x1", [64, 64], 128, 64, 1, 1, (1, 16, 16, 16)),
]
FWD_CASES = [(c["name"], dt) for c in FWD_DGRAD for dt in L.DTYPES]
DGRAD_CASES = [(c["name"], dt) for c in FWD_DGRAD if c["dgrad"] for dt in L.DTYPES]
WGRAD_CASES = [(c["name"], dt) for c in WGRAD for dt in L.DTYPES]
BY_NAME = {("fd", c["name"]): c for c in FWD_DGRAD} | {("w", c["name"]): c for c in WGRAD}
COVERED = ({(c["fwd"], "fwd") for c in FWD_DGRAD} | {(c["dgrad"], "dgrad") for c in FWD_DGRAD if c["dgrad"]}
           | {(c["wgrad"], "wgrad") for c in WGRAD})


def seed_for(kind, name):
    return 5000 + 100 * ("fwd", "dgrad", "wgrad").index(kind) + 7 * [c["name"] for c in (WGRAD if kind == "wgrad" else FWD_DGRAD)].index(name)


_data = {}


def data(kind, name, nonfinite=False):
    """The integer operands and the exact integer reference of one case, on the CPU, computed once per process.
    nonfinite: weights without 0 (no ``0 * inf`` whose outcome would be an implementation's choice) and a third sample that
    carries no plant, so that "every other sample is untouched" has something to look at."""
    key = (kind, name, nonfinite)
    if key not in _data:
        c = BY_NAME[("w" if kind == "wgrad" else "fd", name)]
        if nonfinite:
            c = dict(c, dims=(3,) + c["dims"][1:])
        seed = seed_for(kind, name)
        if kind == "fwd":
            x, wt, b, ref, _, _ = L.forward_data(c, seed, "cpu", nonzero_w=nonfinite)
            _data[key] = c, {"x": x, "wt": wt, "b": b, "ref": ref}
        elif kind == "dgrad":
            dy, wt, ref, prev = L.dgrad_data(c, seed, "cpu", nonzero_w=nonfinite)
            _data[key] = c, {"dy": dy, "wt": wt, "ref": ref, "prev": prev}
        else:
            x, dy, ref = L.wgrad_data(c, seed, "cpu")
            _data[key] = c, {"x": x, "dy": dy, "ref": ref}
    return _data[key]


# ---- exact scaling, bit patterns ----------------------------------------------------------------------------------------------
def scaled(t, s):
    """t (integers, any dtype) times 2^s as f32 on the CPU, asserted exact (scaled back in float64 it gives the integers:
    a CPU that flushed f32 subnormals would fail here, not in a kernel's comparison)."""
    v = t.float()
    out = torch.ldexp(v, torch.tensor(s))
    assert out.dtype == torch.float32 and torch.equal(out.double() * 2.0 ** -s, v.double()), f"2^{s} times the integers is not exact in f32"
    return out


def stored(t, dtype):
    """One rounding to the storage type on the CPU (nearest even; 65520 and above become inf in fp16)."""
    return t.to(L.storage(dtype))


def bits(t):
    """Bit patterns as int64; every NaN is the one pattern -1 and -0 is +0."""
    t = t.detach().cpu().contiguous()
    i = t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).to(torch.int64)
    i = torch.where(t == 0, torch.zeros_like(i), i)
    return torch.where(t.isnan(), torch.full_like(i, -1), i)


def same_bits(got, want, what, nan_allowed=None):
    """(nan_allowed: a mask of elements that may ALSO be NaN -- see ``structural_zero_reach``)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got), bits(want)
    if nan_allowed is not None:
        g = torch.where(nan_allowed & (g == -1), w, g)
    if not torch.equal(g, w):
        ne = g != w
        idx = [tuple(i) for i in ne.nonzero()[:8].tolist()]
        gf, wf = got.detach().cpu().float(), want.float()
        lines = [f"{what}: bit patterns differ on {int(ne.sum())} of {ne.numel()} elements"]
        lines += [f"  {i}: got {float(gf[i])!r} ({int(g[i]):#x}) want {float(wf[i])!r} ({int(w[i]):#x})" for i in idx]
        flushed = bool(((gf == 0) & (wf != 0))[ne].all())
        saturated = bool((gf.isfinite() & ~wf.isfinite())[ne].all())
        lines.append(f"  every differing element is 0 where a non-zero value is expected: {flushed}; finite where inf / NaN is expected: {saturated}")
        pytest.fail("\n".join(lines), pytrace=False)


def to_cl_cpu(t, dtype):
    """NCDHW f32 on the CPU -> channels-last storage type, channels padded with zeros to a multiple of 8, on the CPU."""
    n, c, d, h, w = t.shape
    out = torch.zeros((n, d, h, w, (c + 7) // 8 * 8), dtype=L.storage(dtype))
    out[..., :c] = t.permute(0, 2, 3, 4, 1).to(L.storage(dtype))
    return out


def sources_cl(x, c, dtype):
    """The layer's source tensors on the GPU, cut from the NCDHW f32 CPU tensor of all its input channels."""
    srcs, o = [], 0
    for ch in c["src_c"]:
        srcs.append(to_cl_cpu(x[:, o:o + ch], dtype).cuda())
        o += ch
    return srcs


def from_cl_cpu(t, c):
    """channels-last on the GPU -> the first c channels as NCDHW on the CPU, in the tensor's own type."""
    return t[..., :c].permute(0, 4, 1, 2, 3).contiguous().cpu()


# ---- exponents, chosen from the integer reference alone -----------------------------------------------------------------------
def shares_below_normal(ref, s, dtype):
    """(share of the non-zero outputs that are subnormal in the storage type, share that are normal) at scale 2^s."""
    mag = ref.abs()[ref != 0].double() * 2.0 ** s
    sub = float((mag < 2.0 ** MIN_NORMAL_EXP[dtype]).double().mean())
    return sub, 1.0 - sub


def straddle_shift(ref):
    """fp16: the smallest k >= 0 for which at least 10 % of the non-zero outputs of ``ref * 2^(k - 24)`` are NORMAL.  With
    operands in {-3..3} the results of these layers stay below 1024 quanta at q = 2^-24 (the largest is 746: all subnormal);
    shifted by k <= 8 the 16-bit operand is still subnormal (3 * 2^(k - 24) < 2^-14) while the results lie on both sides of
    2^-14, so the store meets subnormal results, normal results and the boundary between them.  (Integers below 2048 times a
    power of two are fp16 numbers: the rounding itself is the business of tests/conv_layer_cases.py, not of these runs.)"""
    for k in range(0, 9):
        if shares_below_normal(ref, Q_EXP["fp16"] + k, "fp16")[1] >= 0.10:
            return k
    raise AssertionError("no shift up to 8 puts 10 % of the results into fp16's normal range")


def overflow_share(ref, e, extra=None):
    v = scaled(ref, e) if extra is None else scaled(ref, e) + extra
    return float((v.abs() >= FP16_INF_FROM).double().mean())


def top_exponent(ref, prev=None):
    """fp16, top of the range: the largest e <= 14 (3 * 2^14 is representable, so the scaled operand and ``prev`` are) at which
    at most half of the outputs reach 65520 -- with ``prev``, both without it and with it added; the caller asserts that at
    least 1 % do."""
    for e in range(14, -1, -1):
        if overflow_share(ref, e) <= 0.5 and (prev is None or overflow_share(ref, e, scaled(prev, e)) <= 0.5):
            return e
    raise AssertionError("more than half of the outputs overflow without any scaling")


# ---- expectations ---------------------------------------------------------------------------------------------------------------
def expect_forward(dt, s, dtype):
    """Stored forward result with x and the bias times 2^s."""
    return stored(scaled(dt["ref"], s), dtype)


def expect_dgrad(c, dt, s, dtype, accumulate):
    """Stored data gradient with dy (and, for ``+=``, the previous gradient) times 2^s, per destination.  The tiled kernel's
    staged ``+=`` rounds the new value before it adds (``conv_layer_cases.tiled_rounds_before_it_adds``)."""
    new = scaled(dt["ref"], s)
    if accumulate:
        if L.tiled_rounds_before_it_adds(c):
            new = stored(new, dtype).float()
        new = new + scaled(dt["prev"], s)
    return stored(new, dtype)


def plants(c, kind):
    """(sample, channel, z, y, x) of the +inf (sample 0) and of the NaN (sample 1; sample 0 where a weight-gradient shape has
    one sample only): next to faces, so that the tap footprints are clipped, and in channels that exist in every case."""
    n, d, h, w = c["dims"]
    ch = (c["cin"] if kind == "fwd" else c["cout"]) - 1
    return (0, ch, 0, h - 1, 5), (min(1, n - 1), 0, d // 2, 3, w - 1)


def planted(t, c, kind):
    t = t.float().clone()
    p_inf, p_nan = plants(c, kind)
    t[p_inf], t[p_nan] = float("inf"), float("nan")
    return t


def expect_nonfinite(c, dt, kind, dtype, accumulate=False):
    """F.conv3d (or its weight gradient) on the planted f32 operands on the CPU, rounded to the storage type."""
    if "planted_conv" not in dt:              # (once per case: its two storage types and both destination states share it)
        if kind == "fwd":
            dt["planted_conv"] = L.conv_ref(planted(dt["x"], c, kind)[:, :c["cin"]], dt["wt"], dt["b"], c["taps"], c["dilation"])
        else:
            assert kind == "dgrad", kind
            dt["planted_conv"] = L.conv_ref(planted(dt["dy"], c, kind), dt["wt"].transpose(0, 1).flip(2, 3, 4).contiguous(), None,
                                            c["taps"], c["dilation"])
    v = dt["planted_conv"]
    if kind == "dgrad" and accumulate:
        if L.tiled_rounds_before_it_adds(c):
            v = stored(v, dtype).float()
        v = v + dt["prev"].float()
    return stored(v, dtype)


def footprint(c, kind, dt):
    """From integers alone: (where the +inf of sample 0 arrives with a positive weight, with a negative weight, where the NaN
    of sample 1 arrives) as boolean NCDHW masks of the output -- the plant's indicator convolved with the weights."""
    src = dt["x"][:, :c["cin"]] if kind == "fwd" else dt["dy"]
    wt = dt["wt"] if kind == "fwd" else dt["wt"].transpose(0, 1).flip(2, 3, 4).contiguous()
    p_inf, p_nan = plants(c, kind)
    one = torch.zeros(src.shape, dtype=torch.float32)
    one[p_inf] = 1.0
    sign = L.conv_ref(one, wt, None, c["taps"], c["dilation"])
    one.zero_()
    one[p_nan] = 1.0
    reach = L.conv_ref(one, wt.abs(), None, c["taps"], c["dilation"])
    return sign > 0, sign < 0, reach > 0


def structural_zero_reach(c, kind):
    """Output elements at which a kernel form multiplies a plant by a zero that is part of its own K layout.  The streaming
    kernel folds the x-taps of an 8- or 16-channel source into the K = 32 of one MFMA (se-unet-airseg_amd/csrc/conv_stream.hip: 4 slots of 8
    channels or 2 x 2 slots of 16, for at most 16 destination channels); three slots are the taps x-1, x, x+1 and the fourth
    holds ZERO weights and reads voxel x+2.  0 x inf is NaN, so a non-finite voxel also reaches the column two (dilated) voxels
    to its left, over the y and z extent of its footprint, as NaN.  That is the kind of implementation choice the non-zero
    weights keep out of the expectation: nothing is hidden, the step is dropped either way.  These elements may hold the exact
    value or NaN; every other element of every case is held to the bit.  None for every other kernel form."""
    src, dst = (c["src_c"][0], c["cout"]) if kind == "fwd" else (c["cout"], c["src_c"][0])
    if c["fwd" if kind == "fwd" else "dgrad"] != "Stream" or (dst + 7) // 8 * 8 > 16 or not ((src == 8 and c["dilation"] == 1) or src == 16):
        return None
    n, d, h, w = c["dims"]
    dl = c["dilation"]
    m = torch.zeros((n, dst, d, h, w), dtype=torch.bool)
    for (smp, _, z, y, x) in plants(c, kind):
        if x - 2 * dl >= 0:
            m[smp, :, max(z - dl, 0):z + dl + 1, max(y - dl, 0):y + dl + 1, x - 2 * dl] = True
    return m


def wgrad_touched(c, dt):
    """[cout, cin, k, k, k] mask of the weight-gradient entries whose sum contains a planted dy voxel: those of the plant's
    output channel whose tap reads x INSIDE the volume at that voxel."""
    n, d, h, w = c["dims"]
    k = 3 if c["taps"] == 27 else 1
    m = torch.zeros((c["cout"], c["cin"], k, k, k), dtype=torch.bool)
    for (_, co, z, y, x) in plants(c, "wgrad"):
        for kz in range(k):
            for ky in range(k):
                for kx in range(k):
                    off = [(t - k // 2) * c["dilation"] for t in (kz, ky, kx)]
                    if 0 <= z + off[0] < d and 0 <= y + off[1] < h and 0 <= x + off[2] < w:
                        m[co, :, kz, ky, kx] = True
    return m


def wgrad_plant_channels(c):
    return sorted({p[1] for p in plants(c, "wgrad")})


# ---- running a forced kernel ----------------------------------------------------------------------------------------------------
def run_forward(S, c, x_f32, wt, b_f32, dtype):
    srcs = sources_cl(x_f32, c, dtype)
    raw, part, slots = L.run_forward(S, c["fwd"], srcs, wt.cuda(), None if b_f32 is None else b_f32.cuda(), c)
    return from_cl_cpu(raw, c["cout"]), part, slots


def run_dgrad(S, c, dy_f32, wt, prev_f32, dtype, accumulate):
    """Returns the destinations joined along the channel axis (NCDHW, storage type, CPU).  Overwrite runs over a poisoned buffer."""
    dy_cl = to_cl_cpu(dy_f32, dtype).cuda()
    dsts, o = [], 0
    for ch in c["src_c"]:
        if accumulate:
            dsts.append(to_cl_cpu(prev_f32[:, o:o + ch], dtype).cuda())
        else:
            dsts.append(torch.full(tuple(dy_cl.shape[:4]) + (ch,), 7.0, dtype=dy_cl.dtype, device="cuda"))
        o += ch
    L.run_dgrad(S, c["dgrad"], dy_cl, wt.cuda(), c, dsts, [int(accumulate)] * len(dsts))
    return torch.cat([from_cl_cpu(t, ch) for t, ch in zip(dsts, c["src_c"])], 1)


def run_wgrad(S, c, x_f32, dy_f32, dtype):
    srcs = sources_cl(x_f32, c, dtype)
    _, forced = L.run_wgrad(S, c["wgrad"], srcs, to_cl_cpu(dy_f32, dtype).cuda(), c)
    return forced().cpu()
