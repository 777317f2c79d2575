"""The machinery of the per-layer convolution tests: every convolution pass of a plan, at the layer's own shape and on the kernel
the plan routes it to, BITWISE.  ``Config(batch, extent, width)`` holds what ``SE_UNet.conv_plan`` gives for one descriptor
(batch x 2 x extent^3, or batch x 2 x D x H x W for an extent given as a tuple, that channel width) in bf16 and fp16 storage, and
the case lists generated from it; the test modules (tests/test_conv_layers_gpu.py: the benchmarked 4 x 2 x 128^3 at width 1, and
two small plans; tests/test_conv_layers_config4_gpu.py: 160^3 at width 2; tests/test_conv_layers_ragged_gpu.py: non-cubic extents
that leave every tile of the kernel family ragged) parametrise over those lists and call ``forward_case`` / ``dgrad_case`` /
``wgrad_case``, so a layer that is added or re-routed later is covered without editing a test.

Why equality and not a tolerance: the operands are small integers.  With x, w, bias in {-3..3} every product and every partial
sum of a 3x3x3 convolution with up to 256 input channels is an integer of magnitude at most 27 * 256 * 9 + 3 = 62 211 < 2^24,
exact in f32 in ANY summation order -- on the matrix cores and in ``F.conv3d`` on the CPU alike -- and the 16-bit stored value
is that integer rounded once to nearest-even (many outputs exceed 256 and many are exact ties, so the rounding is exercised;
62 211 + 3 for ``+=`` is below fp16's 65 504: no overflow).  For the weight gradient x, dy are in {-1, 0, 1}: every partial
sum is bounded by N * voxels (2^23 at 4 x 128^3, 8 192 000 at 2 x 160^3, both below 2^24).  A plain float32 convolution on the CPU
is therefore an exact reference, and a kernel that drops or doubles one plane at a segment seam, or one patch of a work-item
loop, differs by whole integers.  Only the InstanceNorm statistics carry a tolerance: the fp32 row of tests/test_ops_gpu.py
(mean atol 2e-5, rstd rtol 2e-4), against float64 statistics of the exact integer result.

The reference of a layer is computed once and shared by the two storage types (cases are ordered layer-major; one layer's
tensors are kept at a time)."""
import os

import pytest
import torch
import torch.nn.functional as F

DTYPES = ("bf16", "fp16")


def extents(extent):
    """(D, H, W) of an extent given as one int (a cube) or as a (D, H, W) tuple."""
    d, h, w = (extent,) * 3 if isinstance(extent, int) else extent
    return int(d), int(h), int(w)


def plan_of(dtype, batch, extent, width):
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    from seunet_amd.SE_UNet import conv_plan, make_desc
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return conv_plan(make_desc(batch, 2, 1, *extents(extent), width, _lib.dtype_code(dtype), 0, 0.01))


class Config:
    """The plan of batch x 2 x extent^3 (extent: an int) or batch x 2 x D x H x W (extent: a tuple) at channel width `width` per
    storage type, and the cases generated from it.  `levels` keeps only the layers of those plan levels in LAYERS, CASES and
    DGRAD_CASES (PLANS and ROUTED stay whole: they describe the plan)."""

    def __init__(self, batch, extent, width, dtypes=DTYPES, levels=None):
        self.batch, self.extent, self.width, self.dtypes = batch, extent, width, tuple(dtypes)
        self.levels = None if levels is None else tuple(levels)
        self.key = (batch, extent, width)
        self.PLANS = {dt: {c["name"]: c for c in plan_of(dt, batch, extent, width)} for dt in self.dtypes}
        self.LAYERS = [n for n, c in self.PLANS[self.dtypes[0]].items() if self.levels is None or c["level"] in self.levels]
        # (kernel, pass) pairs the plan routes: a plan that silently routed everything to one kernel would make the cases pass
        # vacuously, so the test modules assert what they expect to find here
        self.ROUTED = {(c[p], p) for dt in self.dtypes for c in self.PLANS[dt].values() for p in ("fwd", "dgrad", "wgrad") if c[p]}
        # (layer, storage type, layout of a two-source layer: "plan" = one allocation, the sources at the byte distance the plan
        # reports, as the network's workspace presents them to the 32-bit buffer descriptor; dc5 also with two separate allocations)
        self.CASES = [(n, dt, lay) for n in self.LAYERS for lay in (("plan", "separate") if n == "dc5" else ("plan",)) for dt in self.dtypes]
        self.DGRAD_CASES = [c for c in self.CASES if self.PLANS[c[1]][c[0]]["need_dgrad"]]

    def passes(self, name, dtype=None):
        c = self.PLANS[dtype or self.dtypes[0]][name]
        return c["fwd"], c["dgrad"], c["wgrad"]


ids = lambda c: "-".join(c) if isinstance(c, tuple) else None


def ops_or_skip():
    """The body of the test modules' module-scoped ``S`` fixture."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib, ops
    _lib.load()
    return ops


def storage(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float16


def ints(shape, lo, hi, seed, device="cuda"):
    """Seeded integers in [lo, hi] as int8 on the GPU (the CPU reference reads a copy of the same values).
    (device="cpu": the CPU generator's draw instead, for data a host test has to see as well -- tests/range_cases.py)"""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=device, dtype=torch.int8)


_cache = {}


def shared(key, make):
    """One entry: the tensors of the layer under test, shared by its bf16 and fp16 cases; dropped when the next layer starts."""
    if key not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        _cache[key] = make()
    return _cache[key]


def place_pair(a, b, dist):
    """Copies of the channels-last tensors a, b inside ONE allocation with b.data_ptr() - a.data_ptr() == dist."""
    na, nb = a.numel() * a.element_size(), b.numel() * b.element_size()
    assert dist % 256 == 0 and (dist >= na or -dist >= nb), (dist, na, nb)
    off_a, off_b = (0, dist) if dist > 0 else (-dist, 0)
    buf = torch.empty(max(off_a + na, off_b + nb), dtype=torch.uint8, device=a.device)
    assert buf.data_ptr() % 256 == 0
    va = buf[off_a:off_a + na].view(a.dtype).view(a.shape)
    vb = buf[off_b:off_b + nb].view(b.dtype).view(b.shape)
    va.copy_(a)
    vb.copy_(b)
    assert vb.data_ptr() - va.data_ptr() == dist
    return va, vb


def sources(S, x_i8, c, dtype, layout):
    """The layer's source tensors (channels-last, storage type) cut from the NCDHW int8 tensor of all its input channels."""
    srcs, o = [], 0
    for ch in c["src_c"]:
        srcs.append(S.to_cl(x_i8[:, o:o + ch].float(), dtype))
        o += ch
    if len(srcs) == 2 and layout == "plan":
        srcs = list(place_pair(srcs[0], srcs[1], c["src_dist"]))
    return srcs


def explain(got, want, axes, samples=None):
    """What differs: count, the first few positions with got / want, and the distinct indices along z and the 4-row y patches
    (a seam bug reads as "planes 64 and 65 of every sample"); for a weight gradient the (co, ci, tap) positions.
    (samples: the sample numbers the rows of got / want stand for, when they are a selection of a larger batch)"""
    ne = got != want
    smp = (lambda i: samples[i]) if samples is not None else (lambda i: i)
    lines = [f"{int(ne.sum())} of {ne.numel()} elements differ"]
    if got.dim() == 5 and axes[0] == "n":
        n0 = int(ne.flatten(1).any(1).nonzero()[0])
        z0 = int(ne[n0].any(dim=0).flatten(1).any(1).nonzero()[0])
        for c, y, x in ne[n0, :, z0].nonzero()[:6].tolist():
            lines.append(f"  (n, c, z, y, x) = ({smp(n0)}, {c}, {z0}, {y}, {x}): got {float(got[n0, c, z0, y, x])} want {float(want[n0, c, z0, y, x])}")
        zs = ne.permute(2, 0, 1, 3, 4).flatten(1).any(1).nonzero().flatten().tolist()
        ys = ne.permute(3, 0, 1, 2, 4).flatten(1).any(1).nonzero().flatten().tolist()
        xs = ne.permute(4, 0, 1, 2, 3).flatten(1).any(1).nonzero().flatten().tolist()
        ns = [smp(i) for i in ne.flatten(1).any(1).nonzero().flatten().tolist()]
        cs = ne.permute(1, 0, 2, 3, 4).flatten(1).any(1).nonzero().flatten().tolist()
        lines += [f"  samples {ns}", f"  channels {cs}", f"  z planes {zs}", f"  y rows {ys} (4-row patches {sorted({y // 4 for y in ys})})",
                  f"  x columns in 32-wide blocks {sorted({x // 32 for x in xs})}"]
    else:
        g, w = got.flatten(2), want.flatten(2)
        for co, ci, t in (g != w).nonzero()[:8].tolist():
            lines.append(f"  (co, ci, tap) = ({co}, {ci}, {t}): got {float(g[co, ci, t])} want {float(w[co, ci, t])}")
        lines.append(f"  taps {sorted(set((g != w).nonzero()[:, 2].tolist()))}")
    return "\n".join(lines)


def assert_same(got, want, what, axes=("n", "c", "z", "y", "x"), samples=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        pytest.fail(f"{what}: not bitwise equal\n{explain(got, want, axes, samples)}", pytrace=False)


def rounded(ref_cpu, dtype):
    """The exact f32 integers rounded once to the storage type (on the CPU), back as f32 on the GPU."""
    return ref_cpu.to(storage(dtype)).cuda().float()


def conv_ref(x, w, b, taps, dil):
    return F.conv3d(x, w, b, padding=dil, dilation=dil) if taps == 27 else F.conv3d(x, w, b)


# ---------------------------------------------------------------------------------------------------
# forward (+ InstanceNorm statistics)
# ---------------------------------------------------------------------------------------------------
def forward_data(c, seed, device="cuda", nonzero_w=False):
    """(nonzero_w: weights of 0 become 1, for operands that hold an infinity -- tests/range_cases.py)"""
    n, d, h, w = c["dims"]
    k = 3 if c["taps"] == 27 else 1
    x = ints((n, sum(c["src_c"]), d, h, w), -3, 3, seed, device)
    x[:, c["cin"]:] = 0                                  # ec1: the logical 2 of the 8 packed channels
    wt = ints((c["cout"], c["cin"], k, k, k), -3, 3, seed + 1, device).float().cpu()
    if nonzero_w:
        wt[wt == 0] = 1.0
    b = ints((c["cout"],), -3, 3, seed + 2, device).float().cpu() if c["taps"] == 27 else None     # (the aggregation convs have no bias)
    ref = conv_ref(x[:, :c["cin"]].cpu().float(), wt, b, c["taps"], c["dilation"])
    mean = torch.stack([r.double().mean(dim=(1, 2, 3)) for r in ref])
    var = torch.stack([r.double().var(dim=(1, 2, 3), unbiased=False) for r in ref])
    return x, wt, b, ref, mean, (var + 1e-5).rsqrt()


def run_forward(S, kernel, srcs, wt, b, c):
    if kernel == "Stream":
        raw, part, slots = S.conv3d_stream(srcs[0], wt, b, c["dilation"], want_stats=True)
    elif kernel == "March":
        (raw,), part, slots = S.conv3d_march(srcs, wt, b, c["dilation"], want_stats=True)
    else:
        assert kernel == "Tiled", kernel
        (raw,), part, slots = S.conv3d(srcs, wt, b, c["dilation"], S._lib.CONV_MFMA, cin=c["cin"], want_stats=True)
    return raw, part, slots


def check_stats(S, part, slots, c, mean64, rstd64, what, rows=None):
    """(rows: the samples mean64 / rstd64 describe, all of them by default)"""
    n, d, h, w = c["dims"]
    mean, rstd = S.stats_finalize(part, slots, d * h * w)
    mean, rstd = mean.cpu().double()[:, :c["cout"]], rstd.cpu().double()[:, :c["cout"]]
    if rows is not None:
        mean, rstd = mean[list(rows)], rstd[list(rows)]
    em = float((mean - mean64).abs().max())
    er = float(((rstd - rstd64).abs() / rstd64).max())
    print(f"{what}: max |mean - float64| = {em:.3e} (|mean| <= {float(mean64.abs().max()):.3e}), max rel rstd error = {er:.3e}")
    assert em <= 2e-5, f"{what}: mean off by {em:.3e} (atol 2e-5)"
    assert er <= 2e-4, f"{what}: rstd off by {er:.3e} relative (rtol 2e-4)"


def forward_case(S, cfg, case):
    name, dtype, layout = case
    c = cfg.PLANS[dtype][name]
    x, wt, b, ref, mean64, rstd64 = shared((cfg.key, "fwd", name), lambda: forward_data(c, 1000 + 10 * cfg.LAYERS.index(name)))
    srcs = sources(S, x, c, dtype, layout)
    raw, part, slots = run_forward(S, c["fwd"], srcs, wt.cuda(), None if b is None else b.cuda(), c)
    what = f"{name} forward on {c['fwd']} ({dtype}, {c['src_c']} -> {c['cout']} channels, dilation {c['dilation']}, {c['dims']})"
    assert_same(S.from_cl(raw, c["cout"]), rounded(ref, dtype), what)
    check_stats(S, part, slots, c, mean64, rstd64, what)


# ---------------------------------------------------------------------------------------------------
# data gradient
# ---------------------------------------------------------------------------------------------------
def dgrad_data(c, seed, device="cuda", nonzero_w=False):
    n, d, h, w = c["dims"]
    k = 3 if c["taps"] == 27 else 1
    cin = sum(c["src_c"])
    dy = ints((n, c["cout"], d, h, w), -3, 3, seed, device)
    wt = ints((c["cout"], cin, k, k, k), -3, 3, seed + 1, device).float().cpu()
    if nonzero_w:
        wt[wt == 0] = 1.0
    # the transposed convolution as a convolution with the transposed, mirrored weight (exact in f32 like the forward)
    ref = conv_ref(dy.cpu().float(), wt.transpose(0, 1).flip(2, 3, 4).contiguous(), None, c["taps"], c["dilation"])
    prev = ints((n, cin, d, h, w), -3, 3, seed + 2, device)
    return dy, wt, ref, prev


def run_dgrad(S, kernel, dy_cl, wt, c, dsts, acc):
    if kernel == "Stream":
        S.conv3d_stream(dy_cl, wt, None, c["dilation"], transpose_flip=True, dst=dsts[0], accumulate=bool(acc[0]))
    elif kernel == "March":
        S.conv3d_march([dy_cl], wt, None, c["dilation"], transpose_flip=True, dsts=dsts, dst_channels=c["src_c"], accumulate=acc)
    else:
        assert kernel == "Tiled", kernel
        S.conv3d([dy_cl], wt, None, c["dilation"], S._lib.CONV_MFMA, transpose_flip=True, dsts=dsts, dst_channels=c["src_c"], accumulate=acc)


def tiled_rounds_before_it_adds(c):
    """conv_igemm.hip, `+=` in 16-bit storage: a launch with a destination wider than 32 bytes per written voxel pitch goes
    through the LDS stage, which holds the new values already rounded, and stores round(round(new) + old) (stated in the
    kernel's comment on its store paths; found by this file: ec7 / ec10 / ec11 / ec12 / dc1 / dc2 in bf16 were one ulp off
    round(new + old) on 3 % of the elements).  Launches whose destinations all have <= 16 channels add in f32 and round once.
    The channel count enters nowhere else: launch_conv sets ``direct`` from ``dst.C[i] * st > 16`` alone, a workgroup always
    stages 32 output columns, and the staged ``+=`` is the same unpack / add / pack per 16-byte piece whatever the
    destination's width -- so the 128-channel destinations of the width-2 plan (ec8, ec9, dc1, dc3, ec63 ...) are described
    by the same predicate."""
    st = c["dilation"] if c["taps"] == 27 else 1
    return c["dgrad"] == "Tiled" and any(ch * st > 16 for ch in c["src_c"])


def dgrad_case(S, cfg, case):
    """Three destination states: overwrite (over a poisoned buffer), += onto an integer-valued previous gradient (expected:
    the exact integer sum plus the old value, rounded ONCE -- on the marching and streaming kernels; the tiled kernel's staged
    store path rounds the new value first, see ``tiled_rounds_before_it_adds``, and the expectation mirrors that), and -- for
    the layers with several sources -- a null first destination (those channels are dropped) next to one that accumulates.
    (Only ec1 meets the network input, and it runs no data gradient at all; the x-branch's gradient does not go through a
    convolution kernel.)"""
    name, dtype, layout = case
    c = cfg.PLANS[dtype][name]
    dy, wt, ref, prev = shared((cfg.key, "dgrad", name), lambda: dgrad_data(c, 2000 + 10 * cfg.LAYERS.index(name)))
    dy_cl = S.to_cl(dy.float(), dtype)
    wt_g = wt.cuda()
    split = c["src_c"]
    offs = [sum(split[:i]) for i in range(len(split))]
    what = f"{name} data gradient on {c['dgrad']} ({dtype}, {c['cout']} -> {split} channels, dilation {c['dilation']}, {c['dims']})"
    states = [("overwrite", [0] * len(split), [False] * len(split)), ("+=", [1] * len(split), [False] * len(split))]
    if len(split) > 1:
        states.append(("null first destination, += second", [0, 1, 0][:len(split)], [True] + [False] * (len(split) - 1)))
    for label, acc, null in states:
        dsts = []
        for o, ch, a, dropped in zip(offs, split, acc, null):
            if dropped:
                dsts.append(None)
            elif a:
                dsts.append(S.to_cl(prev[:, o:o + ch].float(), dtype))
            else:
                dsts.append(torch.full(tuple(dy_cl.shape[:4]) + (ch,), 7.0, dtype=dy_cl.dtype, device="cuda"))
        if len(dsts) == 2 and layout == "plan" and not any(null):
            dsts = list(place_pair(dsts[0], dsts[1], c["src_dist"]))
        run_dgrad(S, c["dgrad"], dy_cl, wt_g, c, dsts, acc)
        for i, (o, ch, a) in enumerate(zip(offs, split, acc)):
            if dsts[i] is None:
                continue
            want = ref[:, o:o + ch]
            if a:
                new = want.to(storage(dtype)).float() if tiled_rounds_before_it_adds(c) else want
                want = new + prev[:, o:o + ch].cpu().float()
            assert_same(S.from_cl(dsts[i]), rounded(want, dtype), f"{what}, {label}, destination {i}")
        del dsts


# ---------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------
def wgrad_data(c, seed, device="cuda"):
    n, d, h, w = c["dims"]
    k = 3 if c["taps"] == 27 else 1
    x = ints((n, sum(c["src_c"]), d, h, w), -1, 1, seed, device)
    x[:, c["cin"]:] = 0
    dy = ints((n, c["cout"], d, h, w), -1, 1, seed + 1, device)
    pad = c["dilation"] if k == 3 else 0
    ref = torch.nn.grad.conv3d_weight(x[:, :c["cin"]].cpu().float(), (c["cout"], c["cin"], k, k, k), dy.cpu().float(),
                                      padding=pad, dilation=c["dilation"] if k == 3 else 1)
    return x, dy, ref


def run_wgrad(S, kernel, srcs, dy_cl, c):
    """(the routed call, the call that forces the kernel the plan names)"""
    L = S._lib
    if kernel == "Stream":                       # routed by Plan::route itself, ahead of wgrad_kernel
        f = lambda: S.conv3d_wgrad_stream(srcs[0], dy_cl, c["cin"], c["cout"], c["dilation"])
        return f, f
    forced = {"March": L.CONV_MARCH, "Wgrad1x1": L.CONV_MARCH, "Tiled": L.CONV_TILED}[kernel]
    call = lambda impl: S.conv3d_wgrad(srcs, dy_cl, c["cin"], c["cout"], c["taps"], c["dilation"], impl)
    return (lambda: call(L.CONV_MFMA)), (lambda: call(forced))


def check_wgrad(S, c, srcs, dy_cl, ref, what):
    routed, forced = run_wgrad(S, c["wgrad"], srcs, dy_cl, c)
    dw = routed()
    assert_same(dw.cpu(), ref, what, axes=("co", "ci", "tap"))
    assert_same(forced(), dw, what + ": the kernel the plan names, forced, against the routed call", axes=("co", "ci", "tap"))
    assert_same(routed(), dw, what + ": second run against the first", axes=("co", "ci", "tap"))
    if c["wgrad"] == "Stream":                   # what seunet_conv3d_wgrad picks for the same operands must be exact as well
        other = S.conv3d_wgrad(srcs, dy_cl, c["cin"], c["cout"], c["taps"], c["dilation"], S._lib.CONV_MFMA)
        assert_same(other.cpu(), ref, what + ": seunet_conv3d_wgrad's own choice", axes=("co", "ci", "tap"))


def wgrad_case(S, cfg, case):
    name, dtype, layout = case
    c = cfg.PLANS[dtype][name]
    x, dy, ref = shared((cfg.key, "wgrad", name), lambda: wgrad_data(c, 3000 + 10 * cfg.LAYERS.index(name)))
    srcs = sources(S, x, c, dtype, layout)
    what = f"{name} weight gradient on {c['wgrad']} ({dtype}, {c['src_c']} x {c['cout']} channels, dilation {c['dilation']}, {c['dims']})"
    check_wgrad(S, c, srcs, S.to_cl(dy.float(), dtype), ref, what)


# ---------------------------------------------------------------------------------------------------
# forward of a large-batch plan, a few samples checked
# ---------------------------------------------------------------------------------------------------
def forward_samples_case(S, cfg, name, dtype, samples):
    """The forward of a two-source layer at cfg's batch and the plan's source distance, compared for `samples` only.  Samples
    are independent, so the reference is computed for those alone: they hold distinct random integers, every other sample holds
    a copy of one further draw (a sample mix-up or an offset that wraps lands in different values).  The first of those other
    samples is compared with the reference as well, and the rest bitwise with it on the GPU, so that a wrap which lands in
    them alone is seen too."""
    c = cfg.PLANS[dtype][name]
    n, d, h, w = c["dims"]
    assert len(c["src_c"]) == 2 and max(samples) < n and len(set(samples)) == len(samples), (c, samples)
    few = dict(c, dims=(len(samples) + 1, d, h, w))
    x, wt, b, ref, mean64, rstd64 = shared((cfg.key, "fwd", name), lambda: forward_data(few, 1000 + 10 * cfg.LAYERS.index(name)))
    row = [len(samples)] * n
    for r, smp in enumerate(samples):
        row[smp] = r
    srcs, o = [], 0
    for ch in c["src_c"]:
        cl = S.to_cl(x[:, o:o + ch].float(), dtype)
        srcs.append(cl[torch.tensor(row, device=cl.device)].contiguous())
        o += ch
    srcs = list(place_pair(srcs[0], srcs[1], c["src_dist"]))
    raw, part, slots = run_forward(S, c["fwd"], srcs, wt.cuda(), None if b is None else b.cuda(), c)
    what = (f"{name} forward on {c['fwd']} ({dtype}, {c['src_c']} -> {c['cout']} channels, {c['dims']}, sources {c['src_dist']} bytes "
            f"apart, samples {list(samples)})")
    others = [i for i in range(n) if i not in samples]
    seen = list(samples) + others[:1]              # (row r of the reference is sample seen[r])
    got = S.from_cl(raw[torch.tensor(seen, device=raw.device)].contiguous(), c["cout"])
    assert_same(got, rounded(ref[:len(seen)], dtype), what, samples=seen)
    for i in others[1:]:
        assert torch.equal(raw[i], raw[others[0]]), f"{what}: samples {i} and {others[0]} hold the same input and differ"
    check_stats(S, part, slots, c, mean64[:len(samples)], rstd64[:len(samples)], what, rows=samples)
