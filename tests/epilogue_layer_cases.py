"""The machinery of the per-layer epilogue tests: every epilogue, pooling, up-sampling and head pass of a training step, at the
shape and storage type a configuration runs it with, against a float64 restatement (tests/epilogue_ref.py) under DERIVED bounds
-- and bitwise wherever the operation only selects or rounds once.

``Config(batch, extent, width, levels=None, dtypes=None)`` generates the cases from ``SE_UNet.conv_plan`` for batch x 2 x
extent^3 (an int) or batch x 2 x D x H x W (a tuple) at that channel width and from the module's own blocks (one or two gates,
head and head slot, the block a max-pool follows), so a block that is added later is covered without editing a test; the test
modules (tests/test_epilogue_layers_gpu.py: the benchmarked 4 x 2 x 128^3 at width 1; tests/test_epilogue_layers_config4_gpu.py:
2 x 2 x 160^3 at width 2; tests/test_epilogue_layers_ragged_gpu.py: the non-cubic configurations of
tests/epilogue_ragged_cases.py) parametrise over its lists and call the case functions below.  Inputs are seeded, already
rounded to the storage type, with a per-(sample, channel) offset and scale (a lane-group or sample mix-up changes the answer); the parameters are the module's seeded initial values, level gradients / head
weights / DropLayer scales random f32.  One block's tensors live at a time.

Tolerances (u = 2^-24; the counts are justified in tests/epilogue_ref.py and next to each use):
  bitwise        pooled values, arg-max words, the fused-pool block's ``out`` against the unfused kernel, max-pool forward and
                 backward (``+=`` rounds once), the two ways of finalising pass A against each other
  1 ulp of f32   statistics whose sums are f64 (plus the float64 summation term, which is ~1e-10 of it)
  element bound  |got - ref| <= 0.5 ulp_T(|ref| + K u A) + K u A
  sum bound      |got - ref| <= (L + K) u S
None is a fraction of max|ref| except the x-branch weight gradient in fp32 storage, which keeps its existing 2e-6 bar.  Every K
and L is a function of the channel count (lg = log2(C / 8)), of the slot count and of the extents: nothing is specific to one
configuration."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_ref as R  # noqa: E402
from conv_layer_cases import _cache, extents, ops_or_skip, shared  # noqa: E402,F401  (one cache: a module's tensors go when the next starts)

# eps and the LeakyReLU slope reach the kernels as C floats: the reference takes the same two numbers
EPS, SLOPE = float(torch.tensor(1e-5, dtype=torch.float32)), float(torch.tensor(0.01, dtype=torch.float32))
U = R.U


def slots_of(dims):
    from seunet_amd import _lib
    return _lib.load().seunet_epilogue_slots(_lib.Dims(*dims))


NONPOW2 = [("np2-32", 32, (3, 6, 10, 14)), ("np2-16", 16, (3, 12, 20, 24)), ("np2-64", 64, (3, 40, 48, 56))]


class Config:
    """The plan of batch x 2 x extent^3 (extent: an int) or batch x 2 x D x H x W (extent: a tuple) at channel width `width`, the
    module with its seeded initial parameters, the slot count of every level, what each block is, and the case lists.  `levels`
    keeps only the cases whose tensor lives on one of those plan levels (a block's own level; the level an up-sampling reads and
    a max-pool reads -- for the packed input of POOLS_X that is the level above the block's); `dtypes` keeps only those storage
    types.  PLAN, BLOCKS and SLOTS stay whole: they describe the plan."""

    def __init__(self, batch, extent, width, levels=None, dtypes=None):
        import seunet_amd  # noqa: F401
        from seunet_amd import _lib
        from seunet_amd.SE_UNet import SE_UNet, conv_plan, make_desc
        if not os.path.exists(_lib.LIB_PATH):
            import __graft_entry__
            __graft_entry__.build()
        self.batch, self.extent, self.width = batch, extents(extent), width
        self.levels = None if levels is None else tuple(levels)
        self.dtypes = None if dtypes is None else tuple(dtypes)
        self.key = (batch, extent, width)
        self.PLAN_LIST = conv_plan(make_desc(batch, 2, 1, *self.extent, width, _lib.BF16, 0, SLOPE))
        with torch.random.fork_rng(devices=[]):      # seeded initial values without touching the session's generator
            torch.default_generator.manual_seed(1234)     # (the CPU generator only: parameters are drawn on the CPU)
            self.NET = SE_UNet(2, 1, width_mult=width, act_dtype="bf16", negative_slope=SLOPE)
        self.SLOTS = {c["level"]: slots_of(c["dims"]) for c in self.PLAN_LIST}
        self.PLAN = {c["name"]: c for c in self.PLAN_LIST}
        self.BLOCKS = B = self._blocks()
        on = lambda level: self.levels is None or level in self.levels
        dts = lambda level=0: tuple(dt for dt in dtypes_for(level) if self.dtypes is None or dt in self.dtypes)
        self.GATED = [n for n, b in B.items() if b["gated"] and on(b["level"])]
        self.AGG = [n for n, b in B.items() if not b["gated"] and on(b["level"])]
        self.AGG_X = [n for n in self.AGG if B[n]["xr"]]
        self.AGG_1 = [n for n in self.AGG if not B[n]["xr"]]
        self.max_C = max(b["C"] for b in B.values())
        self.UPS = [(n, B[b["up_from"]]["C"], B[b["up_from"]]["dims"]) for n, b in B.items() if b["up_from"] and on(b["level"] + 1)]
        self.POOLS = [(n, B[n]["C"], B[n]["dims"]) for n in self.AGG_X]                            # pool0 / pool1 / pool2
        self.POOLS_X = [(self.PLAN[n]["x_name"], 8, self.PLAN_LIST[[c["level"] for c in self.PLAN_LIST].index(B[n]["level"] - 1)]["dims"])
                        for n, b in B.items() if not b["gated"] and b["xr"] and b["level"] >= 1 and on(b["level"] - 1)]   # pool0x / pool1x: the packed input
        self.GATE_CASES = [(n, dt) for n in self.GATED for dt in dts(B[n]["level"])]
        self.X_CASES = [(n, dt, kind) for n in self.AGG_X for dt in dts(B[n]["level"]) for kind in ("random", "ties")]
        self.AGG1_CASES = [(n, dt) for n in self.AGG_1 for dt in dts(B[n]["level"])]
        self.POOL_FWD_CASES = [(n, c, dims, dt) for n, c, dims in self.POOLS + self.POOLS_X for dt in dts()]
        self.POOL_BWD_CASES = [(n, c, dims, dt, acc) for n, c, dims in self.POOLS for dt in dts() for acc in (0, 1)]
        self.UP_CASES = [(n, c, dims, dt) for n, c, dims in self.UPS for dt in dts()]
        self.UP_BWD_CASES = [c + (acc,) for c in self.UP_CASES for acc in (0, 1)]

    def _blocks(self):
        """Per block of the plan: kind, gates, head, head slot, whether it is the first of its (head, level) to write the level
        map, the pool-fused form, the up-sampling in front of it."""
        NET, PLAN_LIST = self.NET, self.PLAN_LIST
        info, seen = {}, set()
        gated_order = [n for n, m in NET.named_children() if hasattr(m, "conv_se")]      # registration order = head channel order
        for i, c in enumerate(PLAN_LIST):
            mod = getattr(NET, c["name"])
            b = {"gated": hasattr(mod, "conv_se"), "level": c["level"], "C": c["cout"], "dims": c["dims"]}
            if b["gated"]:
                b["gates"] = mod.n_gates
                b["head"] = 0 if c["name"].startswith("ec") else 1
                b["slot"] = [n for n in gated_order if n.startswith("ec" if b["head"] == 0 else "dc")].index(c["name"])
                b["first"] = (b["head"], c["level"]) not in seen
                seen.add((b["head"], c["level"]))
            else:
                b["xr"] = c["x_name"] is not None and not c["x_materialised"]
                b["pool"] = i + 1 < len(PLAN_LIST) and PLAN_LIST[i + 1]["level"] == c["level"] + 1
            b["up_from"] = PLAN_LIST[i - 1]["name"] if i > 0 and PLAN_LIST[i - 1]["level"] == c["level"] + 1 else None
            info[c["name"]] = b
        return info


def dtypes_for(level):
    """bf16 and fp16 everywhere; fp32 storage for the (small) blocks of levels 2 and 3."""
    return ("bf16", "fp16") + (("fp32",) if level >= 2 else ())


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def seed_of(*parts):
    return sum((i + 1) * 7919 * sum(map(ord, str(p))) for i, p in enumerate(parts)) % (2 ** 31)


def act(shape, dtype, g, centre=0.6, spread=1.0):
    """[N, D, H, W, C] in the storage type: unit noise with a per-(sample, channel) scale in [0.5, 2) and an offset that differs
    between channels and samples (not centred)."""
    n, c = shape[0], shape[-1]
    scale = 0.5 + 1.5 * torch.rand((n, 1, 1, 1, c), generator=g, device="cuda")
    off = centre * (2 * torch.rand((n, 1, 1, 1, c), generator=g, device="cuda") - 1) + 0.25 * centre
    t = torch.randn(shape, generator=g, device="cuda")
    return (t * scale * spread + off).to(R.storage(dtype))


def levels(shape, dtype, g, count):
    """Values drawn from `count` levels per channel (many equal values: the tie case)."""
    n, c = shape[0], shape[-1]
    lv = torch.randint(0, count, shape, generator=g, device="cuda").float()
    scale = 0.5 + torch.rand((n, 1, 1, 1, c), generator=g, device="cuda")
    return ((lv - 0.4 * count) * scale).to(R.storage(dtype))


def f64(t):
    return t.detach().double().cuda()


GRAD_CLIP = 0.9375          # 15/16: times 2^16 it is 61440, below fp16's 65504


def scale_grad(t, grad_scale, clip=GRAD_CLIP):
    """An incoming gradient for the number-range tests (tests/test_epilogue_range_gpu.py): rounded to multiples of 2^-4, then
    times ``grad_scale``, an exact power of two, in the tensor's own type.  With 2^-20 the values are multiples of 2^-24 below
    2^-14: exact fp16 subnormals, which the assert states.  With a scale of 1 and above (the overflow-on-store runs) a 16-bit
    gradient is first clamped to +-clip, so that it stays finite up to 2^16 (clip = 15/16) while the pass's results cross
    65520: with the Gaussian tails of ``act`` no power of two does both.  (The gated blocks attenuate g_e -- two sigmoid gates --
    so their runs clamp it to 2^-10 and let the f32 level gradient, which is not clamped, carry draw across 65520 at up to 2^25.)  None leaves the tensor as it is."""
    if grad_scale is None:
        return t
    q = (t.float() * 16).round() / 16
    if grad_scale >= 1 and t.element_size() == 2:
        q = q.clamp(-clip, clip)
    out = (q * grad_scale).to(t.dtype)
    assert bool(out.isfinite().all()) and torch.equal(out.double(), q.double() * grad_scale), "the scaled gradient is not exact in its type"
    if grad_scale == 2.0 ** -20:
        assert float(q.abs().max()) < 64 and float(out.abs().max()) < 2.0 ** -14 and bool((out != 0).any())
    return out


def report(got, ref, bound, what):
    """Asserts |got - ref| <= bound element by element and prints the largest error / bound ratio.  The comparison is written
    so that a NaN (or an infinity) the kernel left anywhere fails it: NaN <= bound is false."""
    err = (got.double() - ref).abs()
    bound = bound.expand_as(err) if isinstance(bound, torch.Tensor) else torch.full_like(err, bound)
    bad = ~(err <= bound)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    ratio = float(torch.where(ratio.isnan(), torch.full_like(ratio, float("inf")), ratio).max())
    print(f"  {what}: max err / bound = {ratio:.3g}")
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        lines = [f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound or not finite (worst err / bound {ratio:.3g})"]
        for i in idx:
            i = tuple(i)
            lines.append(f"  {i}: got {float(got[i]):.9g} want {float(ref[i]):.9g} bound {float(bound[i]):.3g}")
        pytest.fail("\n".join(lines), pytrace=False)


def same(got, want, what):
    if not torch.equal(got, want):
        ne = got != want
        idx = [tuple(i) for i in ne.nonzero()[:6].tolist()]
        pytest.fail(f"{what}: not bitwise equal, {int(ne.sum())} of {ne.numel()} differ; first at "
                    + ", ".join(f"{i}: got {float(got[i])} want {float(want[i])}" for i in idx), pytrace=False)


def thread_chain(dims, C):
    """Voxels one thread of pass A sums: ceil(V / (slots x voxels per block)), 256 threads, C / 8 lanes per voxel."""
    V = dims[1] * dims[2] * dims[3]
    return -(-V // (slots_of(dims) * (256 // (C // 8))))


def stat_tol(ref_mean, ref_rstd, x, eps):
    """1 ulp of f32 at the float64 value, plus what a float64 sum of V terms can be off by (V 2^-53 of the magnitudes; for
    rstd through var = E[x^2] - mean^2: d rstd = rstd^3 / 2 d var)."""
    V = x.shape[0]
    f = V * 2.0 ** -53
    m_abs, m2 = x.abs().mean(0), (x * x).mean(0)
    return (R.ulp32(ref_mean) + f * m_abs,
            R.ulp32(ref_rstd) + 0.5 * ref_rstd ** 3 * f * (m2 + 2 * ref_mean.abs() * m_abs))


def check_stats(S, t, what):
    n, d, h, w, c = t.shape
    part, slots = S.channel_stats(t)
    mean, rstd = S.stats_finalize(part, slots, d * h * w, EPS)
    for i in range(n):
        x = t[i].double().reshape(-1, c)
        rm, rr = R.stats(x, EPS)
        tm, tr = stat_tol(rm, rr, x, EPS)
        report(mean[i], rm, tm, f"{what} mean[{i}]")
        report(rstd[i], rr, tr, f"{what} rstd[{i}]")
    return mean, rstd


# ---- gated blocks -----------------------------------------------------------------------------------------------------------
ids = lambda c: "-".join("x".join(map(str, e)) if isinstance(e, tuple) else str(e) for e in c) if isinstance(c, tuple) else None


def gate_params(cfg, name):
    mod, b = getattr(cfg.NET, name), cfg.BLOCKS[name]
    C = b["C"]
    p = {"w_se": mod.conv_se.weight.detach().reshape(C).cuda(),
         "w_se2": mod.conv_se2.weight.detach().reshape(C).cuda() if b["gates"] == 2 else None,
         "w_side": mod.conv2.weight.detach().reshape(2, C).cuda(), "b_side": mod.conv2.bias.detach().cuda()}
    g = gen(seed_of(name, "head"))
    nch = 24 if b["head"] == 0 else 12
    p["head_w_all"] = torch.randn(nch, generator=g, device="cuda")
    # DropLayer scales: 0 for a dropped channel, channel_num / kept otherwise; one row per sample
    keep = (torch.rand((cfg.batch, nch), generator=g, device="cuda") >= 0.3).float()
    p["drop_all"] = keep * nch / (keep.sum() + 0.01)
    p["nch"], p["slot"] = nch, b["slot"]
    return p


def gate_block(S, cfg, name, dtype):
    def make():
        b = cfg.BLOCKS[name]
        n, d, h, w = b["dims"]
        g = gen(seed_of(name, dtype))
        raw = act((n, d, h, w, b["C"]), dtype, g, centre=0.8)
        mean, rstd = check_stats(S, raw, f"{name} {dtype}")
        return {"raw": raw, "mean": mean, "rstd": rstd, "p": gate_params(cfg, name), "g": g}
    return shared((cfg.key, "gate", name, dtype), make)


def gate_stats_and_forward(S, cfg, case):
    """channel_stats + finalize; gate_epilogue_fwd with the level map written or accumulated as the network does for this
    block, with and without DropLayer scales."""
    name, dtype = case
    b, t = cfg.BLOCKS[name], gate_block(S, cfg, name, dtype)
    p, raw = t["p"], t["raw"]
    n, d, h, w = b["dims"]
    C, V, lgl = b["C"], d * h * w, R.lg_lanes(b["C"])
    sl = slice(2 * p["slot"], 2 * p["slot"] + 2)
    head_w, drop = p["head_w_all"][sl].contiguous(), p["drop_all"][:, sl]
    prev = torch.randn((n, d, h, w), generator=t["g"], device="cuda")
    maps = {}
    for with_drop in (True, False):
        # (a block that WRITES the map must not read it: NaN there would survive)
        lm = torch.full_like(prev, float("nan")) if b["first"] else prev.clone()
        e, _ = S.gate_epilogue_fwd(raw, t["mean"], t["rstd"], p["w_se"], p["w_se2"], p["w_side"], p["b_side"], SLOPE, level_map=lm,
                                   level_accumulate=0 if b["first"] else 1, head_w=head_w, drop=drop if with_drop else None,
                                   drop_stride=p["nch"], want_side=False)
        maps[with_drop] = lm
    w2 = None if p["w_se2"] is None else f64(p["w_se2"])
    for i in range(n):
        fw = R.gate_forward(raw[i].double().reshape(V, C), f64(t["mean"][i]), f64(t["rstd"][i]), f64(p["w_se"]), w2,
                            f64(p["w_side"]), f64(p["b_side"]), SLOPE)
        # e: KE roundings relative to |e| F (tests/epilogue_ref.py)
        report(e[i].reshape(V, C), fw["e"], R.element_bound(fw["e"], fw["e"].abs() * fw["F"][:, None], R.KE(C), dtype), f"{name} {dtype} e[{i}]")
        for with_drop in (True, False):
            hw = f64(head_w) * (f64(drop[i]) if with_drop else 1.0)
            ref = hw[0] * fw["side"][:, 0] + hw[1] * fw["side"][:, 1]
            S_ = hw[0].abs() * fw["side_abs"][:, 0] + hw[1].abs() * fw["side_abs"][:, 1]
            if not b["first"]:
                ref, S_ = ref + prev[i].double().reshape(V), S_ + prev[i].double().reshape(V).abs()
            # chain: 7 + lg additions of the channel dot product, + bias; per term: e (KE), w e, head_w drop, hw side, the sum of
            # the two side channels, the accumulation
            report(maps[with_drop][i].reshape(V), ref, R.sum_bound(S_, 8 + lgl, R.KE(C) + 5), f"{name} {dtype} level map[{i}] drop={with_drop}")


def gate_backward(S, cfg, case, grad_scale=None, store_check=None, grad_clip=GRAD_CLIP):
    """The form training runs: sse_bwd_kernel<.., LEVEL = true> with g_e and g_level (level 0: laid out as the logit gradient
    (N, 1, D, H, W)), finalised by seunet_gate_bwd_finalize as the network does -- and by stats_finalize + pgrad_reduce, which
    share the device code and must give the same bits."""
    name, dtype = case
    b, t = cfg.BLOCKS[name], gate_block(S, cfg, name, dtype)
    p, raw = t["p"], t["raw"]
    n, d, h, w = b["dims"]
    C, V, lv = b["C"], d * h * w, b["level"]
    sl = slice(2 * p["slot"], 2 * p["slot"] + 2)
    head_w, drop = p["head_w_all"][sl].contiguous(), p["drop_all"][:, sl]
    g = gen(seed_of(name, dtype, "bwd"))
    g_e = act((n, d, h, w, C), dtype, g, centre=0.2)
    gl = torch.randn((n, 1, d, h, w), generator=g, device="cuda") * 0.5 + 0.1
    g_e, gl = scale_grad(g_e, grad_scale, grad_clip), scale_grad(gl, grad_scale)
    args = (raw, t["mean"], t["rstd"], p["w_se"], p["w_se2"], p["w_side"], p["b_side"], SLOPE)
    kw = dict(g_e=g_e, g_level=gl, head_w=head_w, drop=drop, drop_stride=p["nch"])
    out = S.gate_epilogue_bwd(*args, **kw, fused_finalize=True)
    split = S.gate_epilogue_bwd(*args, **kw, fused_finalize=False)
    for k in out:
        same(out[k].float(), split[k].float(), f"{name} {dtype} {k}: fused finaliser vs stats_finalize + pgrad_reduce")
    w2 = None if p["w_se2"] is None else f64(p["w_se2"])
    T = thread_chain(b["dims"], C)
    # f32 chains.  statistics: the thread's T voxels in 16-bit storage, 8 staged voxels in f32 storage, then f64.  parameter
    # records: T voxels, the strided shuffle sum (<= 6), 3 cross-wave additions, the cast of the f64 record sum; dhead_w also
    # the 8-channel chain and the 6-step lane sum of its per-thread value
    L_stat = (8 if dtype == "fp32" else T) + 1
    L_par = T + 6 + 3 + 1 + 8 + 6
    KD = R.K_DXH(C)
    tot, tot_abs = {}, {}
    for i in range(n):
        fw = R.gate_forward(raw[i].double().reshape(V, C), f64(t["mean"][i]), f64(t["rstd"][i]), f64(p["w_se"]), w2,
                            f64(p["w_side"]), f64(p["b_side"]), SLOPE)
        dr = f64(drop[i])
        bw = R.gate_backward(fw, g_e[i].double().reshape(V, C), gl[i].double().reshape(V), f64(head_w) * dr, dr, f64(p["w_se"]), w2,
                             f64(p["w_side"]), f64(p["b_side"]), SLOPE)
        ab = bw["abs"]
        report(out["m1"][i], bw["sum_dxh"] / V, R.sum_bound(ab["sum_dxh"] / V, L_stat, KD), f"{name} {dtype} m1[{i}]")
        report(out["m2"][i], bw["sum_dxh_xh"] / V, R.sum_bound(ab["sum_dxh_xh"] / V, L_stat, KD + 3), f"{name} {dtype} m2[{i}]")
        # draw from the kernel's own m1, m2 (checked above), as it is from the kernel's mean and rstd: K_DXH + 6 roundings
        m1, m2, rs = f64(out["m1"][i]), f64(out["m2"][i]), f64(t["rstd"][i])
        ref = R.in_backward(bw["dxh"], fw["xh"], rs, m1, m2)
        A = rs * (ab["dxh"] + m1.abs() + (fw["xh"] * m2).abs())
        (store_check or report)(out["draw"][i].reshape(V, C), ref, R.element_bound(ref, A, KD + 6, dtype), f"{name} {dtype} draw[{i}]")
        for k in ("dw_se", "dw_se2", "dw_side", "db_side", "dhead_w"):
            tot[k] = tot.get(k, 0) + bw[k]
            tot_abs[k] = tot_abs.get(k, 0) + ab[k]
        del fw, bw, ab, ref, A
    for k in tot:
        report(out[k], tot[k].reshape(-1), R.sum_bound(tot_abs[k].reshape(-1), L_par, KD + 3), f"{name} {dtype} {k}")


# ---- aggregation blocks -----------------------------------------------------------------------------------------------------
# extents that are not powers of two and differ per axis; the same for every configuration (the benchmark module runs them)
NONPOW2_CASES = [(n, dt, kind) for n, _, _ in NONPOW2 for dt in ("bf16", "fp16", "fp32") for kind in ("random", "ties")]


def x_case_shape(cfg, name):
    for n, C, dims in NONPOW2:
        if n == name:
            w2 = torch.randn((C, 2), generator=torch.Generator().manual_seed(C)) * 0.7
            return C, dims, None, w2.cuda()
    b = cfg.BLOCKS[name]
    return b["C"], b["dims"], b["level"], getattr(cfg.NET, cfg.PLAN[name]["x_name"]).conv1.weight.detach().reshape(b["C"], 2).cuda()


def x_block(S, cfg, name, dtype, kind):
    def make():
        C, (n, d, h, w), _, w2 = x_case_shape(cfg, name)
        seed = seed_of(name, dtype, kind)
        for attempt in range(16):
            g = gen(seed)
            x_in = torch.zeros((n, d, h, w, 8), dtype=R.storage(dtype), device="cuda")
            if kind == "ties":       # raw from 4 levels, each input channel from 2: many windows hold their maximum twice
                raw = levels((n, d, h, w, C), dtype, g, 4)
                x_in[..., :2] = levels((n, d, h, w, 2), dtype, g, 2)
            else:
                raw = act((n, d, h, w, C), dtype, g, centre=0.8)
                x_in[..., :2] = act((n, d, h, w, 2), dtype, g, centre=0.5)
            mean2, rstd2, mom = S.xbranch_stats(x_in, w2, 2, EPS)
            if kind == "random":
                break
            # few input levels: a flagged value would flag a whole level at once.  The seed is chosen so that none is (the
            # reference alone decides); the tie case then goes through the pooled backward with nothing excluded.
            fl = 0
            for i in range(n):
                r2, r2a = R.xbranch(x_in[i, ..., :2].double().reshape(-1, 2), f64(w2))
                fl += int(((r2 - f64(mean2[i])).abs() <= 4 * U * r2a).sum())
            if fl == 0:
                break
            seed += 1
        else:
            pytest.fail(f"{name} {dtype} ties: 16 seeds in a row leave x-branch signs undecided ({fl} elements with the last one)",
                        pytrace=False)
        mean, rstd = check_stats(S, raw, f"{name} {dtype} {kind}")
        return {"raw": raw, "x_in": x_in, "w2": w2, "mean": mean, "rstd": rstd, "mean2": mean2, "rstd2": rstd2, "mom": mom, "g": g}
    return shared((cfg.key, "x", name, dtype, kind), make)


def aggregation_x_pool_forward_and_backward(S, cfg, case, grad_scale=None, store_check=None):
    """The encoder aggregation block as the network runs it: x-branch statistics from the input's moments, the kernel that also
    writes the pooled tensor and the arg-max words, and both backward passes with the pooled gradient added on the fly.  The
    cases named np2-* have extents that are not powers of two and differ per axis (the multiply-high divisions of the routing)."""
    name, dtype, kind = case
    t = x_block(S, cfg, name, dtype, kind)
    C, (n, d, h, w), lv, w2 = x_case_shape(cfg, name)
    V, Vo = d * h * w, d * h * w // 8
    raw, x_in = t["raw"], t["x_in"]
    w2d = f64(w2)
    # x-branch statistics: 1 ulp of f32 at the float64 statistics of w2 . x formed in float64
    for i in range(n):
        r2, _ = R.xbranch(x_in[i, ..., :2].double().reshape(V, 2), w2d)
        rm, rr = R.stats(r2, EPS)
        tm, tr = stat_tol(rm, rr, r2, EPS)
        report(t["mean2"][i], rm, tm, f"{name} {dtype} mean2[{i}]")
        report(t["rstd2"][i], rr, tr, f"{name} {dtype} rstd2[{i}]")
    plain = S.cat_epilogue_fwd_x(raw, t["mean"], t["rstd"], x_in, w2, 2, t["mean2"], t["rstd2"], SLOPE)
    out, pooled, words = S.cat_epilogue_fwd_x_pool(raw, t["mean"], t["rstd"], x_in, w2, 2, t["mean2"], t["rstd2"], SLOPE)
    same(out.float(), plain.float(), f"{name} {dtype} {kind}: out of the pool-fused kernel vs cat_epilogue_fwd_x")
    same(S.maxpool_fwd(out).float(), pooled.float(), f"{name} {dtype} {kind}: maxpool_fwd(out) vs the fused kernel's pooled tensor")
    assert int((words >> 24).abs().max()) == 0, "bits 24-31 of an arg-max word are not zero"
    g = gen(seed_of(name, dtype, kind, "bwd"))
    g_out = act((n, d, h, w, C), dtype, g, centre=0.2)
    g_pool = act((n, d // 2, h // 2, w // 2, C), dtype, g, centre=0.2)
    g_out, g_pool = scale_grad(g_out, grad_scale), scale_grad(g_pool, grad_scale)
    res = S.cat_epilogue_bwd_x(g_out, raw, t["mean"], t["rstd"], x_in, w2, 2, t["mean2"], t["rstd2"], t["mom"], SLOPE, EPS,
                               pool_argmax=words, pool_g=g_pool)
    T = thread_chain((n, d, h, w), C)
    L = 0 if dtype == "fp32" else T      # (f32 storage: the thread sums are f64)
    tied_n = flagged_n = 0
    dw_ref, dw_tol = torch.zeros((C, 2), dtype=torch.float64, device="cuda"), torch.zeros((C, 2), dtype=torch.float64, device="cuda")
    for i in range(n):
        xi = x_in[i, ..., :2].double().reshape(V, 2)
        fw = R.cat_forward(raw[i].double().reshape(V, C), f64(t["mean"][i]), f64(t["rstd"][i]), xi, w2d, f64(t["mean2"][i]),
                           f64(t["rstd2"][i]), SLOPE)
        report(out[i].reshape(V, C), fw["out"], R.element_bound(fw["out"], fw["A"], fw["K"], dtype), f"{name} {dtype} {kind} out[{i}]")
        flagged_n += int(fw["flagged"].sum())
        # pooled tensor and arg-max words from the STORED out
        stored = out[i].float()
        m, first, tied = R.pool_first_max(stored)
        tied_n += int(tied.sum())
        same(pooled[i].float().reshape(Vo, C), m, f"{name} {dtype} {kind} pooled[{i}]")
        ncdhw = stored.permute(3, 0, 1, 2)[None].contiguous()
        tp, idx = F.max_pool3d(ncdhw, 2, return_indices=True)
        same(pooled[i].float(), tp[0].permute(1, 2, 3, 0), f"{name} {dtype} {kind} pooled[{i}] vs F.max_pool3d")
        same(R.decode_words(words[i], C), first, f"{name} {dtype} {kind} arg-max fields[{i}]")
        # backward: routing from torch's own max_pool3d indices on the stored out
        gp = g_pool[i].double()
        routed = R.route_pool_grad(gp, idx[0].permute(1, 2, 3, 0), d, h, w).reshape(V, C)
        go = g_out[i].double().reshape(V, C)
        bw = R.cat_backward(fw, go + routed, go.abs() + routed.abs(), SLOPE)
        xh, xh2, rs = fw["xh"], fw["xh2"], f64(t["rstd"][i])
        xh2m = xh2.abs() + fw["xh2_err"]
        flip = bw["flip"]                              # |g| of the elements whose x-branch sign the f32 evaluation does not decide
        # sums: g + pooled g (1), LeakyReLU' (1), the cast to the record (1); the products with xhat 3 more
        report(res["m1"][i], bw["d1"].mean(0), R.sum_bound(bw["d1_abs"].mean(0), L, 3), f"{name} {dtype} {kind} m1[{i}]")
        report(res["m2"][i], (bw["d1"] * xh).mean(0), R.sum_bound((bw["d1_abs"] * xh.abs()).mean(0), L, 6), f"{name} {dtype} {kind} m2[{i}]")
        report(res["m1b"][i], bw["d2"].mean(0), R.sum_bound(bw["d2_abs"].mean(0), L, 3) + flip.mean(0), f"{name} {dtype} {kind} m1b[{i}]")
        report(res["m2b"][i], (bw["d2"] * xh2).mean(0), R.sum_bound((bw["d2_abs"] * xh2m).mean(0), L, 6) + (flip * xh2m).mean(0),
               f"{name} {dtype} {kind} m2b[{i}]")
        # dx = the stored branch's draw, from the kernel's own m1, m2: 8 roundings (sum, LeakyReLU', xhat 2, product, two
        # subtractions, product).  The sign of xhat is exact in both evaluations: nothing is excluded.
        m1, m2 = f64(res["m1"][i]), f64(res["m2"][i])
        ref = R.in_backward(bw["d1"], xh, rs, m1, m2)
        A = rs * (bw["d1_abs"] + m1.abs() + (xh * m2).abs())
        (store_check or report)(res["dx"][i].reshape(V, C), ref, R.element_bound(ref, A, 8, dtype), f"{name} {dtype} {kind} dx[{i}]")
        # dW2 in float64 from float64 statistics of the x-branch (the kernel forms it in f64 from the sums S_k = sum dxhat2 x_k,
        # sum dxhat2 and the input's moments); its tolerance propagates the sum bounds of those three sums through
        # dW2_i = rs (A_i - rs^2 (wa A_0 + wb A_1)(wa C_0i + wb C_1i)),  A_k = S_k - mean(x_k) sum dxhat2
        r2, _ = R.xbranch(xi, w2d)
        mean2d, rstd2d = R.stats(r2, EPS)
        xh2d = (r2 - mean2d) * rstd2d
        d2 = bw["d2"]
        draw2 = R.in_backward(d2, xh2d, rstd2d, d2.mean(0), (d2 * xh2d).mean(0))
        dw_ref += draw2.t() @ xi
        dS = torch.stack([R.sum_bound((bw["d2_abs"] * xi[:, k:k + 1].abs()).sum(0), L, 4) + (flip * xi[:, k:k + 1].abs()).sum(0)
                          for k in range(2)], 1)                                                        # [C, 2]
        dSd = R.sum_bound(bw["d2_abs"].sum(0), L, 3) + flip.sum(0)
        mx = xi.mean(0)
        cov = (xi.t() @ xi) / V - mx[:, None] * mx[None, :]
        dA = dS + mx.abs()[None, :] * dSd[:, None]
        cw = w2d @ cov                                                                                  # [C, 2]: wa C_0i + wb C_1i
        dw_tol += rstd2d[:, None] * (dA + rstd2d[:, None] ** 2 * cw.abs() * (w2d.abs() * dA).sum(1, keepdim=True))
        del fw, bw, ref, A, routed, go, draw2
    got = res["dw2"].reshape(C, 2)
    if dtype == "fp32":
        report(got, dw_ref, torch.full_like(dw_ref, 2e-6 * float(dw_ref.abs().max())), f"{name} {dtype} {kind} dW2")
    else:
        report(got, dw_ref, dw_tol + R.ulp32(dw_ref), f"{name} {dtype} {kind} dW2")
    tie_share, flag_share = tied_n / (n * Vo * C), flagged_n / (n * V * C)
    print(f"  {name} {dtype} {kind}: tied maxima {tie_share:.4f} of (window, channel) pairs, undecided x-branch signs {flag_share:.2e}")
    if kind == "ties":
        assert tie_share > 0.10, tie_share
        assert flagged_n == 0
    else:
        assert flag_share < 1e-5, flag_share


def aggregation_one_branch(S, cfg, case, grad_scale=None, store_check=None):
    """ec123, dc22, dc42: cat_epilogue_fwd / cat_epilogue_bwd without a second branch."""
    name, dtype = case
    b = cfg.BLOCKS[name]
    n, d, h, w = b["dims"]
    C, V = b["C"], d * h * w
    g = gen(seed_of(name, dtype))
    raw = act((n, d, h, w, C), dtype, g, centre=0.8)
    g_out = scale_grad(act((n, d, h, w, C), dtype, g, centre=0.2), grad_scale)
    mean, rstd = check_stats(S, raw, f"{name} {dtype}")
    out = S.cat_epilogue_fwd(raw, mean, rstd, slope=SLOPE)
    dx, _ = S.cat_epilogue_bwd(g_out, raw, mean, rstd, slope=SLOPE)
    L = 0 if dtype == "fp32" else thread_chain(b["dims"], C)
    for i in range(n):
        mu, rs = f64(mean[i]), f64(rstd[i])
        xh = (raw[i].double().reshape(V, C) - mu) * rs
        y = R.lrelu(xh, SLOPE)
        report(out[i].reshape(V, C), y, R.element_bound(y, y.abs(), 3, dtype), f"{name} {dtype} out[{i}]")     # x - mean, rstd, slope
        go = g_out[i].double().reshape(V, C)
        dd = go * torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, SLOPE))
        m1, m2 = dd.mean(0), (dd * xh).mean(0)
        # this wrapper does not return the kernel's m1, m2: the float64 ones are used and their sum bounds enter the element's
        e1, e2 = R.sum_bound(dd.abs().mean(0), L, 2 + 1), R.sum_bound((dd * xh).abs().mean(0), L, 5 + 1)
        ref = R.in_backward(dd, xh, rs, m1, m2)
        A = rs * (dd.abs() + m1.abs() + (xh * m2).abs())
        (store_check or report)(dx[i].reshape(V, C), ref, R.element_bound(ref, A, 7, dtype) + rs * (e1 + xh.abs() * e2), f"{name} {dtype} dx[{i}]")


# ---- max-pool ------------------------------------------------------------------------------------------------------------------
def maxpool_forward(S, case):
    name, C, (n, d, h, w), dtype = case
    t = act((n, d, h, w, C), dtype, gen(seed_of("pool", name, dtype)))
    got = S.maxpool_fwd(t)
    for i in range(n):
        want = F.max_pool3d(t[i].float().permute(3, 0, 1, 2)[None], 2)[0].permute(1, 2, 3, 0)
        same(got[i].float(), want, f"maxpool_fwd after {name} {dtype} [{i}]")


def maxpool_backward(S, case, grad_scale=None, shares=None):
    """g_in (+)= the pooled gradient at the first maximum of every window: round_T(g + prev) formed in f32 is exact.
    (shares: a list that receives, per sample, the share of the expected elements that are inf -- the overflow-on-store runs)"""
    name, C, (n, d, h, w), dtype, acc = case
    g = gen(seed_of("poolb", name, dtype))
    t = levels((n, d, h, w, C), dtype, g, 6)             # ties included
    g_out = act((n, d // 2, h // 2, w // 2, C), dtype, g)
    prev = act((n, d, h, w, C), dtype, g)
    g_out, prev = scale_grad(g_out, grad_scale), scale_grad(prev, grad_scale)
    got = S.maxpool_bwd(t, g_out, prev.clone() if acc else None)
    for i in range(n):
        _, first, _ = R.pool_first_max(t[i].float())
        k = torch.arange(8, device="cuda")[None, :, None]
        win = torch.where(first[:, None, :] == k, g_out[i].float().reshape(-1, 1, C), torch.zeros((), device="cuda"))
        want = R.unpool_windows(win, d, h, w)
        if acc:
            want = (want + prev[i].float()).to(R.storage(dtype)).float()
        if shares is not None:
            shares.append(float(want.isinf().double().mean()))
        same(got[i].float(), want, f"maxpool_bwd after {name} {dtype} accumulate={acc} [{i}]")


# ---- x2 up-sampling ------------------------------------------------------------------------------------------------------------
def upsample_forward(S, case):
    """10 roundings: 1 - ly, 1 - lx, their product, the product with the value, 3 additions of the four corners; then 1 - lz,
    a product and an addition along z.  A: the same interpolation of |input| (all weights are non-negative).  The f32 source
    coordinate adds R.lambda_term (lambda is off by <= u (n - 1) per axis)."""
    name, C, (n, d, h, w), dtype = case
    t = act((n, d, h, w, C), dtype, gen(seed_of("up", name, dtype)))
    got = S.upsample2_fwd(t)
    for i in range(n):
        x = t[i].double()
        ref, A = R.upsample(x), R.upsample(x.abs())
        report(got[i], ref, R.element_bound(ref, A, 10, dtype, U * R.lambda_term(x.abs())), f"upsample2_fwd into {name} {dtype} [{i}]")


def upsample_backward(S, case, grad_scale=None, store_check=None):
    """The marching kernel reduces y (weight 2 roundings, product, <= 5 additions), x (2, 1, <= 6) and z (2, 1, <= 6) and adds
    the previous gradient once: 27.  A: the adjoint applied to |g|, plus |previous|; R.lambda_term as in the forward."""
    name, C, (n, d, h, w), dtype, acc = case
    g = gen(seed_of("upb", name, dtype))
    g_out = act((n, 2 * d, 2 * h, 2 * w, C), dtype, g)
    prev = act((n, d, h, w, C), dtype, g)
    g_out, prev = scale_grad(g_out, grad_scale), scale_grad(prev, grad_scale)
    got = S.upsample2_bwd(g_out, prev.clone() if acc else None)
    for i in range(n):
        x = g_out[i].double()
        ref, A = R.upsample(x, transpose=True), R.upsample(x.abs(), transpose=True)
        if acc:
            ref, A = ref + prev[i].double(), A + prev[i].double().abs()
        (store_check or report)(got[i], ref, R.element_bound(ref, A, 27, dtype, U * R.lambda_term(x.abs(), transpose=True)), f"upsample2_bwd out of {name} {dtype} accumulate={acc} [{i}]")


# ---- heads ---------------------------------------------------------------------------------------------------------------------
def head_forward(S, cfg, nlevels):
    """pred = bias + level 0 + sum_l interpolation_{2^l}(level l).  Per coarse term 10 roundings (as the up-sampling forward:
    two weights, their product, 4 products and 3 additions, then 1 - lx, a product, an addition); the chain adds <= 4 terms."""
    n, (D, H, W) = cfg.batch, cfg.extent
    g = gen(seed_of("head", nlevels))
    maps = [torch.randn((n, D >> l, H >> l, W >> l), generator=g, device="cuda") * (1 + l) + 0.3 for l in range(nlevels)]
    bias = torch.randn(1, generator=g, device="cuda")
    pred = S.head_fwd(maps, bias)
    for i in range(n):
        ref = bias.double() + maps[0][i].double()
        S_ = bias.double().abs() + maps[0][i].double().abs()
        lam = 0.0       # (the f32 source coordinates of the coarse levels: R.lambda_term)
        for l in range(1, nlevels):
            m = maps[l][i].double()[..., None]
            ref = ref + R.upsample(m, 2 ** l)[..., 0]
            S_ = S_ + R.upsample(m.abs(), 2 ** l)[..., 0]
            lam = lam + U * R.lambda_term(m.abs(), 2 ** l)[..., 0]
        report(pred[i, 0], ref, R.sum_bound(S_, 4, 10) + lam, f"head_fwd {nlevels} levels [{i}]")


def head_backward(S, cfg, nlevels, grad_scale=None):
    """Three axis passes per level, each a chain of up to T taps of its own axis (weight 2 roundings, product 1): L = T_x + T_y +
    T_z (3 T_l on a cube), K = 9.  The bias gradient's partials are all f64: 1 ulp of f32 at the float64 sum."""
    n, (D, H, W) = cfg.batch, cfg.extent
    g_pred = scale_grad(torch.randn((n, 1, D, H, W), generator=gen(seed_of("headb", nlevels)), device="cuda") + 0.1, grad_scale)
    lv, gb = S.head_bwd(g_pred, nlevels)
    tot = g_pred.double().sum()
    report(gb, tot.reshape(1), R.ulp32(tot).reshape(1) + g_pred.numel() * 2.0 ** -53 * g_pred.double().abs().sum().reshape(1), "head_bwd bias gradient")
    for l in range(1, nlevels):
        taps = sum(R.max_taps(e >> l, 2 ** l, "cuda") for e in (D, H, W))
        for i in range(n):
            x = g_pred[i, 0].double()[..., None]
            ref = R.upsample(x, 2 ** l, transpose=True)[..., 0]
            S_ = R.upsample(x.abs(), 2 ** l, transpose=True)[..., 0]
            report(lv[l][i], ref, R.sum_bound(S_, taps, 9) + U * R.lambda_term(x.abs(), 2 ** l, transpose=True)[..., 0], f"head_bwd {nlevels} levels, level {l} [{i}]")


# ---- one forward of the real network, block by block -----------------------------------------------------------------------------
def network_forward_block_by_block(S, cfg, dtype):
    """One eval-mode forward of the configuration's network (the benchmark module: 4 x 2 x 128^3).  Every block's stored ``out``
    against the float64 epilogue of its own stored ``raw`` / ``mean`` / ``rstd`` and the module's parameters (the bounds of the
    op-level cases); the x-branches' mean / rstd
    against float64 moments of the (rounded, pooled) input; and both heads' logits recomputed in float64 from the eighteen
    gated blocks: side conv of the float64 e, head weight of the block's slot, the level map of its level, trilinear
    interpolation, bias.  This is the part that sees the wiring: which block feeds which level map of which head.
    (The level maps are formed from the kernels' unrounded e, so the reference takes the float64 e of the stored raw tensor
    rather than the stored, rounded ``out``: that keeps the bound free of a 0.5 ulp_T term per channel.)"""
    from seunet_amd.SE_UNet import SE_UNet
    _cache.clear()
    torch.cuda.empty_cache()
    with torch.random.fork_rng(devices=[]):
        torch.default_generator.manual_seed(1234)     # (the CPU generator only: parameters are drawn on the CPU)
        net = SE_UNet(2, 1, width_mult=cfg.width, act_dtype=dtype, negative_slope=SLOPE)
    net = net.cuda().eval()
    g = gen(seed_of("net", dtype))
    D, H, W = cfg.extent
    x = torch.randn((cfg.batch, 2, D, H, W), generator=g, device="cuda")
    x = x * torch.tensor([1.0, 0.6], device="cuda").view(1, 2, 1, 1, 1) + 0.4 * torch.randn((cfg.batch, 2, 1, 1, 1), generator=g, device="cuda")
    x_lv = [x.to(R.storage(dtype)).float()]                       # the network's rounded copy of the input, pooled per level
    for _ in range(2):
        x_lv.append(F.max_pool3d(x_lv[-1], 2))
    ext = lambda l: (D >> l, H >> l, W >> l)           # the level maps are (N, 1, D_l, H_l, W_l)
    lvl = {(hd, l): torch.zeros((cfg.batch, (D >> l) * (H >> l) * (W >> l)), dtype=torch.float64, device="cuda") for hd in (0, 1) for l in range(4 - hd)}
    lvl_S = {k: torch.zeros_like(v) for k, v in lvl.items()}
    heads = (net.dc0_0, net.dc0_1)
    groups = [[n] for n in cfg.PLAN if cfg.BLOCKS[n]["level"] == 0] + [[n for n in cfg.PLAN if cfg.BLOCKS[n]["level"] == l] for l in (1, 2, 3)]
    seen = 0
    for names in groups:
        ask = list(names) + [cfg.PLAN[n]["x_name"] for n in names if cfg.PLAN[n]["x_name"]]
        pred0, pred1, inter = net.forward_with_intermediates(x, ask)
        for name in names:
            b, rec, mod = cfg.BLOCKS[name], inter[name], getattr(net, name)
            n, d, h, w = b["dims"]
            C, V = b["C"], d * h * w
            cl = lambda t, i: t[i].permute(1, 2, 3, 0).reshape(V, -1).double()
            for i in range(n):
                raw, mu, rs = cl(rec["raw"], i), f64(rec["mean"][i]), f64(rec["rstd"][i])
                got = cl(rec["out"], i)
                if b["gated"]:
                    w2 = f64(mod.conv_se2.weight.reshape(C)) if b["gates"] == 2 else None
                    fw = R.gate_forward(raw, mu, rs, f64(mod.conv_se.weight.reshape(C)), w2, f64(mod.conv2.weight.reshape(2, C)),
                                        f64(mod.conv2.bias), SLOPE)
                    report(got, fw["e"], R.element_bound(fw["e"], fw["e"].abs() * fw["F"][:, None], R.KE(C), dtype), f"net {dtype} {name} out[{i}]")
                    hw = f64(heads[b["head"]].weight.reshape(-1)[2 * b["slot"]:2 * b["slot"] + 2])
                    lvl[(b["head"], b["level"])][i] += hw[0] * fw["side"][:, 0] + hw[1] * fw["side"][:, 1]
                    lvl_S[(b["head"], b["level"])][i] += hw[0].abs() * fw["side_abs"][:, 0] + hw[1].abs() * fw["side_abs"][:, 1]
                elif b["xr"]:
                    xr = inter[cfg.PLAN[name]["x_name"]]
                    w2x = f64(getattr(net, cfg.PLAN[name]["x_name"]).conv1.weight.reshape(C, 2))
                    xi = x_lv[b["level"]][i].permute(1, 2, 3, 0).reshape(V, 2).double()
                    rm, rr = R.stats(R.xbranch(xi, w2x)[0], EPS)
                    tm, tr = stat_tol(rm, rr, R.xbranch(xi, w2x)[0], EPS)
                    report(xr["mean"][i], rm, tm, f"net {dtype} {cfg.PLAN[name]['x_name']} mean[{i}]")
                    report(xr["rstd"][i], rr, tr, f"net {dtype} {cfg.PLAN[name]['x_name']} rstd[{i}]")
                    fw = R.cat_forward(raw, mu, rs, xi, w2x, f64(xr["mean"][i]), f64(xr["rstd"][i]), SLOPE)
                    report(got, fw["out"], R.element_bound(fw["out"], fw["A"], fw["K"], dtype), f"net {dtype} {name} out[{i}]")
                else:
                    y = R.lrelu((raw - mu) * rs, SLOPE)
                    report(got, y, R.element_bound(y, y.abs(), 3, dtype), f"net {dtype} {name} out[{i}]")
                del raw, got
            seen += 1
        del inter
    assert seen == len(cfg.PLAN_LIST) == 24
    # logits.  Chain: the channel dot product and its bias (8 + lg, lg of the widest block: 11 at 64 channels, 12 at 128), <= 3
    # accumulations of a level's blocks, <= 4 additions in the head.  Per term: e (KE of the widest block), w e, hw side, the sum of
    # the two side channels (KE + 4), and the head's 10 (see head_forward)
    for hd, pred in ((0, pred0), (1, pred1)):
        bias = f64(heads[hd].bias)
        for i in range(cfg.batch):
            ref = bias + lvl[(hd, 0)][i].reshape(D, H, W)
            S_ = bias.abs() + lvl_S[(hd, 0)][i].reshape(D, H, W)
            lam = 0.0
            for l in range(1, 4 - hd):
                m = lvl[(hd, l)][i].reshape(*ext(l), 1)
                ms = lvl_S[(hd, l)][i].reshape(*ext(l), 1)
                ref = ref + R.upsample(m, 2 ** l)[..., 0]
                S_ = S_ + R.upsample(ms, 2 ** l)[..., 0]
                lam = lam + U * R.lambda_term(ms, 2 ** l)[..., 0]
            report(pred[i, 0], ref, R.sum_bound(S_, 8 + R.lg_lanes(cfg.max_C) + 3 + 4, R.KE(cfg.max_C) + 4 + 10) + lam, f"net {dtype} pred{hd}[{i}]")
    print(f"  peak device memory of this process so far: {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
