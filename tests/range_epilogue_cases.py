"""The machinery of tests/test_epilogue_range_gpu.py: the backward epilogue, pooling, up-sampling and head passes on a non-finite
incoming gradient and at the top of fp16's range (the convolutions' side: tests/range_cases.py).

Non-finite: one +inf (then one NaN) at one element of SAMPLE 0's incoming gradient.  The set E that the plant must reach comes
from the float64 reference alone: the output elements that change when the planted element alone is moved by a large finite
amount.  That leaves out taps whose weight is exactly zero (align-corners up-sampling) and takes in every voxel of the (n, c)
whose InstanceNorm means the plant enters.  Required: every element of E -- parameter-gradient entries included -- is non-finite
in the kernel's output, and every output of the other sample equals the unplanted run bitwise.  Nothing is required of sample 0
outside E.  Keys "s:..." are per-sample outputs [n, ...], keys "p:..." parameter gradients (summed over the samples).

Overflow on store: see ``OverflowStore``."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_layer_cases as E  # noqa: E402
import epilogue_ref as ER  # noqa: E402

FP16_INF_FROM = 65520.0
K_MAX = 16                   # GRAD_CLIP x 2^16 = 61440: the largest power of two at which a clamped 16-bit gradient is finite
assert E.GRAD_CLIP * 2.0 ** K_MAX <= 65504 < E.GRAD_CLIP * 2.0 ** (K_MAX + 1)


# ---- overflow on store (fp16) ------------------------------------------------------------------------------------------------------
class Recorder:
    """First run, gradients at scale 1 (clamped): the usual bound check; |ref| and the bound of every stored element are kept."""

    def __init__(self):
        self.mags, self.bounds = [], []

    def __call__(self, got, ref, bound, what):
        E.report(got, ref, bound, what)
        self.mags.append(ref.abs().flatten())
        self.bounds.append((bound.expand_as(ref) if isinstance(bound, torch.Tensor) else torch.full_like(ref, bound)).flatten())

    def exponent(self, k_max=K_MAX, share=0.10):
        """k from the float64 reference alone: the smallest power of two that lifts the top `share` of |ref| to 65520,
        at most k_max."""
        m = torch.cat(self.mags)
        q = float(m.kthvalue(max(1, int(m.numel() * (1 - share)))).values)
        return min(k_max, max(0, math.ceil(math.log2(FP16_INF_FROM / q)))) if q > 0 else k_max

    def shares(self, k):
        """(overflow, finite, left out) of the run at 2^k, from this run's reference: everything is linear in the gradient,
        so reference and bound of the scaled run are these times 2^k (the bound's half spacing of the storage type as well,
        away from the subnormal range)."""
        m, b = torch.cat(self.mags) * 2.0 ** k, torch.cat(self.bounds) * 2.0 ** k
        so, sf = float((m - b >= FP16_INF_FROM).double().mean()), float((m + b < FP16_INF_FROM).double().mean())
        return so, sf, 1.0 - so - sf


def shares_ok(so, sf, sl):
    return so >= 0.01 and sf >= 0.25 and sl <= 0.02


class OverflowStore:
    """Second run, gradients times 2^k: a 16-bit stored output against its float64 reference and EXISTING bound b.
    |ref| - b >= 65520: the element must be +-inf with the reference's sign.  |ref| + b < 65520: finite and within b.
    Otherwise it is left out.  The shares of the three classes are counted over the case (its samples together)."""

    def __init__(self, k):
        self.k, self.counts = k, [0, 0, 0]

    def __call__(self, got, ref, bound, what):
        b = bound.expand_as(ref) if isinstance(bound, torch.Tensor) else torch.full_like(ref, bound)
        over, fin = ref.abs() - b >= FP16_INF_FROM, ref.abs() + b < FP16_INF_FROM
        no, nf = int(over.sum()), int(fin.sum())
        self.counts = [self.counts[0] + no, self.counts[1] + nf, self.counts[2] + ref.numel() - no - nf]
        print(f"  {what}: k = {self.k}: overflow {no / ref.numel():.4f}, finite {nf / ref.numel():.4f}, left out {1 - (no + nf) / ref.numel():.5f}")
        g = got.double()
        bad_inf = over & ~(g.isinf() & (g.sign() == ref.sign()))
        if bool(bad_inf.any()):
            i = tuple(bad_inf.nonzero()[0].tolist())
            pytest.fail(f"{what}: {int(bad_inf.sum())} of {no} elements beyond fp16's range are not +-inf with the reference's sign, "
                        f"first {i}: got {float(got[i])!r} want {float(ref[i])!r}", pytrace=False)
        bad_fin = fin & ~((g - ref).abs() <= b)           # (inf or NaN where a finite value belongs fails here)
        if bool(bad_fin.any()):
            i = tuple(bad_fin.nonzero()[0].tolist())
            pytest.fail(f"{what}: {int(bad_fin.sum())} of {nf} in-range elements are beyond the bound or not finite, "
                        f"first {i}: got {float(got[i])!r} want {float(ref[i])!r} bound {float(b[i]):.3g}", pytrace=False)

    def shares(self):
        t = sum(self.counts)
        return tuple(c / t for c in self.counts)


# The gated blocks attenuate g_e (two sigmoid gates, rstd <= 2): their g_e is clamped to 2^-10, finite up to 2^25, and the f32
# level gradient, which is not clamped, carries draw across 65520.
GATE_CLIP, GATE_K_MAX = 2.0 ** -10, 25
assert GATE_CLIP * 2.0 ** GATE_K_MAX <= 65504 < GATE_CLIP * 2.0 ** (GATE_K_MAX + 1)


def overflow_case(run, k_max=K_MAX):
    """run(grad_scale, store_check): one case function.  Scale 1 first; k is chosen from its float64 reference, and the shares
    that k gives -- at least 1 % overflow, at least 25 % finite, at most 2 % left out, over the case -- are asserted on that
    reference before the scaled run's output exists.  Then 2^k."""
    rec = Recorder()
    run(1.0, rec)
    k = rec.exponent(k_max)
    assert shares_ok(*rec.shares(k)), f"k = {k}: overflow, finite, left out = {rec.shares(k)} of the reference"
    chk = OverflowStore(k)
    run(2.0 ** k, chk)
    so, sf, sl = chk.shares()
    print(f"  chosen k = {k}: overflow {so:.4f}, finite {sf:.4f}, left out {sl:.5f} of the case")
    assert shares_ok(so, sf, sl), (k, so, sf, sl)
    return k, (so, sf, sl)


# ---- a non-finite incoming gradient ----------------------------------------------------------------------------------------------
def reach_set(f, g0, idx, delta=1.0e6):
    """E per output key of the float64 reference f (sample 0's incoming gradient g0 -> dict of outputs): what moves when
    g0[idx] alone moves by delta."""
    base = f(g0)
    g1 = g0.clone()
    g1[idx] += delta
    moved = f(g1)
    assert set(base) == set(moved)
    return {k: base[k] != moved[k] for k in base}


def raw_equal(a, b):
    v = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def check_plants(run, f, g, idx, what):
    """run(g) -> the kernel's outputs for the whole batch's incoming gradient g [n, ...]; f: the float64 reference of sample 0."""
    Eset = reach_set(f, g[0].double(), idx)
    assert any(bool(m.any()) for k, m in Eset.items() if k.startswith("s:")), f"{what}: the plant reaches nothing in the reference"
    clean = run(g)
    assert set(clean) == set(Eset), (sorted(clean), sorted(Eset))
    for k, v in clean.items():
        assert bool(v.isfinite().all()), f"{what}: {k} of the unplanted run is not finite"
    print(f"  {what}: E holds " + ", ".join(f"{int(m.sum())} of {m.numel()} {k[2:]}" for k, m in Eset.items()))
    for val in (float("inf"), float("nan")):
        gp = g.clone()
        gp[(0,) + tuple(idx)] = val
        out = run(gp)
        for k, m in Eset.items():
            got = out[k][0] if k.startswith("s:") else out[k]
            hidden = m.reshape(got.shape) & got.isfinite()
            if bool(hidden.any()):
                pytest.fail(f"{what}, {val} planted at {tuple(idx)} of sample 0: {int(hidden.sum())} of the {int(m.sum())} elements of {k[2:]} that the "
                            f"plant reaches are finite, first {hidden.nonzero()[:4].tolist()}", pytrace=False)
            if k.startswith("s:") and out[k].shape[0] > 1:
                assert raw_equal(out[k][1:], clean[k][1:]), f"{what}, {val} planted in sample 0: {k[2:]} of another sample changed"


def plant_index(shape):
    """An element of a [D, H, W, C] (or [1, D, H, W]) gradient: x = 0 coincides with a coarse node of the align-corners grid (one
    of the two taps there has weight exactly zero), z and y lie between nodes."""
    if len(shape) == 4 and shape[0] == 1:
        return (0, shape[1] // 2 + 1, shape[2] // 3, 0)
    return (shape[0] // 2, shape[1] // 3, 0, shape[3] // 2)


def maxpool_backward_nonfinite(S, case):
    name, C, (n, d, h, w), dtype, acc = case
    g = E.gen(E.seed_of("poolb", name, dtype, "nf"))
    t = E.levels((n, d, h, w, C), dtype, g, 6)
    g_out = E.act((n, d // 2, h // 2, w // 2, C), dtype, g)
    prev = E.act((n, d, h, w, C), dtype, g)
    _, first, _ = ER.pool_first_max(t[0].float())
    k = torch.arange(8, device="cuda")[None, :, None]

    def f(g0):
        win = torch.where(first[:, None, :] == k, g0.reshape(-1, 1, C), torch.zeros((), dtype=g0.dtype, device="cuda"))
        return {"s:g_in": ER.unpool_windows(win, d, h, w) + (prev[0].double() if acc else 0)}

    check_plants(lambda gg: {"s:g_in": S.maxpool_bwd(t, gg, prev.clone() if acc else None)}, f, g_out, plant_index(g_out.shape[1:]),
                 f"maxpool_bwd after {name} {dtype} accumulate={acc}")


def upsample_backward_nonfinite(S, case):
    name, C, (n, d, h, w), dtype, acc = case
    g = E.gen(E.seed_of("upb", name, dtype, "nf"))
    g_out = E.act((n, 2 * d, 2 * h, 2 * w, C), dtype, g)
    prev = E.act((n, d, h, w, C), dtype, g)
    f = lambda g0: {"s:g_in": ER.upsample(g0, transpose=True) + (prev[0].double() if acc else 0)}
    check_plants(lambda gg: {"s:g_in": S.upsample2_bwd(gg, prev.clone() if acc else None)}, f, g_out, plant_index(g_out.shape[1:]),
                 f"upsample2_bwd out of {name} {dtype} accumulate={acc}")


def head_backward_nonfinite(S, cfg, nlevels):
    n, (D, H, W) = cfg.batch, cfg.extent
    g_pred = torch.randn((n, 1, D, H, W), generator=E.gen(E.seed_of("headb", nlevels, "nf")), device="cuda") + 0.1

    def run(gg):
        lv, gb = S.head_bwd(gg, nlevels)
        return {**{f"s:level {l}": lv[l] for l in range(1, nlevels)}, "p:bias": gb.reshape(1)}

    def f(g0):
        x = g0[0][..., None]
        return {**{f"s:level {l}": ER.upsample(x, 2 ** l, transpose=True)[..., 0] for l in range(1, nlevels)}, "p:bias": x.sum().reshape(1)}

    check_plants(run, f, g_pred, plant_index(g_pred.shape[1:]), f"head_bwd {nlevels} levels")


def aggregation_one_branch_nonfinite(S, cfg, case):
    name, dtype = case
    b = cfg.BLOCKS[name]
    n, d, h, w = b["dims"]
    C, V = b["C"], d * h * w
    g = E.gen(E.seed_of(name, dtype, "nf"))
    raw = E.act((n, d, h, w, C), dtype, g, centre=0.8)
    g_out = E.act((n, d, h, w, C), dtype, g, centre=0.2)
    part, slots = S.channel_stats(raw)
    mean, rstd = S.stats_finalize(part, slots, V, E.EPS)
    mu, rs = E.f64(mean[0]), E.f64(rstd[0])
    xh = (raw[0].double().reshape(V, C) - mu) * rs
    slope = torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, E.SLOPE))

    def f(g0):
        dd = g0.reshape(V, C) * slope
        return {"s:dx": ER.in_backward(dd, xh, rs, dd.mean(0), (dd * xh).mean(0)).reshape(d, h, w, C)}

    idx = plant_index(g_out.shape[1:])
    check_plants(lambda gg: {"s:dx": S.cat_epilogue_bwd(gg, raw, mean, rstd, slope=E.SLOPE)[0]}, f, g_out, idx, f"{name} {dtype} cat_epilogue_bwd")
    # the whole (n, c) of the plant is in E: its InstanceNorm means carry it to every voxel
    assert bool(reach_set(f, g_out[0].double(), idx)["s:dx"][..., idx[3]].all())


def gate_backward_nonfinite(S, cfg, case):
    name, dtype = case
    b, t = cfg.BLOCKS[name], E.gate_block(S, cfg, name, dtype)
    p, raw = t["p"], t["raw"]
    n, d, h, w = b["dims"]
    C, V = b["C"], d * h * w
    sl = slice(2 * p["slot"], 2 * p["slot"] + 2)
    drop_all = p["drop_all"].clone()
    drop_all[0] = torch.where(drop_all[0] == 0, torch.ones_like(drop_all[0]), drop_all[0])     # sample 0: no exact-zero multiplier
    head_w, drop = p["head_w_all"][sl].contiguous(), drop_all[:, sl]
    g = E.gen(E.seed_of(name, dtype, "bwd", "nf"))
    g_e = E.act((n, d, h, w, C), dtype, g, centre=0.2)
    gl = torch.randn((n, 1, d, h, w), generator=g, device="cuda") * 0.5 + 0.1
    args = (raw, t["mean"], t["rstd"], p["w_se"], p["w_se2"], p["w_side"], p["b_side"], E.SLOPE)
    pkeys = ("dw_se", "dw_se2", "dw_side", "db_side", "dhead_w")

    def run_with(ge, glv):
        out = S.gate_epilogue_bwd(*args, g_e=ge, g_level=glv, head_w=head_w, drop=drop, drop_stride=p["nch"], fused_finalize=True)
        return {"s:draw": out["draw"], "s:m1": out["m1"], "s:m2": out["m2"], **{"p:" + k: out[k].reshape(-1) for k in pkeys}}

    run = lambda gg: run_with(gg, gl)

    w2 = None if p["w_se2"] is None else E.f64(p["w_se2"])
    rs = E.f64(t["rstd"][0])
    fw = ER.gate_forward(raw[0].double().reshape(V, C), E.f64(t["mean"][0]), rs, E.f64(p["w_se"]), w2, E.f64(p["w_side"]), E.f64(p["b_side"]), E.SLOPE)
    dr = E.f64(drop[0])

    def f_with(ge0, gl0):
        bw = ER.gate_backward(fw, ge0.reshape(V, C), gl0, E.f64(head_w) * dr, dr, E.f64(p["w_se"]), w2,
                              E.f64(p["w_side"]), E.f64(p["b_side"]), E.SLOPE)
        dxh = bw["dxh"]
        m1, m2 = dxh.mean(0), (dxh * fw["xh"]).mean(0)
        return {"s:draw": ER.in_backward(dxh, fw["xh"], rs, m1, m2).reshape(d, h, w, C), "s:m1": m1, "s:m2": m2,
                **{"p:" + k: bw[k].reshape(-1) for k in pkeys}}

    f = lambda g0: f_with(g0, gl[0].double().reshape(V))
    check_plants(run, f, g_e, plant_index(g_e.shape[1:]), f"{name} {dtype} gate_epilogue_bwd, plant in g_e")
    # ... and in the f32 gradient of the level map, which also feeds dw_side, db_side and dhead_w
    run_l = lambda gg: run_with(g_e, gg)
    f_l = lambda g0: f_with(g_e[0].double(), g0.reshape(V))
    check_plants(run_l, f_l, gl, plant_index(gl.shape[1:]), f"{name} {dtype} gate_epilogue_bwd, plant in g_level")


def aggregation_x_pool_backward_nonfinite(S, cfg, case):
    """The encoder aggregation block's backward with the pooled gradient added on the fly: one plant in g_out, then one in
    the pooled gradient (which reaches the block through the arg-max words)."""
    name, dtype, kind = case
    t = E.x_block(S, cfg, name, dtype, kind)
    C, (n, d, h, w), _, w2 = E.x_case_shape(cfg, name)
    V = d * h * w
    raw, x_in = t["raw"], t["x_in"]
    w2d = E.f64(w2)
    out, pooled, words = S.cat_epilogue_fwd_x_pool(raw, t["mean"], t["rstd"], x_in, w2, 2, t["mean2"], t["rstd2"], E.SLOPE)
    g = E.gen(E.seed_of(name, dtype, kind, "bwd", "nf"))
    g_out = E.act((n, d, h, w, C), dtype, g, centre=0.2)
    g_pool = E.act((n, d // 2, h // 2, w // 2, C), dtype, g, centre=0.2)

    def run_with(go, gp):
        res = S.cat_epilogue_bwd_x(go, raw, t["mean"], t["rstd"], x_in, w2, 2, t["mean2"], t["rstd2"], t["mom"], E.SLOPE, E.EPS,
                                   pool_argmax=words, pool_g=gp)
        return {**{"s:" + k: res[k] for k in ("dx", "m1", "m2", "m1b", "m2b")}, "p:dw2": res["dw2"].reshape(-1)}

    xi = x_in[0, ..., :2].double().reshape(V, 2)
    rs = E.f64(t["rstd"][0])
    fw = ER.cat_forward(raw[0].double().reshape(V, C), E.f64(t["mean"][0]), rs, xi, w2d, E.f64(t["mean2"][0]), E.f64(t["rstd2"][0]), E.SLOPE)
    _, idx = F.max_pool3d(out[0].float().permute(3, 0, 1, 2)[None].contiguous(), 2, return_indices=True)
    idx = idx[0].permute(1, 2, 3, 0)
    r2, _ = ER.xbranch(xi, w2d)
    mean2d, rstd2d = ER.stats(r2, E.EPS)
    xh2d = (r2 - mean2d) * rstd2d

    def f_with(go0, gp0):
        gy = go0.reshape(V, C) + ER.route_pool_grad(gp0, idx, d, h, w).reshape(V, C)
        bw = ER.cat_backward(fw, gy, gy.abs(), E.SLOPE)
        d1, d2 = bw["d1"], bw["d2"]
        m1, m2 = d1.mean(0), (d1 * fw["xh"]).mean(0)
        draw2 = ER.in_backward(d2, xh2d, rstd2d, d2.mean(0), (d2 * xh2d).mean(0))
        return {"s:dx": ER.in_backward(d1, fw["xh"], rs, m1, m2).reshape(d, h, w, C), "s:m1": m1, "s:m2": m2, "s:m1b": d2.mean(0),
                "s:m2b": (d2 * fw["xh2"]).mean(0), "p:dw2": (draw2.t() @ xi).reshape(-1)}

    check_plants(lambda gg: run_with(gg, g_pool), lambda g0: f_with(g0, g_pool[0].double()), g_out, plant_index(g_out.shape[1:]),
                 f"{name} {dtype} {kind} cat_epilogue_bwd_x, plant in g_out")
    check_plants(lambda gg: run_with(g_out, gg), lambda g0: f_with(g_out[0].double(), g0), g_pool, plant_index(g_pool.shape[1:]),
                 f"{name} {dtype} {kind} cat_epilogue_bwd_x, plant in the pooled gradient")
