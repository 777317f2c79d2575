"""tests/epilogue_ref.py (the float64 restatement the GPU epilogue tests compare the kernels with) against torch autograd of
F.instance_norm / F.leaky_relu / F.conv3d / F.max_pool3d / F.interpolate(align_corners=True) in float64 on the CPU: two
float64 evaluations of the same graph, so they agree to 1e-10 of the largest element.  Needs no GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_ref as R  # noqa: E402

EPS, SLOPE = 1e-5, 0.01
C, D, H, W = 16, 4, 6, 8
V = D * H * W


def close(got, want, what):
    err = float((got - want).abs().max())
    lim = 1e-10 * max(float(want.abs().max()), 1e-300)
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def cl(t):
    """(1, C, D, H, W) -> [V, C]"""
    return t[0].permute(1, 2, 3, 0).reshape(-1, t.shape[1])


def rnd(*shape, seed):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("gates", (1, 2))
def test_gated_block_matches_autograd(gates):
    raw = (rnd(1, C, D, H, W, seed=1) * 1.7 + 0.4).requires_grad_()
    w_se, w_se2 = (rnd(C, seed=2) * 0.5).requires_grad_(), (rnd(C, seed=3) * 0.5).requires_grad_()
    w_side, b_side = (rnd(2, C, seed=4) * 0.3).requires_grad_(), rnd(2, seed=5).requires_grad_()
    head_w, drop = rnd(2, seed=6).requires_grad_(), torch.tensor([1.4, 0.7], dtype=torch.float64)
    g_e, gl = rnd(1, C, D, H, W, seed=7), rnd(1, D, H, W, seed=8)
    a = F.leaky_relu(F.instance_norm(raw, eps=EPS), SLOPE)
    e = a * torch.sigmoid(F.conv3d(a, w_se.view(1, C, 1, 1, 1)))
    if gates == 2:
        e = e * torch.sigmoid(F.conv3d(e, w_se2.view(1, C, 1, 1, 1)))
    side = F.conv3d(e, w_side.view(2, C, 1, 1, 1), b_side)
    level = (side * (head_w * drop).view(1, 2, 1, 1, 1)).sum(1)
    ((e * g_e).sum() + (level * gl).sum()).backward()

    with torch.no_grad():
        r = cl(raw)
        mean, rstd = R.stats(r, EPS)
        w2 = w_se2 if gates == 2 else None
        fw = R.gate_forward(r, mean, rstd, w_se, w2, w_side, b_side, SLOPE)
        close(fw["e"], cl(e), "e")
        close(fw["side"], cl(side), "side")
        hw = head_w * drop
        bw = R.gate_backward(fw, cl(g_e), gl.reshape(-1), hw, drop, w_se, w2, w_side, b_side, SLOPE)
        draw = R.in_backward(bw["dxh"], fw["xh"], rstd, bw["sum_dxh"] / V, bw["sum_dxh_xh"] / V)
        close(draw, cl(raw.grad), "draw")
        close(bw["dw_se"], w_se.grad, "dw_se")
        if gates == 2:
            close(bw["dw_se2"], w_se2.grad, "dw_se2")
        close(bw["dw_side"], w_side.grad, "dw_side")
        close(bw["db_side"], b_side.grad, "db_side")
        close(bw["dhead_w"], head_w.grad, "dhead_w")
        # the absolute-value evaluation dominates the value, term by term
        for k, v in bw["abs"].items():
            assert bool((v >= bw[k].abs() * (1 - 1e-12)).all()), k


def test_aggregation_block_with_pool_matches_autograd():
    raw = (rnd(1, C, D, H, W, seed=11) * 2 - 0.6).requires_grad_()
    x = rnd(1, 2, D, H, W, seed=12) + torch.tensor([0.3, -1.1], dtype=torch.float64).view(1, 2, 1, 1, 1)
    w2 = rnd(C, 2, seed=13).requires_grad_()
    g, gp = rnd(1, C, D, H, W, seed=14), rnd(1, C, D // 2, H // 2, W // 2, seed=15)
    out = F.leaky_relu(F.instance_norm(raw, eps=EPS), SLOPE) + \
        F.leaky_relu(F.instance_norm(F.conv3d(x, w2.view(C, 2, 1, 1, 1)), eps=EPS), SLOPE)
    pooled, idx = F.max_pool3d(out, 2, return_indices=True)
    ((out * g).sum() + (pooled * gp).sum()).backward()

    with torch.no_grad():
        r, xi = cl(raw), cl(x)
        mean, rstd = R.stats(r, EPS)
        mean2, rstd2 = R.stats(R.xbranch(xi, w2)[0], EPS)
        fw = R.cat_forward(r, mean, rstd, xi, w2, mean2, rstd2, SLOPE)
        close(fw["out"], cl(out), "out")
        assert not bool(fw["flagged"].any())
        o4 = fw["out"].reshape(D, H, W, C)
        m, first, _ = R.pool_first_max(o4)
        close(m, cl(pooled), "pooled")
        routed = R.route_pool_grad(cl(gp).reshape(D // 2, H // 2, W // 2, C), cl(idx).reshape(D // 2, H // 2, W // 2, C), D, H, W)
        gy = cl(g) + routed.reshape(-1, C)
        bw = R.cat_backward(fw, gy, gy.abs(), SLOPE)
        draw1 = R.in_backward(bw["d1"], fw["xh"], rstd, bw["d1"].mean(0), (bw["d1"] * fw["xh"]).mean(0))
        close(draw1, cl(raw.grad), "dx")
        draw2 = R.in_backward(bw["d2"], fw["xh2"], rstd2, bw["d2"].mean(0), (bw["d2"] * fw["xh2"]).mean(0))
        close(draw2.t() @ xi, w2.grad, "dW2")


def test_first_maximum_rule_is_max_pool3d_s_on_ties():
    """Values from a few levels, so most windows hold their maximum more than once: the z-y-x first-maximum rule the argmax
    words follow is the one max_pool3d's indices follow, and the words decode to it."""
    t = torch.randint(0, 3, (D, H, W, C), generator=torch.Generator().manual_seed(3)).double()
    m, first, tied = R.pool_first_max(t)
    assert float(tied.double().mean()) > 0.5
    pooled, idx = F.max_pool3d(t.permute(3, 0, 1, 2)[None], 2, return_indices=True)
    idx = cl(idx)                                                    # [Vo, C] flat voxel index
    vo = torch.arange(idx.shape[0])
    zo, yo, xo = vo // ((H // 2) * (W // 2)), (vo // (W // 2)) % (H // 2), vo % (W // 2)
    base = ((2 * zo) * H + 2 * yo) * W + 2 * xo
    off = idx - base[:, None]
    k = 4 * (off // (H * W)) + 2 * ((off % (H * W)) // W) + (off % W)
    assert torch.equal(k, first)
    assert torch.equal(m, cl(pooled))
    words = (first.reshape(-1, C // 8, 8) << (3 * torch.arange(8))).sum(2).int()
    assert torch.equal(R.decode_words(words, C), first)
    assert torch.equal(R.unpool_windows(R.pool_windows(t), D, H, W), t)


@pytest.mark.parametrize("factor", (2, 4, 8))
def test_interpolation_and_adjoint_match_interpolate(factor):
    t = rnd(1, 3, 4, 5, 7, seed=21).requires_grad_()
    up = F.interpolate(t, scale_factor=factor, mode="trilinear", align_corners=True)
    g = rnd(*up.shape, seed=22)
    (up * g).sum().backward()
    with torch.no_grad():
        tc = t[0].permute(1, 2, 3, 0)
        close(R.upsample(tc, factor, f32_weights=False), up[0].permute(1, 2, 3, 0), "interpolation")
        close(R.upsample(g[0].permute(1, 2, 3, 0), factor, f32_weights=False, transpose=True), t.grad[0].permute(1, 2, 3, 0), "adjoint")
        # the f32-weight form differs from it by the rounding of the source coordinate only
        d = (R.upsample(tc, factor, f32_weights=True) - R.upsample(tc, factor, f32_weights=False)).abs().max()
        assert 0 <= float(d) < 1e-5 * float(tc.abs().max())
    assert R.max_taps(16, 2, "cpu") in (4, 5) and R.max_taps(16, 8, "cpu") <= 24


def test_spacing_and_bounds():
    one = torch.tensor([1.0, 1.5, 0.0, 3e-6, -260.0], dtype=torch.float64)
    assert R.ulp_T(one, "bf16")[:2].tolist() == [2.0 ** -7, 2.0 ** -7] and float(R.ulp_T(one, "bf16")[4]) == 2.0
    assert R.ulp_T(one, "fp16").tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -24, 2.0 ** -24, 0.25]
    assert float(R.ulp_T(one, "fp32").abs().max()) == 0.0
    r = rnd(4096, seed=31) * torch.logspace(-6, 4, 4096, dtype=torch.float64)
    for dt in ("bf16", "fp16"):
        err = (r.to(R.storage(dt)).double() - r).abs()
        assert bool((err <= 0.5 * R.ulp_T(r, dt)).all())
        assert bool((err <= R.element_bound(r, r.abs(), 0, dt)).all())
    assert R.KE(8) == 23 and R.KE(64) == 29 and R.K_DXH(32) == 32 + 4 + 4 * 27
