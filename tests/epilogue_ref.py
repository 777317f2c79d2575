"""Plain float64 restatement of the epilogue and resampling passes, and the derived error bounds the GPU tests assert.

Everything here is ordinary torch arithmetic in float64 on ONE sample, channels-last ``[D, H, W, C]`` (or ``[V, C]``), on
whatever device the inputs live on; nothing calls the native library.  tests/test_epilogue_ref_host.py pins these functions
against torch autograd of ``F.instance_norm`` / ``F.leaky_relu`` / ``F.conv3d`` / ``F.max_pool3d`` / ``F.interpolate`` on the
CPU; tests/test_epilogue_layers_gpu.py compares the HIP kernels with them.

Two evaluations of every backward expression are returned: its value, and the same expression tree evaluated on ABSOLUTE
values (every sum a sum of magnitudes).  The second is the ``A`` / ``S`` of the bounds: a chain of K f32 roundings through an
expression of sums and products is off by at most K u A (u = 2^-24, first order), whatever cancels in the value.

Rounding counts (from csrc/gate.hip and csrc/cat.hip; lg = log2(C / 8), the depth of the cross-lane sum of a per-voxel dot product):
  * a = LeakyReLU((x - mean) rstd): 3.  A per-voxel dot product z = sum_c w_c a_c: 1 product + 7 + lg additions on top of its
    operands, so |dz| <= (11 + lg) u Z with Z = sum_c |w_c a_c|.
  * 16-bit gate g = rcp(1 + exp2(-log2e z)): constant and product 2 (as 2 u |z| on the exponent), v_exp_f32 1 ulp = 2 u,
    addition 1, v_rcp_f32 1 ulp = 2 u: relative (5 + 2 |z|) u, plus (1 - g) |dz| from its argument.  The f32-storage gate (expf,
    IEEE division) is inside the same figure.
  * e = a g1 g2: rel(e) <= KE u (1 + Z1)(1 + Z2), KE = 23 + 2 lg  [rel(b) <= (13 + lg)(1 + Z1) u for b = a g1; the second gate
    sees b, so its argument error is Z2 (rel(b) + (8 + lg) u); add the two products and the second gate's own 5 u].
  * g (1 - g) is formed from the computed g: its ABSOLUTE error is <= g (1 - g) |dz| + 6 u g, which is not small relative to
    g (1 - g) when g -> 1.  The absolute-value evaluation therefore uses g (2 - g) >= g (1 - g) + g in its place.
  * dxhat of a gated block: 5 (de + g_level (w20 hw0 + w21 hw1)) + 2 x (1 + 7 + lg) (the two channel dot products) + 2 x 3
    (q = t g (1 - g)) + 2 x 2 (de g + q w) + 1 (LeakyReLU') = 32 + 2 lg roundings of its own, and the longest path multiplies four
    factors (b, g2 (1 - g2), a, g1 (1 - g1)) that each carry rel <= KE u F, F = (1 + Z1)(1 + Z2):  K_DXH = 32 + 2 lg + 4 KE.
  * draw = rstd (dxhat - m1 - xhat m2): 6 more (xhat 2, product, two subtractions, product).
"""
import math

import torch

U = 2.0 ** -24
MANT = {"bf16": 8, "fp16": 11}            # significand bits (hidden bit included)
MIN_EXP = {"bf16": -126, "fp16": -14}     # exponent of the smallest normal number


def storage(dtype):
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype]


def ulp_T(r, dtype):
    """Spacing of the storage type at |r| (float64 tensor in, float64 out); 0 for fp32 storage, whose one final rounding is
    counted in K like every other f32 rounding."""
    if dtype == "fp32":
        return torch.zeros_like(r)
    _, e = torch.frexp(r.abs())                          # |r| = m 2^e, m in [0.5, 1)
    e = torch.where(r == 0, torch.full_like(e, MIN_EXP[dtype] + 1), e).clamp(min=MIN_EXP[dtype] + 1)
    return torch.ldexp(torch.ones_like(r), e - MANT[dtype])


def ulp32(r):
    """Spacing of float32 at |r| (normal range)."""
    _, e = torch.frexp(r.abs())
    return torch.ldexp(torch.ones_like(r), e.clamp(min=-125) - 24)


def element_bound(ref, A, K, dtype, extra=0.0):
    """|got - ref| for a value computed in f32 with K roundings over terms of total magnitude A and rounded once to the
    storage type: the f32 value v is within E = K u A (+ extra, a term derived separately) of ref, and the stored value
    within half a spacing AT v of v."""
    E = K * U * A + extra
    return 0.5 * ulp_T(ref.abs() + E, dtype) + E


def sum_bound(S, L, K):
    """|got - ref| of a sum whose longest f32 chain has L additions, of summands with K roundings each and magnitudes S."""
    return (L + K) * U * S


def lg_lanes(C):
    return int(math.log2(C // 8))


def KE(C):
    return 23 + 2 * lg_lanes(C)


def K_DXH(C):
    return 32 + 2 * lg_lanes(C) + 4 * KE(C)


def lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


# ---- InstanceNorm statistics ---------------------------------------------------------------------------------------------
def stats(t, eps):
    """(mean, rstd) per channel of t [V, C] (biased variance, as nn.InstanceNorm3d)."""
    mean = t.mean(0)
    var = (t * t).mean(0) - mean * mean
    return mean, 1.0 / torch.sqrt(var.clamp(min=0) + eps)


# ---- gated block -----------------------------------------------------------------------------------------------------------
def gate_forward(raw, mean, rstd, w_se, w_se2, w_side, b_side, slope):
    """raw [V, C]; mean, rstd, w_se, w_se2 (or None) [C]; w_side [2, C]; b_side [2].  Returns the forward's intermediates."""
    xh = (raw - mean) * rstd
    a = lrelu(xh, slope)
    g1 = torch.sigmoid(a @ w_se)
    b = a * g1[:, None]
    Z1 = a.abs() @ w_se.abs()
    if w_se2 is not None:
        g2 = torch.sigmoid(b @ w_se2)
        Z2 = b.abs() @ w_se2.abs()
    else:
        g2, Z2 = torch.ones_like(g1), torch.zeros_like(g1)
    e = b * g2[:, None]
    side = e @ w_side.t() + b_side
    F = (1 + Z1) * (1 + Z2)
    side_abs = (e.abs() * F[:, None]) @ w_side.abs().t() + b_side.abs()      # (e carries rel <= KE u F into the side conv)
    return {"xh": xh, "a": a, "b": b, "g1": g1, "g2": g2, "e": e, "side": side, "side_abs": side_abs, "F": F}


def _gate_bwd_core(de, gl, wc, a, b, g1, g2, s1, s2, w_se, w_se2, mask):
    de = de + gl[:, None] * wc
    q2 = None
    if w_se2 is not None:
        q2 = (de * b).sum(1) * s2
        de = de * g2[:, None] + q2[:, None] * w_se2
    q1 = (de * a).sum(1) * s1
    return (de * g1[:, None] + q1[:, None] * w_se) * mask, q1, q2


def gate_backward(fw, g_e, gl, hw, drop, w_se, w_se2, w_side, b_side, slope):
    """The block's backward for the upstream gradients g_e [V, C] of e and gl [V] of the level map it feeds with
    level += hw[0] side[0] + hw[1] side[1], hw[k] = head weight x drop[k].  Returns the sums (not yet divided or
    combined over samples) with their absolute-value counterparts under "abs"."""
    a, b, g1, g2, e, xh = fw["a"], fw["b"], fw["g1"], fw["g2"], fw["e"], fw["xh"]
    mask = torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, slope))
    wc = w_side[0] * hw[0] + w_side[1] * hw[1]
    wc_abs = w_side[0].abs() * abs(hw[0]) + w_side[1].abs() * abs(hw[1])
    two = w_se2 is not None
    dxh, q1, q2 = _gate_bwd_core(g_e, gl, wc, a, b, g1, g2, g1 * (1 - g1), g2 * (1 - g2), w_se, w_se2, mask)
    dxh_abs, q1a, q2a = _gate_bwd_core(g_e.abs(), gl.abs(), wc_abs, a.abs(), b.abs(), g1, g2, g1 * (2 - g1), g2 * (2 - g2),
                                       w_se.abs(), w_se2.abs() if two else None, mask)
    F = fw["F"]
    dxh_abs = dxh_abs * F[:, None]
    G = (gl[:, None] * e).sum(0)
    G_abs = (gl.abs()[:, None] * e.abs() * F[:, None]).sum(0)
    sg, sg_abs = gl.sum(), gl.abs().sum()
    val = {"dxh": dxh, "sum_dxh": dxh.sum(0), "sum_dxh_xh": (dxh * xh).sum(0),
           "dw_se": (q1[:, None] * a).sum(0), "dw_se2": (q2[:, None] * b).sum(0) if two else torch.zeros_like(w_se),
           "dw_side": torch.stack([hw[0] * G, hw[1] * G]), "db_side": torch.stack([hw[0] * sg, hw[1] * sg]),
           "dhead_w": torch.stack([drop[k] * ((w_side[k] * G).sum() + b_side[k] * sg) for k in range(2)])}
    ab = {"dxh": dxh_abs, "sum_dxh": dxh_abs.sum(0), "sum_dxh_xh": (dxh_abs * xh.abs()).sum(0),
          "dw_se": ((q1a * F)[:, None] * a.abs()).sum(0),
          "dw_se2": ((q2a * F)[:, None] * b.abs()).sum(0) if two else torch.zeros_like(w_se),
          "dw_side": torch.stack([abs(hw[0]) * G_abs, abs(hw[1]) * G_abs]),
          "db_side": torch.stack([abs(hw[0]) * sg_abs, abs(hw[1]) * sg_abs]),
          "dhead_w": torch.stack([abs(drop[k]) * ((w_side[k].abs() * G_abs).sum() + b_side[k].abs() * sg_abs) for k in range(2)])}
    val["abs"] = ab
    return val


def in_backward(dxh, xh, rstd, m1, m2):
    """draw = rstd (dxhat - m1 - xhat m2)."""
    return rstd * (dxh - m1 - xh * m2)


# ---- aggregation block with the recomputed x-branch and the fused pool ------------------------------------------------------
def xbranch(x_in, w2):
    """raw2 = w2 . x of the 2-channel input x_in [V, 2], w2 [C, 2], and the magnitude of its terms."""
    return x_in @ w2.t(), x_in.abs() @ w2.abs().t()


def cat_forward(raw, mean, rstd, x_in, w2, mean2, rstd2, slope):
    xh = (raw - mean) * rstd
    r2, r2a = xbranch(x_in, w2)
    d2 = r2 - mean2
    T2 = r2a + mean2.abs()                               # what x2 - mean2 combines: its f32 value is off by <= 4 u T2
    flagged = d2.abs() <= 4 * U * r2a                    # the sign of xhat2 is not decided by the f32 evaluation
    xh2 = d2 * rstd2
    y1, y2 = lrelu(xh, slope), lrelu(xh2, slope)
    f2 = torch.where((xh2 > 0) | flagged, torch.ones_like(xh2), torch.full_like(xh2, slope))
    # 7 roundings: x2 (2 products, 1 addition), - mean2, * rstd2, * slope, the final addition; the first branch has 4
    return {"out": y1 + y2, "A": y1.abs() + f2 * rstd2 * T2, "K": 7, "xh": xh, "xh2": xh2, "xh2_err": rstd2 * T2,
            "flagged": flagged}


def pool_windows(t):
    """[D, H, W, C] -> [Vo, 8, C]: the eight voxels of every 2x2x2 window, k = 4 (z & 1) + 2 (y & 1) + (x & 1)."""
    D, H, W, C = t.shape
    return t.reshape(D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 2, 4, 1, 3, 5, 6).reshape(-1, 8, C)


def unpool_windows(w, D, H, W):
    C = w.shape[2]
    return w.reshape(D // 2, H // 2, W // 2, 2, 2, 2, C).permute(0, 3, 1, 4, 2, 5, 6).reshape(D, H, W, C)


def pool_first_max(t):
    """(maximum [Vo, C], position of the FIRST maximum in z-y-x order [Vo, C], windows whose maximum occurs twice [Vo, C])."""
    w = pool_windows(t)
    m = w.max(1).values
    eq = w == m[:, None]
    k = torch.arange(8, device=t.device)[None, :, None]
    first = torch.where(eq, k, torch.full_like(k, 8)).min(1).values
    return m, first, eq.sum(1) > 1


def decode_words(words, C):
    """argmax words [Vo, C / 8] int32 -> positions [Vo, C]."""
    sh = 3 * torch.arange(8, device=words.device)
    return ((words.long()[..., None] >> sh) & 7).reshape(words.shape[0], C)


def route_pool_grad(g_pool, idx, D, H, W):
    """Pooled gradient [Do, Ho, Wo, C] -> [D, H, W, C] at the flat voxel indices idx [Do, Ho, Wo, C] (max_pool3d's indices)."""
    C = g_pool.shape[3]
    full = torch.zeros(D * H * W, C, dtype=g_pool.dtype, device=g_pool.device)
    full.scatter_add_(0, idx.reshape(-1, C), g_pool.reshape(-1, C))
    return full.reshape(D, H, W, C)


def cat_backward(fw, gy, gy_abs, slope):
    """Per-sample sums of the aggregation block's backward for the total upstream gradient gy [V, C]."""
    xh, xh2, fl = fw["xh"], fw["xh2"], fw["flagged"]
    f1 = torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, slope))
    f2 = torch.where(xh2 > 0, torch.ones_like(xh2), torch.full_like(xh2, slope))
    d1, d2 = gy * f1, gy * f2
    d1a, d2a = gy_abs * f1, gy_abs * torch.where(fl, torch.ones_like(f2), f2)
    return {"d1": d1, "d2": d2, "d1_abs": d1a, "d2_abs": d2a, "flip": torch.where(fl, gy_abs, torch.zeros_like(gy_abs))}


# ---- trilinear x2^l interpolation, align_corners=True ---------------------------------------------------------------------
def _ac_src(n_in, n_out, device, f32_weights):
    """Source coordinate of every output index (float64 values) with the scale formed in float32 or float64."""
    ft = torch.float32 if f32_weights else torch.float64
    scale = (torch.tensor(float(n_in - 1), device=device, dtype=ft) / torch.tensor(float(n_out - 1), device=device, dtype=ft)
             if n_out > 1 else torch.zeros((), device=device, dtype=ft))
    return scale.double() * torch.arange(n_out, device=device, dtype=torch.float64)


def ac_matrix(n_in, n_out, device, f32_weights):
    """[n_out, n_in] float64 interpolation matrix.  f32_weights: scale = (in - 1) / (out - 1) is the float32 quotient the kernels
    form, and src = scale * o, lambda = src - floor(src) are exact from there.  The kernels round src once more (or not: the
    compiler may contract ``scale * o - i0`` into one fma, differently per kernel), so their lambda is within u src <=
    u (in - 1) of this one (the one rounding of the product; the quotient is the same correctly rounded f32 number here and
    there): ``lambda_term`` below is the bound of what that does to a result.  Otherwise float64 throughout, which is what F.interpolate computes for a float64 tensor."""
    src = _ac_src(n_in, n_out, device, f32_weights)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    lam = src - i0.double()
    M = torch.zeros(n_out, n_in, dtype=torch.float64, device=device)
    r = torch.arange(n_out, device=device)
    M.index_put_((r, i0), 1.0 - lam, accumulate=True)
    M.index_put_((r, i1), lam, accumulate=True)
    return M


def ac_band(n_in, n_out, device):
    """[n_out, n_in] ones wherever an input index is within one (and a little) of the output's source coordinate: every input a
    kernel can give weight to, whichever side of an integer its rounded coordinate falls."""
    src = _ac_src(n_in, n_out, device, True)
    i = torch.arange(n_in, device=device, dtype=torch.float64)
    return ((i[None, :] - src[:, None]).abs() <= 1 + 1e-4).double()


def apply3(t, Mz, My, Mx):
    """t [D, H, W, C] -> [Mz rows, My rows, Mx rows, C]: the separable linear map along the three axes."""
    D, H, W, C = t.shape
    t = (Mz @ t.reshape(D, -1)).reshape(Mz.shape[0], H, W * C)
    t = torch.matmul(My, t).reshape(Mz.shape[0] * My.shape[0], W, C)
    return torch.matmul(Mx, t).reshape(Mz.shape[0], My.shape[0], Mx.shape[0], C)


def upsample(t, factor=2, f32_weights=True, transpose=False):
    """x factor trilinear interpolation of t [D, H, W, C] (or, transpose=True, its adjoint applied to a fine tensor)."""
    D, H, W, _ = t.shape
    if transpose:
        D, H, W = D // factor, H // factor, W // factor
    Ms = [ac_matrix(n, n * factor, t.device, f32_weights) for n in (D, H, W)]
    if transpose:
        Ms = [M.t().contiguous() for M in Ms]
    return apply3(t, *Ms)


def lambda_term(t_abs, factor=2, transpose=False):
    """Bound of what a lambda off by d does to an interpolated value, divided by u: along each axis the two neighbours' weights
    move by d <= u (n_in - 1), so the value moves by at most d times the sum of the magnitudes in reach along that axis,
    interpolated normally along the other two.  Returns sum_axes (n_in - 1) B_axis(|t|) (multiply by u)."""
    D, H, W, _ = t_abs.shape
    if transpose:
        D, H, W = D // factor, H // factor, W // factor
    Ms = [ac_matrix(n, n * factor, t_abs.device, True) for n in (D, H, W)]
    Bs = [ac_band(n, n * factor, t_abs.device) for n in (D, H, W)]
    if transpose:
        Ms, Bs = [M.t().contiguous() for M in Ms], [B.t().contiguous() for B in Bs]
    out = 0
    for ax, n in enumerate((D, H, W)):
        mats = [Bs[k] if k == ax else Ms[k] for k in range(3)]
        out = out + (n - 1) * apply3(t_abs, *mats)
    return out


def max_taps(n_in, factor, device):
    """Most fine indices that can feed one coarse index along an axis (the length of the adjoint's summation chain)."""
    return int(ac_band(n_in, n_in * factor, device).sum(0).max())
