"""The loss kernels of a training step (csrc/loss.hip: the two-stage reduction to the seven whole-batch sums, the one-launch
value kernel, the fused gradient kernel) at the benchmarked shape and at the sizes where a reduction or a grid-stride loop goes
wrong, against the float64 restatement tests/loss_ref.py under DERIVED bounds -- and bitwise wherever float32 arithmetic is
exact or the operation is elementwise.

Tolerances (u = 2^-24; every count is justified in tests/loss_ref.py).  None is a fraction of max|ref|:
  bitwise        sums 0, 1, 2, 5, 6 of dyadic inputs against int64 arithmetic on the CPU (``test_exact_sums``); the ``terms``
                 specialisations against the full form; run to run; any prior contents of ``partial``; batch halves added in
                 f64; the value against the restatement's value from the kernel's own sums; the gradient for a misaligned
                 pointer against the aligned evaluation; a power-of-two upstream scale; exact zeros where the logit saturates
  sum bound      |got - ref| <= (L + K) u S               (L: depth of the f32 additions at that n, K: roundings in a term)
  element bound  |got - ref| <= K u mag                   (probability entry)
                 |got - ref| <= u mag (K p (1 - p) + K_P p) + (1 + mag) 2^-126      (logit entry)
                 plus, end to end, what the sum bound propagates into the ratio (value) or the coefficients (gradient)

Why the exact sums are exact.  p = k / 256 (k = 0..256), t and s in {0, 1}, w in {1, 2}: every term of sums 0, 1, 2, 5, 6 and
every intermediate (p s <= 1, p s + s <= 2, times w <= 4) is a multiple of 2^-8 not above 4 = 2^10 units.  A thread adds at
most 4 x 8 terms here (n <= 2^23 = 4 x 128^3, the largest case: 8 trips of the 16-byte path), a block has 256 threads: every
partial a thread, a wave or a block can form is at most 256 x 32 x 2^10 = 2^23 < 2^24 units, so every float32 addition is
exact in any order; the final pass is float64, exact up to 2^53 units.  The total (up to 2^33 units) is far beyond 2^24, so a final
pass in float32 would round.  A dropped or doubled element, float4 or block moves a sum by whole units.

One case's tensors are alive at a time; the float64 reference runs on the GPU (see tests/loss_ref.py for why that is sound)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = R.U
MIX = (0.3, 1.0, 0.5)
COEFS = {"dice": (1.0, 0.0, 0.0), "gul": (0.0, 1.0, 0.0), "atr": (0.0, 0.0, 1.0), "mix": MIX}
STAGE_COEF = {1: ((1.0, 0.0, 0.0), (1.0, 0.0, 0.0)), 2: ((0.0, 1.0, 0.0), (0.0, 0.5, 0.0)), 3: ((0.0, 1.0, 0.5), (0.0, 0.5, 0.5))}
EXACT = [0, 1, 2, 5, 6]
ROUNDED = [3, 4]
BENCH = (4, 1, 128, 128, 128)
SHAPES = {"bench": (BENCH, BENCH), "config4": ((1, 1, 160, 160, 160),) * 2, "3class": ((2, 3, 64, 64, 64), (2, 1, 64, 64, 64)),
          "ragged": ((1, 1, 31, 33, 35),) * 2}
# flat sizes: n4 = 1024 * 256 * k and one float4 either side (k = 1, 2: the reduction's full stride; k = 4 = 4096 * 256: the
# gradient's grid clamp), and the clamp in elements for the scalar path (odd n)
SIZES = {f"{k}stride{d:+d}": 4 * (R.STRIDE * k + d) for k in (1, 2, 4) for d in (-1, 0, 1)}
SIZES.update({"clamp-1": R.GRAD_THREADS - 1, "clamp+1": R.GRAD_THREADS + 1, "2stride+3": 2 * R.STRIDE + 3})
CASES = list(SHAPES) + list(SIZES)
SOFT_SUMS = ("bench", "3class", "ragged", "2stride+1", "2stride+3")       # soft labels run on a subset of the sizes
SOFT_GRAD = ("bench", "3class", "ragged")
assert SIZES["4stride+0"] == 4 * R.GRAD_THREADS and all(n % 2 for k, n in SIZES.items() if k[0] in "c")


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def shapes_of(case):
    return SHAPES[case] if case in SHAPES else ((SIZES[case],), (SIZES[case],))


def is_vec(*tensors):
    """The kernels' own rule for the 16-byte path."""
    return tensors[0].numel() % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def misaligned(t):
    """The same values at a pointer that is 4 bytes past a 16-byte boundary."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    base[1:].copy_(t.reshape(-1))
    out = base[1:]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# ---- the C ABI, one call each --------------------------------------------------------------------------------------------------
def k_sums(L, p, t, w, s, sig, terms=0, partial=None):
    from seunet_amd import _lib
    n = p.numel()
    assert all(v is None or (v.numel() == n and v.dtype == torch.float32 and v.is_contiguous() and v.is_cuda) for v in (p, t, w, s))
    if partial is None:
        partial = torch.empty(L.seunet_loss_partial_floats(), dtype=torch.float32, device=p.device)
    assert partial.numel() >= L.seunet_loss_partial_floats()
    out = torch.empty(R.NSUMS, dtype=torch.float64, device=p.device)
    _lib.check(L.seunet_loss_sums(p.data_ptr(), int(sig), t.data_ptr(), _lib.ptr(w), _lib.ptr(s), n, partial.data_ptr(),
                                  out.data_ptr(), int(terms), _lib.stream_ptr()), "loss_sums")
    return out


def k_grad(L, p, t, w, s, sig, sums, coef, g_scale=1.0, g_dev=None, out=None):
    from seunet_amd import _lib
    n = p.numel()
    out = torch.empty(n, dtype=torch.float32, device=p.device) if out is None else out
    assert all(v is None or (v.numel() == n and v.dtype == torch.float32 and v.is_contiguous() and v.is_cuda) for v in (p, t, w, s, out))
    assert sums.dtype == torch.float64 and sums.numel() == R.NSUMS and sums.is_contiguous()
    _lib.check(L.seunet_loss_grad(p.data_ptr(), int(sig), t.data_ptr(), _lib.ptr(w), _lib.ptr(s), n, sums.data_ptr(),
                                  coef[0], coef[1], coef[2], g_scale, _lib.ptr(g_dev), out.data_ptr(), _lib.stream_ptr()), "loss_grad")
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def planted(n, vec):
    """Element positions a wrong loop bound or a wrong block offset misses: the first and last element, the last float4 (element)
    of every stride trip, the first element of every block's second trip, both sides of the gradient grid's clamp."""
    per = 4 if vec else 1
    stride = R.STRIDE * per
    pos = {0, n - 1, n - per}
    for j in range(1, n // stride + 2):
        pos.update((j * stride - 1, j * stride - per, j * stride))
    pos.update(stride + b * 256 * per for b in range(1024))
    pos.update((R.GRAD_THREADS * per - 1, R.GRAD_THREADS * per))
    return torch.tensor(sorted(q for q in pos if 0 <= q < n), dtype=torch.long)


def dyadic_inputs(shape, lshape, seed):
    """int64 (P, t, w, s) on the CPU with p = P / 256: noise, a per-sample offset of p, a per-sample slab of label, and the
    planted positions (both paths' positions, whichever path runs) at p = 255/256, t = s = 1, w = 2 amid a zeroed float4."""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for d in shape:
        n *= d
    samples = shape[0] if len(shape) > 1 else 1
    P = torch.randint(0, 257, shape, generator=g)
    P = ((P.reshape(samples, -1) + 37 * torch.arange(samples)[:, None]) % 257).reshape(shape)
    t = (torch.randint(0, 8, lshape, generator=g) == 0).long()
    for i, ti in enumerate(t.reshape(samples, -1)):
        ti[i * 1000:i * 1000 + ti.numel() // 7] = 1
    t = torch.broadcast_to(t, shape).contiguous()
    s = t * torch.randint(0, 2, shape, generator=g)
    w = 1 + torch.randint(0, 2, shape, generator=g)
    pos = torch.cat([planted(n, True), planted(n, False)]).unique()
    for v, plant in ((P, 255), (t, 1), (s, 1), (w, 2)):
        flat = v.reshape(-1)
        quad = (pos // 4 * 4)[:, None] + torch.arange(4)
        flat[quad[quad < n]] = 0 if plant != 2 else 1
        flat[pos] = plant
    return P, t, w, s


def int_sums(P, t, w, s):
    """The seven sums in units of 2^-8 by int64 arithmetic (entries 3 and 4 unused), as the float64 numbers they are."""
    S = [int((P * t).sum()), int(P.sum()), 256 * int(t.sum()), 0, 0, int((w * P * s * s).sum()), int((w * (P * s + 256 * s)).sum())]
    return torch.tensor([v / 256.0 for v in S], dtype=torch.float64)


def dev(v):
    return None if v is None else v.reshape(-1).float().cuda()


def real_inputs(shape, lshape, seed, soft=False):
    """Flat f32 device tensors (logits, label, weight, skeleton): logits N(offset_sample, 3^2) with planted +-100 (first and
    last element and every 4099th), 3 % foreground plus a per-sample slab (or soft labels in (0, 1)), w in [1, 2), a skeleton
    inside the label; the label broadcast over the class axis as losses.py does."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(shape, device="cuda", generator=g) * 3
    samples = shape[0] if len(shape) > 1 else 1
    x = (x.reshape(samples, -1) + torch.linspace(-1, 1, samples, device="cuda")[:, None]).reshape(-1)
    x[::4099] = 100.0
    x[2049::4099] = -100.0
    x[-1] = -100.0
    if soft:
        t = torch.rand(lshape, device="cuda", generator=g).clamp(1e-3, 1 - 1e-3)
    else:
        t = (torch.rand(lshape, device="cuda", generator=g) < 0.03).float()
        for i, ti in enumerate(t.reshape(samples, -1)):
            ti[i * 1000:i * 1000 + ti.numel() // 50] = 1.0
    t = torch.broadcast_to(t, shape).contiguous().reshape(-1)
    w = 1 + torch.rand(shape, device="cuda", generator=g).reshape(-1)
    s = t * (torch.rand(shape, device="cuda", generator=g).reshape(-1) > 0.5).float()
    return x, t, w, s


def d64(*ts):
    return [None if v is None else v.double() for v in ts]


def assert_within(got, ref, lim, what):
    """|got - ref| <= lim elementwise, reporting the worst ratio and where."""
    err = (got.double() - ref).abs()
    bad = ~(err <= lim)                                       # (NaN on either side fails)
    if bool(bad.any()):
        ratio = torch.where(bad, err / lim.clamp(min=1e-300) if torch.is_tensor(lim) else err / lim, torch.zeros_like(err))
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} outside the bound; worst at {i}: got "
                             f"{float(got.reshape(-1)[i]):.9e} ref {float(ref.reshape(-1)[i]):.9e} "
                             f"|diff| {float(err.reshape(-1)[i]):.3e} = {float(ratio.reshape(-1)[i]):.2f} x bound")


# ---- (a) sums that are exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_exact_sums(L, case):
    shape, lshape = shapes_of(case)
    Pi, ti, wi, si = dyadic_inputs(shape, lshape, seed=11)
    want = int_sums(Pi, ti, wi, si)
    p, t, w, s = dev(Pi / 256.0), dev(ti), dev(wi), dev(si)
    n = p.numel()
    assert n <= 2 ** 23 and bool((p * 256 == p.mul(256).round()).all())
    full = k_sums(L, p, t, w, s, 0, terms=7)
    assert torch.equal(full[EXACT].cpu(), want[EXACT]), (full.cpu() - want).tolist()
    ref34 = R.sums(*d64(p, t, w, s))
    assert_within(full[ROUNDED], ref34[ROUNDED], R.sum_bound(ref34, n, is_vec(p, t, w, s), False)[ROUNDED], "sums 3, 4")
    # two runs; any prior contents of the block partials
    assert torch.equal(k_sums(L, p, t, w, s, 0, terms=7), full)
    nan = torch.full((L.seunet_loss_partial_floats(),), float("nan"), dtype=torch.float32, device="cuda")
    assert torch.equal(k_sums(L, p, t, w, s, 0, terms=7, partial=nan), full) and not bool(torch.isnan(nan).any())
    # the specialisations: shared sums bitwise, sums that were not asked for exactly zero; 0 / 3 / 4 / 5 are the full form
    # (regression: with the contraction of 0.2 p + 0.8 t left to the compiler, sum 4 of <2> was 1e-9 off <6> and <7>)
    for terms, have in ((1, [0, 1, 2]), (2, [3, 4]), (6, [3, 4, 5, 6])):
        got = k_sums(L, p, t, w, s, 0, terms=terms)
        rest = [k for k in range(R.NSUMS) if k not in have]
        assert torch.equal(got[have], full[have]), (terms, (got - full).tolist())
        assert bool((got[rest] == 0.0).all()) and not bool(torch.signbit(got[rest]).any()), (terms, got.tolist())
    for terms in (0, 3, 4, 5):
        assert torch.equal(k_sums(L, p, t, w, s, 0, terms=terms), full), terms
    # no weight map is weight 1, no skeleton is skeleton 0 (on the 16-byte path and on the scalar path alike)
    got = k_sums(L, p, t, None, None, 0)
    want1 = int_sums(Pi, ti, torch.ones_like(wi), torch.zeros_like(si))
    assert torch.equal(got[EXACT].cpu(), want1[EXACT]) and float(got[5]) == 0.0 and float(got[6]) == 0.0
    got = k_sums(L, p, t, None, s, 0)
    assert torch.equal(got[EXACT].cpu(), int_sums(Pi, ti, torch.ones_like(wi), si)[EXACT])
    # the data-parallel identity of losses._reduce: the two halves of the batch (of the flat array), added in f64
    h = n // 2 if len(shape) > 1 and shape[0] > 1 else n // 8 * 4
    halves = [k_sums(L, *[v[a:b] for v in (p, t, w, s)], 0) for a, b in ((0, h), (h, n))]
    both = halves[0] + halves[1]
    assert torch.equal(both[EXACT], full[EXACT])
    lim = 2 * torch.maximum(R.sum_bound(ref34, n, True, False), R.sum_bound(ref34, n, False, False))
    assert_within(both[ROUNDED], full[ROUNDED], lim[ROUNDED], "halves, sums 3, 4")
    # a misaligned pointer (scalar path) sums the same elements
    if len(shape) == 1 or case == "ragged":
        for which in range(4):
            args = [misaligned(v) if k == which else v for k, v in enumerate((p, t, w, s))]
            assert not is_vec(*args)
            assert torch.equal(k_sums(L, *args, 0)[EXACT].cpu(), want[EXACT]), which


# ---- (b) sums that round ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,soft", [(c, False) for c in CASES] + [(c, True) for c in SOFT_SUMS],
                         ids=lambda v: v if isinstance(v, str) else ("soft" if v else "binary"))
def test_rounding_sums(L, case, soft):
    shape, lshape = shapes_of(case)
    x, t, w, s = real_inputs(shape, lshape, seed=21, soft=soft)
    n, vec = x.numel(), is_vec(x, t, w, s)
    p32 = torch.sigmoid(x)
    for logits, src, p64 in ((False, p32, p32.double()), (True, x, R.sigmoid(x.double()))):
        ref = R.sums(p64, *d64(t, w, s))
        lim = R.sum_bound(ref, n, vec, logits)
        got = k_sums(L, src, t, w, s, logits)
        assert_within(got, ref, lim, f"sums, logits={logits}")
        assert torch.equal(k_sums(L, src, t, w, s, logits), got)
        if vec:                                          # the scalar path on the same values
            assert_within(k_sums(L, misaligned(src), t, w, s, logits), ref, R.sum_bound(ref, n, False, logits), "misaligned pred")
            assert_within(k_sums(L, src, misaligned(t), w, s, logits), ref, R.sum_bound(ref, n, False, logits), "misaligned label")
    if case == "bench":                                  # torch's float64 reduction on the GPU is the CPU's
        cpu = R.sums(R.sigmoid(x.double().cpu()), *[v.cpu() for v in d64(t, w, s)])
        assert_within(ref.cpu(), cpu, 1e-12 * cpu, "float64 sums, GPU against CPU")


# ---- (d) the gradient kernel alone -----------------------------------------------------------------------------------------------
def check_grad(got, src, t, w, s, S_kernel, coef, logits, scale=1.0, what=""):
    """Element bound against the restatement given the kernel's own sums; finite; zero where the logit saturates."""
    x64, t64, w64, s64 = d64(src, t, w, s)
    if logits:
        ref, mag, _, p, ds = R.grad_logit(x64, t64, w64, s64, S_kernel, coef, scale)
        lim = R.grad_bound_logit(mag, p, ds, coef)
        sat = (src >= 20) | (src <= -90)                   # 1 + e^-20 == 1 in f32; e^90 overflows
        assert bool((got[sat] == 0).all()), what
    else:
        ref, mag, _ = R.grad_pred(x64, t64, w64, s64, S_kernel, coef, scale)
        lim = R.grad_bound_pred(mag, coef)
    assert bool(torch.isfinite(got).all()), what
    assert_within(got, ref, lim, what)


@pytest.mark.parametrize("case,soft", [(c, False) for c in CASES] + [(c, True) for c in SOFT_GRAD],
                         ids=lambda v: v if isinstance(v, str) else ("soft" if v else "binary"))
def test_gradient_kernel(L, case, soft):
    shape, lshape = shapes_of(case)
    x, t, w, s = real_inputs(shape, lshape, seed=31, soft=soft)
    n, vec = x.numel(), is_vec(x, t, w, s)
    p32 = torch.sigmoid(x)
    p32[::4099] = 1.0                                    # probabilities that are exactly 0 and 1
    p32[2049::4099] = 0.0
    for logits, src in ((False, p32), (True, x)):
        S = k_sums(L, src, t, w, s, logits)
        p64 = R.sigmoid(src.double()) if logits else src.double()
        S64 = R.sums(p64, *d64(t, w, s))
        eS = R.sum_bound(S64, n, vec, logits)
        assert_within(S, S64, eS, "sums")
        for name, coef in COEFS.items():
            got = k_grad(L, src, t, w, s, logits, S, coef)
            check_grad(got, src, t, w, s, S.cpu(), coef, logits, what=f"{name} logits={logits}")
            # end to end: float64 sums, and what the sums' error does to the coefficients
            if logits:
                ref, mag, prop, p, ds = R.grad_logit(*d64(src, t, w, s), S64.cpu(), coef, sum_err=eS.cpu())
                lim = R.grad_bound_logit(mag, p, ds, coef) + prop
            else:
                ref, mag, prop = R.grad_pred(*d64(src, t, w, s), S64.cpu(), coef, sum_err=eS.cpu())
                lim = R.grad_bound_pred(mag, coef) + prop
            assert_within(got, ref, lim, f"{name} logits={logits} end to end")
            # no weight map / no skeleton: the gradient of weight 1 / skeleton 0
            if name == "mix":
                one, zero = torch.ones_like(w), torch.zeros_like(s)
                S1 = k_sums(L, src, t, None, None, logits)
                assert torch.equal(S1, k_sums(L, src, t, one, zero, logits))
                assert torch.equal(k_grad(L, src, t, None, None, logits, S1, coef), k_grad(L, src, t, one, zero, logits, S1, coef))
                assert torch.equal(k_grad(L, src, t, None, s, logits, S1, coef), k_grad(L, src, t, one, s, logits, S1, coef))
        # the upstream scale: g_scale x g_scale_dev[0]
        g1 = k_grad(L, src, t, w, s, logits, S, MIX)
        half, three = torch.tensor([0.5], device="cuda"), torch.tensor([3.0], device="cuda")
        g2 = k_grad(L, src, t, w, s, logits, S, MIX, g_scale=65536.0, g_dev=half)
        normal = g1.abs() >= 2.0 ** -126
        assert torch.equal(g2[normal], g1[normal] * 32768.0)           # a power of two: the same bits, another exponent
        assert_within(g2, g1.double() * 32768.0, torch.full_like(g1, 32768.0 * 2.0 ** -149, dtype=torch.float64), "scale 2^15")
        g3 = k_grad(L, src, t, w, s, logits, S, MIX, g_scale=3.0)
        assert torch.equal(k_grad(L, src, t, w, s, logits, S, MIX, g_scale=1.0, g_dev=three), g3)
        assert torch.equal(k_grad(L, src, t, w, s, logits, S, MIX, g_scale=1.5, g_dev=half * 4.0), g3)
        if logits:       # (3 g) s against 3 (g s): three roundings apart (3.001: their second order)
            assert_within(g3, g1.double() * 3.0, 3.001 * U * (g1.double() * 3.0).abs() + 8 * 2.0 ** -149, "scale 3")
        else:            # the scale is the last operation: one rounding of 3 g
            assert torch.equal(g3, g1 * 3.0)
        check_grad(g3, src, t, w, s, S.cpu(), MIX, logits, scale=3.0, what="scale 3 against the restatement")
        # a misaligned pointer, one array at a time (the output among them): elementwise, so the same bits
        if vec:
            arrays = (src, t, w, s)
            for which in range(5):
                args = [misaligned(v) if k == which else v for k, v in enumerate(arrays)]
                out = misaligned(torch.zeros_like(g1)) if which == 4 else None
                assert torch.equal(k_grad(L, *args, logits, S, MIX, out=out), g1), which


# ---- (c) value, and the public entry points --------------------------------------------------------------------------------------
def prep(v, like):
    return None if v is None else torch.broadcast_to(v.float(), like.shape).contiguous()


def check_head(grad, pred, t, w, s, coef, logits, scale=1.0, what=""):
    """One head through the public API: its gradient against the restatement from the kernel's own sums (element bound) and from
    float64 sums (plus the propagated sum error).  Returns (kernel sums, float64 sums, their bound).  ``pred`` is what was
    passed (any dtype / layout); the library converts it to contiguous f32 and so does the reference."""
    from seunet_amd import losses
    pf = pred.detach().contiguous().float()
    tt, ww, ss = prep(t, pf), prep(w, pf), prep(s, pf)
    n, vec = pf.numel(), is_vec(pf, tt, ww, ss)
    S = losses._sums(pf, logits, tt, ww, ss, None, losses._terms(*coef))
    p64 = R.sigmoid(pf.double()) if logits else pf.double()
    S64 = R.sums(p64, *d64(tt, ww, ss))
    eS = R.sum_bound(S64, n, vec, logits)
    active = [k for k in range(R.NSUMS) if coef[(0, 0, 0, 1, 1, 2, 2)[k]]]
    assert_within(S[active], S64[active], eS[active], what + " sums")
    if losses._terms(*coef) in (1, 2, 6):                 # the specialised instantiations; any other mask runs the full form
        idle = [k for k in range(R.NSUMS) if k not in active]
        assert bool((S[idle] == 0).all())
    if grad is not None:
        assert grad.shape == pred.shape and grad.dtype == pred.dtype
        half_ulp = lambda r, e: 0.5 * R.storage_ulp(r.abs() + e, pred.dtype)      # noqa: E731  (16-bit pred: autograd rounds the gradient to it)
        for sums, err in ((S, None), (S64, eS)):
            if logits:
                ref, mag, prop, p, ds = R.grad_logit(pf.double(), *d64(tt, ww, ss), sums.cpu(), coef, scale, None if err is None else err.cpu())
                lim = R.grad_bound_logit(mag, p, ds, coef) + prop
            else:
                ref, mag, prop = R.grad_pred(pf.double(), *d64(tt, ww, ss), sums.cpu(), coef, scale, None if err is None else err.cpu())
                lim = R.grad_bound_pred(mag, coef) + prop
            assert bool(torch.isfinite(grad).all()), what
            assert_within(grad.contiguous(), ref, lim + half_ulp(ref, lim), what + (" gradient" if err is None else " gradient end to end"))
        if logits:
            sat = (pf >= 20) | (pf <= -90)
            assert bool((grad.contiguous()[sat] == 0).all()), what
    return S, S64, eS


def check_value(loss, heads, what):
    """heads: [(kernel sums, float64 sums, bound, coef)].  Bitwise against the restatement's value from the kernel's sums;
    against the float64 value under the propagated bound (and one f32 rounding for the addition of two heads)."""
    assert loss.dtype == torch.float32 and loss.dim() == 0
    want = R.value_f32(heads[0][0].cpu(), heads[0][3], *((heads[1][0].cpu(), heads[1][3]) if len(heads) > 1 else ()))
    assert torch.equal(loss.detach().cpu(), want), (what, float(loss.detach()), float(want))
    ref = sum(float(R.value(S64.cpu(), coef)) for _, S64, _, coef in heads)
    lim = sum(R.value_bound(S64, eS, coef) for _, S64, eS, coef in heads)
    if len(heads) > 1:
        lim += U * (abs(ref) + lim)
    err = abs(float(loss.detach()) - ref)
    assert err <= lim, f"{what}: value {float(loss.detach()):.9e} ref {ref:.9e} |diff| {err:.3e} > {lim:.3e}"


def shaped(shape, lshape, seed, soft=False):
    x, t, w, s = real_inputs(shape, lshape, seed, soft)
    return x.reshape(shape), t.reshape(shape)[:, :1].contiguous() if shape != lshape else t.reshape(shape), w.reshape(shape), s.reshape(shape)


@pytest.mark.parametrize("case", ("bench", "3class"))
@pytest.mark.parametrize("stage", (1, 2, 3))
def test_fused_stage_loss(L, case, stage):
    import seunet_amd as A
    shape, lshape = SHAPES[case]
    xe, t, w, s = shaped(shape, lshape, seed=41)
    xd = (xe * 0.5 + 0.1)
    xd.reshape(-1)[::4099] = -100.0
    xe.requires_grad_(), xd.requires_grad_()
    loss = A.fused_stage_loss(stage, xe, xd, t, w, s)
    loss.backward()
    cd, ce = STAGE_COEF[stage]
    sk = None if stage == 2 else s
    heads = [check_head(xd.grad, xd, t, w, sk, cd, True, what=f"stage {stage} decoder head") + (cd,),
             check_head(xe.grad, xe, t, w, sk, ce, True, what=f"stage {stage} encoder head") + (ce,)]
    check_value(loss, heads, f"stage {stage}")


@pytest.mark.parametrize("soft", (False, True), ids=("binary", "soft"))
@pytest.mark.parametrize("case", ("bench", "3class", "ragged"))
@pytest.mark.parametrize("name", ("dice_loss", "general_union_loss_lib", "atr_loss", "fused_logit_loss"))
def test_public_losses(L, name, case, soft):
    """The three reference-signature losses (probabilities in) and a coefficient mix from logits; the upstream gradient 3."""
    import seunet_amd as A
    shape, lshape = SHAPES[case]
    x, t, w, s = shaped(shape, lshape, seed=51, soft=soft)
    logits = name == "fused_logit_loss"
    pred = (x if logits else torch.sigmoid(x)).requires_grad_()
    if name == "dice_loss":
        loss, coef, ww, ss = A.dice_loss(pred, t), COEFS["dice"], None, None
    elif name == "general_union_loss_lib":
        loss, coef, ww, ss = A.general_union_loss_lib(pred, t, w), COEFS["gul"], w, None
    elif name == "atr_loss":
        loss, coef, ww, ss = A.atr_loss(pred, t, s, w), COEFS["atr"], w, s
    else:
        loss, coef, ww, ss = A.fused_logit_loss(pred, t, w, s, *MIX), MIX, w, s
    (3.0 * loss).backward()
    head = check_head(pred.grad, pred, t, ww, ss, coef, logits, scale=3.0, what=name)
    check_value(loss, [head + (coef,)], name)
    # the unscaled gradient times 3, to the roundings that separate them
    g3 = pred.grad.clone()
    pred.grad = None
    getattr(A, name)(*{"dice_loss": (pred, t), "general_union_loss_lib": (pred, t, w), "atr_loss": (pred, t, s, w),
                       "fused_logit_loss": (pred, t, w, s) + MIX}[name]).backward()
    if logits:
        assert_within(g3, pred.grad.double() * 3.0, 3.001 * U * (pred.grad.double() * 3.0).abs() + 8 * 2.0 ** -149, "3 x loss")
    else:
        assert torch.equal(g3, pred.grad * 3.0)


def test_misaligned_through_the_public_api(L):
    """A 1-D f32 tensor sliced [1:] is contiguous f32, so losses.py passes its pointer on: the scalar path, through ``pred`` and
    through ``label``."""
    import seunet_amd as A
    n = 4 * R.STRIDE + 4
    x, t, w, s = real_inputs((n,), (n,), seed=61)
    ref_loss = None
    for which in ("aligned", "pred", "label"):
        base = torch.zeros(n + 1, device="cuda")
        base[1:] = x
        base.requires_grad_()
        pred = base[1:] if which == "pred" else base[1:] + 0.0          # (+ 0.0: a fresh, aligned tensor of the same values)
        tt = misaligned(t) if which == "label" else t
        assert (pred.data_ptr() % 16 == 4) == (which == "pred") and (tt.data_ptr() % 16 == 4) == (which == "label")
        loss = A.fused_logit_loss(pred, tt, w, s, *MIX)
        loss.backward()
        assert float(base.grad[0]) == 0.0
        head = check_head(base.grad[1:], pred.detach(), tt, w, s, MIX, True, what=which)
        check_value(loss, [head + (MIX,)], which)
        if ref_loss is None:
            ref_loss, ref_S, ref_eS, ref_grad = loss.detach(), head[0], head[2], base.grad[1:].clone()
        else:        # against the aligned evaluation: the sums within the two sum bounds; the gradient within the two element
            # bounds and what that change of the sums propagates
            assert_within(head[0], ref_S, head[2] + ref_eS, which + " sums against aligned")
            xm = pred.detach()
            g, mag, prop, p, ds = R.grad_logit(*d64(xm, tt, w, s), ref_S.cpu(), MIX, sum_err=(head[2] + ref_eS).cpu())
            assert_within(base.grad[1:], ref_grad.double(), 2 * R.grad_bound_logit(mag, p, ds, MIX) + prop, which + " gradient against aligned")
            # and bitwise given the same sums
            assert torch.equal(k_grad(L, xm.contiguous(), tt, w, s, True, ref_S, MIX), k_grad(L, x, t, w, s, True, ref_S, MIX))


# ---- (e) edge inputs ---------------------------------------------------------------------------------------------------------------
EDGES = ("empty_label", "full_label", "soft_label", "zero_weights", "empty_skeleton", "skeleton_outside_label", "planted_100",
         "no_weight", "no_skeleton_with_atr", "bf16_pred", "fp16_pred", "noncontiguous_pred", "three_class")


@pytest.mark.parametrize("entry", ("logits", "probabilities"))
@pytest.mark.parametrize("edge", EDGES)
def test_edge_inputs(L, edge, entry):
    import seunet_amd as A
    shape = (2, 3, 64, 64, 64) if edge == "three_class" else (2, 1, 64, 64, 64)
    lshape = (2, 1, 64, 64, 64)
    x, t, w, s = shaped(shape, lshape, seed=71, soft=edge == "soft_label")
    if edge == "empty_label":
        t, s = torch.zeros_like(t), torch.zeros_like(s)
    elif edge == "full_label":
        t = torch.ones_like(t)
    elif edge == "zero_weights":
        w = w * (w > 1.5)
        w[0] = 0.0                                          # a whole sample without weight
    elif edge == "empty_skeleton":
        s = torch.zeros_like(s)
    elif edge == "skeleton_outside_label":
        s = (1 - torch.broadcast_to(t, shape)) * (w > 1.7)
    elif edge == "no_weight":
        w = None
    elif edge == "no_skeleton_with_atr":
        s = None
    elif edge == "bf16_pred":
        x = x.to(torch.bfloat16)
    elif edge == "fp16_pred":
        x = x.to(torch.float16)
    elif edge == "noncontiguous_pred":
        x = x.transpose(2, 4)
        assert not x.is_contiguous()
    logits = entry == "logits"
    if logits:
        pred = x.detach().clone().requires_grad_() if x.is_contiguous() else x.detach().requires_grad_()
        loss = A.fused_logit_loss(pred, t, w, s, *MIX)
        loss.backward()
        head = check_head(pred.grad, pred, t, w, s, MIX, True, what=edge)
        check_value(loss, [head + (MIX,)], edge)
        if edge == "empty_label":
            assert float(head[0][0]) == 0.0 and float(head[0][2]) == 0.0 and float(head[0][3]) == 0.0
        return
    p = torch.sigmoid(x.float()).to(x.dtype)
    p.reshape(-1)[::4099] = 1.0                             # (a view only when contiguous; the planted values are not needed otherwise)
    w1 = torch.ones(shape, device="cuda") if w is None else w
    s0 = torch.zeros(shape, device="cuda") if s is None else s
    for name, args, ww, ss in (("dice", (t,), None, None), ("gul", (t, w1), w1, None), ("atr", (t, s0, w1), w1, s0)):
        pred = p.detach().requires_grad_()
        loss = {"dice": A.dice_loss, "gul": A.general_union_loss_lib, "atr": A.atr_loss}[name](pred, *args)
        loss.backward()
        head = check_head(pred.grad, pred, t, ww, ss, COEFS[name], False, what=f"{edge} {name}")
        check_value(loss, [head + (COEFS[name],)], f"{edge} {name}")
