"""Per-sample loss sums and values (csrc/loss.hip ``loss_sample_sums_kernel`` / ``loss_sample_final_kernel`` /
``loss_sample_values_kernel``; ``seunet_amd.per_sample_loss``): the key of the online hard mining.

Reference: tests/loss_ref.py in float64, one sample at a time.  Tolerances are the derived bounds of that module with ITS
constants (u = 2^-24, K_SUM, K_P, F64_SUM, TINY) and the depth L of THIS kernel's additions:
    |got - ref| <= (L + K_SUM[k] (+ K_P)) u S + F64_SUM S (+ n TINY 4)
    L = 4 ceil((n / 4) / SAMPLE_STRIDE) + 9   on the 16-byte path,      ceil(n / SAMPLE_STRIDE) + 9   on the scalar path
(a thread's own additions, six butterfly steps, three additions over the block's four waves; the final pass is float64).
Values: ``loss_ref.value_bound`` of ``loss_ref.value`` with the sum bounds above.
Bitwise: a sample of a batch against the same sample computed alone; the general-union sums with ``terms = 2`` against
``terms = 7``; the value against the restatement's value from the kernel's own sums; run to run; and the dyadic case below.

Exact sums.  p = P / 256 (P = 0..256), t and s in {0, 1}, w in {1, 2}: every term of sums 0, 1, 2, 5, 6 is a multiple of 2^-8
not above 4 = 2^10 units, and a block adds at most 2 x 256 x 4 of them here (n <= 4 x SAMPLE_STRIDE + 4), below 2^24 units, so
every float32 addition is exact; they are compared with int64 arithmetic on the CPU.  Sum 4 = sum w (0.2 p + 0.8 t) is NOT
among them although the request for this test lists it: 0.2f and 0.8f are no dyadic fractions, 0.2f p already rounds, so
its partial sums are not exactly representable (tests/test_loss_layers_gpu.py treats it the same way for the whole-batch
kernel).  Sums 3 and 4 of the dyadic case stay under the derived bound.

Shapes: B in {1, 3, 4} x n in {32^3, 4096, 4099 (scalar path)} take one trip of the thread loop; two more cases take a second
trip on either path (n = 4 SAMPLE_STRIDE + 4 and SAMPLE_STRIDE + 3), which the 128^3 samples of training do eight times."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE_STRIDE = 256 * 256          # csrc/loss.hip: SAMPLE_STRIDE = SAMPLE_BLOCKS * 256, SAMPLE_BLOCKS = 256
MIX = (0.3, 1.0, 0.5)
GUL = (0.0, 1.0, 0.0)
EXACT, ROUNDED = [0, 1, 2, 5, 6], [3, 4]
CASES = [(B, n) for B in (1, 3, 4) for n in (32 ** 3, 4096, 4099)] + [(2, 4 * SAMPLE_STRIDE + 4), (2, SAMPLE_STRIDE + 3)]


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def is_vec(n, *tensors):
    """The kernel's own rule for the 16-byte path, per sample."""
    return n % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def k_sample_sums(L, p, t, w, s, sig, terms=0):
    """(B, 7) f64 from (B, n) f32 tensors."""
    from seunet_amd import _lib
    B, n = p.shape
    assert all(v is None or (v.shape == p.shape and v.dtype == torch.float32 and v.is_contiguous() and v.is_cuda) for v in (p, t, w, s))
    floats = L.seunet_loss_sample_partial_floats(B)
    assert floats == B * 256 * R.NSUMS
    partial = torch.full((floats,), float("nan"), dtype=torch.float32, device=p.device)       # any prior contents
    out = torch.full((B, R.NSUMS), float("nan"), dtype=torch.float64, device=p.device)
    _lib.check(L.seunet_loss_sums_per_sample(p.data_ptr(), int(sig), t.data_ptr(), _lib.ptr(w), _lib.ptr(s), B, n, partial.data_ptr(),
                                             out.data_ptr(), int(terms), _lib.stream_ptr()), "loss_sums_per_sample")
    return out


def k_sample_values(L, sums, coef):
    from seunet_amd import _lib
    B = sums.shape[0]
    out = torch.full((B,), float("nan"), dtype=torch.float32, device=sums.device)
    _lib.check(L.seunet_loss_sample_values(sums.data_ptr(), B, coef[0], coef[1], coef[2], out.data_ptr(), _lib.stream_ptr()), "loss_sample_values")
    return out


def sample_sum_bound(S, n, vec, logits):
    """[7] bound for one sample's float64 sums S: loss_ref.sum_bound with this kernel's depth."""
    depth = (4 * math.ceil((n // 4) / SAMPLE_STRIDE) if vec else math.ceil(n / SAMPLE_STRIDE)) + 6 + 3
    K = [k + (R.K_P if (logits and has_p) else 0.0) for k, has_p in zip(R.K_SUM, R.SUM_HAS_P)]
    rel = torch.tensor([(depth + k) * R.U + R.F64_SUM for k in K], dtype=torch.float64, device=S.device)
    return rel * S.abs() + (n * R.TINY * 4 if logits else 0.0)


def real_inputs(B, n, seed):
    """(B, n) f32 device tensors made like tests/test_loss_layers_gpu.py's: logits N(offset_sample, 3^2) with planted +-100,
    3 % foreground plus a per-sample slab, w in [1, 2), a skeleton inside the label."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((B, n), device="cuda", generator=g) * 3 + torch.linspace(-1, 1, B, device="cuda")[:, None]
    flat = x.reshape(-1)
    flat[::4099] = 100.0
    flat[2049::4099] = -100.0
    x[:, -1] = -100.0
    t = (torch.rand((B, n), device="cuda", generator=g) < 0.03).float()
    for i in range(B):
        t[i, i * 100:i * 100 + n // 50] = 1.0
    w = 1 + torch.rand((B, n), device="cuda", generator=g)
    s = t * (torch.rand((B, n), device="cuda", generator=g) > 0.5).float()
    return x.contiguous(), t, w, s


def assert_within(got, ref, lim, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= lim)
    if bool(bad.any()):
        ratio = torch.where(bad, err / lim.clamp(min=1e-300), torch.zeros_like(err))
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} outside the bound; worst at {i}: got {float(got.reshape(-1)[i]):.9e} "
                             f"ref {float(ref.reshape(-1)[i]):.9e} |diff| {float(err.reshape(-1)[i]):.3e} = {float(ratio.reshape(-1)[i]):.2f} x bound")


@pytest.mark.parametrize("B,n", CASES)
def test_sums_and_values(L, B, n):
    import seunet_amd as A
    x, t, w, s = real_inputs(B, n, seed=81)
    vec = is_vec(n, x, t, w, s)
    assert vec == (n % 4 == 0)
    p32 = torch.sigmoid(x)
    for logits, src, p64 in ((True, x, R.sigmoid(x.double())), (False, p32, p32.double())):
        ref = torch.stack([R.sums(p64[b], t[b].double(), w[b].double(), s[b].double()) for b in range(B)])
        lim = torch.stack([sample_sum_bound(ref[b], n, vec, logits) for b in range(B)])
        full = k_sample_sums(L, src, t, w, s, logits, terms=7)
        gul = k_sample_sums(L, src, t, w, s, logits, terms=2)
        for b in range(B):
            print(f"B={B} n={n} logits={logits} sample {b}: worst |diff| / bound = {float(((full[b] - ref[b]).abs() / lim[b].clamp(min=1e-300)).max()):.3f}")
        assert_within(full, ref, lim, f"sums, terms=7, logits={logits}")
        assert_within(gul[:, ROUNDED], ref[:, ROUNDED], lim[:, ROUNDED], f"sums, terms=2, logits={logits}")
        # what was not asked for is exactly +0; what was is the same bits whichever other sums come with it
        rest = [k for k in range(R.NSUMS) if k not in ROUNDED]
        assert bool((gul[:, rest] == 0).all()) and not bool(torch.signbit(gul[:, rest]).any())
        assert torch.equal(gul[:, ROUNDED], full[:, ROUNDED])
        assert torch.equal(k_sample_sums(L, src, t, w, s, logits, terms=0), full)
        assert torch.equal(k_sample_sums(L, src, t, w, s, logits, terms=7), full)                    # run to run
        # no weight map is weight 1, no skeleton is skeleton 0
        assert torch.equal(k_sample_sums(L, src, t, None, None, logits), k_sample_sums(L, src, t, torch.ones_like(w), torch.zeros_like(s), logits))
        # values: bitwise the restatement's value of the kernel's own sums; within the propagated bound of the float64 value
        for coef, S in ((GUL, gul), (MIX, full)):
            vals = k_sample_values(L, S, coef)
            for b in range(B):
                assert torch.equal(vals[b].cpu(), R.value_f32(S[b].cpu(), coef)), (coef, b)
                want, bound = float(R.value(ref[b].cpu(), coef)), R.value_bound(ref[b], lim[b], coef)
                err = abs(float(vals[b]) - want)
                print(f"  value coef={coef} sample {b}: {float(vals[b]):.9e} ref {want:.9e} |diff| {err:.3e} bound {bound:.3e}")
                assert err <= bound, (coef, b, float(vals[b]), want, err, bound)
            # the public entry point is these two launches
            shaped = [v.reshape(B, 1, 1, 1, n) for v in (src, t, w, s)]
            got = A.per_sample_loss(shaped[0], shaped[1], shaped[2], shaped[3] if coef[2] else None, *coef, apply_sigmoid=logits)
            assert got.shape == (B,) and got.dtype == torch.float32 and not got.requires_grad and torch.equal(got, vals)
    # the default arguments are the reference's mining key: general_union_loss_lib of probabilities, sample by sample
    got = A.per_sample_loss(p32, t, w)
    assert torch.equal(got, k_sample_values(L, k_sample_sums(L, p32, t, w, None, False, terms=2), GUL))
    assert torch.equal(A.per_sample_loss(p32, t), k_sample_values(L, k_sample_sums(L, p32, t, None, None, False, terms=2), GUL))


@pytest.mark.parametrize("n", (32 ** 3, 4096, 4099, 4 * SAMPLE_STRIDE + 4, SAMPLE_STRIDE + 3))
def test_a_sample_does_not_depend_on_its_batch(L, n):
    x, t, w, s = real_inputs(4, n, seed=91)
    for logits, src in ((True, x), (False, torch.sigmoid(x))):
        for terms in (2, 7):
            batch = k_sample_sums(L, src, t, w, s, logits, terms=terms)
            for b in range(4):
                alone = k_sample_sums(L, *[v[b:b + 1].clone() for v in (src, t, w, s)], logits, terms=terms)
                assert torch.equal(alone[0], batch[b]), (logits, terms, b, (alone[0] - batch[b]).tolist())
            pair = k_sample_sums(L, *[v[1:3].contiguous() for v in (src, t, w, s)], logits, terms=terms)
            assert torch.equal(pair, batch[1:3])
    if n % 4 == 0:            # a sample that starts 4 bytes past a 16-byte boundary runs the scalar path: the same elements
        base = [torch.zeros(4 * n + 1, device="cuda") for _ in range(4)]
        args = []
        for buf, v in zip(base, (x, t, w, s)):
            buf[1:] = v.reshape(-1)
            args.append(buf[1:].reshape(4, n))
        assert args[0].data_ptr() % 16 == 4
        got = k_sample_sums(L, *args, True)
        ref = torch.stack([R.sums(R.sigmoid(x[b].double()), t[b].double(), w[b].double(), s[b].double()) for b in range(4)])
        assert_within(got, ref, torch.stack([sample_sum_bound(ref[b], n, False, True) for b in range(4)]), "misaligned batch")


def dyadic_inputs(B, n, seed):
    """int64 (P, t, w, s) on the CPU with p = P / 256; the first and last element of every sample, and both sides of every
    stride trip, planted at p = 255/256, t = s = 1, w = 2."""
    g = torch.Generator().manual_seed(seed)
    P = (torch.randint(0, 257, (B, n), generator=g) + 37 * torch.arange(B)[:, None]) % 257
    t = (torch.randint(0, 8, (B, n), generator=g) == 0).long()
    s = t * torch.randint(0, 2, (B, n), generator=g)
    w = 1 + torch.randint(0, 2, (B, n), generator=g)
    pos = {0, n - 1, n - 4}
    for stride in (SAMPLE_STRIDE, 4 * SAMPLE_STRIDE):
        pos.update(q for q in (stride - 1, stride, stride + 1, stride + 3) if q < n)
    pos = torch.tensor(sorted(pos))
    for v, plant in ((P, 255), (t, 1), (s, 1), (w, 2)):
        v[:, pos] = plant
    return P, t, w, s


def int_sums(P, t, w, s):
    """(B, 7) float64: the sums in units of 2^-8 by int64 arithmetic (entries 3 and 4 unused)."""
    z = torch.zeros(P.shape[0], dtype=torch.int64)
    S = torch.stack([(P * t).sum(1), P.sum(1), 256 * t.sum(1), z, z, (w * P * s * s).sum(1), (w * (P * s + 256 * s)).sum(1)], 1)
    return S.double() / 256.0


@pytest.mark.parametrize("B,n", CASES)
def test_exact_sums(L, B, n):
    Pi, ti, wi, si = dyadic_inputs(B, n, seed=13)
    want = int_sums(Pi, ti, wi, si)
    p, t, w, s = [v.float().cuda() for v in (Pi / 256.0, ti, wi, si)]
    assert bool((p * 256 == p.mul(256).round()).all())
    full = k_sample_sums(L, p, t, w, s, 0, terms=7)
    assert torch.equal(full[:, EXACT].cpu(), want[:, EXACT]), (full.cpu() - want).tolist()
    dice = k_sample_sums(L, p, t, w, s, 0, terms=1)
    assert torch.equal(dice[:, [0, 1, 2]].cpu(), want[:, [0, 1, 2]]) and bool((dice[:, 3:] == 0).all())
    ref = torch.stack([R.sums(p[b].double(), t[b].double(), w[b].double(), s[b].double()) for b in range(B)])
    lim = torch.stack([sample_sum_bound(ref[b], n, is_vec(n, p, t, w, s), False) for b in range(B)])
    assert_within(full[:, ROUNDED], ref[:, ROUNDED], lim[:, ROUNDED], "sums 3, 4")
    # the whole-batch kernel sees the same elements: its exact sums are the samples' added up
    from seunet_amd import losses
    whole = losses._sums(p.reshape(-1), 0, t.reshape(-1), w.reshape(-1), s.reshape(-1), None, 7)
    if B * n <= 2 ** 23:
        assert torch.equal(whole[EXACT], full[:, EXACT].sum(0))


def test_rejects_bad_arguments(L):
    from seunet_amd import _lib
    import seunet_amd as A
    assert L.seunet_loss_sample_partial_floats(0) == 0 and "batch" in _lib.last_error()
    x = torch.zeros(8, device="cuda")
    out = torch.zeros(7, dtype=torch.float64, device="cuda")
    part = torch.zeros(256 * 7, device="cuda")
    assert L.seunet_loss_sums_per_sample(x.data_ptr(), 0, x.data_ptr(), None, None, 0, 8, part.data_ptr(), out.data_ptr(), 0, None) != 0
    assert L.seunet_loss_sums_per_sample(x.data_ptr(), 0, x.data_ptr(), None, None, 1, 8, part.data_ptr(), out.data_ptr(), 8, None) != 0
    with pytest.raises(RuntimeError):
        A.per_sample_loss(torch.zeros(2, 8), torch.zeros(2, 8))
