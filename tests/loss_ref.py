"""Plain float64 restatement of the Dice / General-Union / ATR losses of csrc/loss.hip, and the derived error bounds the GPU
tests assert.

Everything here is ordinary torch arithmetic in float64 on whatever device its inputs live on; nothing calls the native library.
tests/test_loss_ref_host.py runs it on the CPU and pins it against float64 autograd of oracle/seunet_oracle.py;
tests/test_loss_layers_gpu.py runs it on the GPU in float64: the elementwise part is elementwise torch, the seven sums are
``torch.sum`` of float64 tensors of non-negative terms (torch's own reduction, off by < 64 x 2^-53 of the sum, a term the sum
bound carries), and the exact-sum test does not use it at all (its reference is int64 arithmetic on the CPU).

The seven whole-batch sums, as the header of csrc/loss.hip defines them (t = label, w = weight or 1, s = skeleton or 0):
  0  sum p t     1  sum p     2  sum t                                   (Dice)
  3  sum w (p + 1e-4)^0.7 t    4  sum w (0.2 p + 0.8 t)                  (general union)
  5  sum w (p s) s             6  sum w (p s + s)                        (ATR)
Each loss is c (1 - (A + 1) / (B + 1)) with (A, B) = (2 S0, S1 + S2), (S3, S4), (S5, S6), so with a = dA/dp / (B + 1) and
b = (A + 1) dB/dp / (B + 1)^2 its derivative is -c (a - b); ``mag`` = sum over the active losses of |c| (|a| + |b|) is the
magnitude the element bounds are relative to.

Rounding model: u = 2^-24; one f32 operation is off by at most u relative; a math function that is off by E ulp is off by at
most 2 E u relative.  The constants 1e-4f, 0.2f, 0.8f, 0.7f, -0.3f of the kernel are float32 roundings of the numbers used
here (relative u each): an exponent off by u relative moves b^e by |e ln b| u, and b = p + 1e-4 >= 1e-4 gives |ln b| <= 9.22.

Math-function constants.  The ROCm installation documents no ulp figures for its device ``expf`` / ``powf``, so they were
measured on an MI355X at the parent commit with a stand-alone HIP program (same compiler flags as csrc/Makefile) against the
device's float64 ``exp`` / ``pow``, exhaustively over every float32 argument the kernels can pass:
  expf(a),  2^-30 <= |a| <= 87 (both signs)            worst 0.8615 ulp
  powf(b, 0.7f),  powf(b, -0.3f),  1e-4f <= b <= 1.0002  worst 1.3297 / 1.3194 ulp
  (1 / (1 + expf(-x)) as a whole, |x| <= 87: worst 2.74 u relative, inside K_P = 5.5 below)
EXPF_ULP and POWF_ULP are those figures with a margin of 2x.

Counts (loss.hip line by line):
  * p from a logit, p = 1 / (1 + expf(-x)): the negation is exact, expf 2 EXPF_ULP u (times e / (1 + e) <= 1), the addition 1,
    the division 1:  K_P = 2 EXPF_ULP + 2, RELATIVE to p -- except that expf overflows for x < -88.7 and p becomes 0 where it
    is < 2^-126: an absolute 2^-126 (TINY) per element accompanies every bound of the logit entry.
  * terms of the sums (K_SUM, probability entry; the logit entry adds K_P to every term that contains p):
      0: one product                                                                                       1
      1, 2: none                                                                                           0
      3: 1e-4f (0.7 u: 1), the addition (0.7 u: 1), the exponent constant (0.7 x 9.22 u: 7), powf, two products
                                                                                          11 + 2 POWF_ULP
      4: per term a constant and a product (2), the addition, the product with w                           4
      5: three products                                                                                    3
      6: a product, the addition, a product                                                                3
  * depth of the additions one term passes through (L): the thread's own additions at that n (4 per trip of the 16-byte path,
    1 per trip of the scalar path), 6 butterfly steps, 3 additions over the block's four waves.  The final pass is float64.
  * gradient, probability entry, per loss (the f64 -> f32 casts of A + 1 and B + 1 count as roundings of their own):
      Dice   a-term: cast of B 1, 2 t B 1, subtraction 1, denominator B B (2 casts + product) 3, division 1, times c 1,
             accumulation 1, times the scale 1 = 10 (b-term 9)                                             10
      GUL    a-term: 0.7f 1, 1e-4f (0.3 u: 1), addition (1), exponent constant (0.3 x 9.22 u: 3), powf 2 POWF_ULP, three
             products 3, times B (cast + product) 2, subtraction 1, denominator 3, division 1, c / accumulation / scale 3
                                                                                          19 + 2 POWF_ULP
      ATR    a-term: w s s 2, times B 2, subtraction 1, denominator 3, division 1, c / accumulation / scale 3
                                                                                                           12
    A mix is bounded by the largest count of its active losses times the whole ``mag``.
  * gradient, logit entry: got = g_p(p^) p^ (1 - p^) with p^ = p (1 + d), |d| <= K_P u.  g_p depends on p through the GUL power
    only: 0.3 K_P u more on its a-term.  1 - p^ and the two products are 3 roundings.  p^ (1 - p^) - p (1 - p) =
    (p^ - p)(1 - p - p^), at most K_P u p in magnitude: ABSOLUTE in p(1-p), which is what is left near saturation.  So
      |got - ref| <= u mag ((K + 3 + 0.3 K_P) p (1 - p) + K_P p) + (1 + mag) TINY.
"""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
EXPF_ULP = 1.75                    # 2 x 0.8615 measured (see above)
POWF_ULP = 2.7                     # 2 x 1.3297 measured
K_P = 2 * EXPF_ULP + 2
SIGMA, ALPHA, GAMMA = 1e-4, 0.2, 0.7
NSUMS = 7
STRIDE = 1024 * 256                # threads of the reduction grid
GRAD_THREADS = 4096 * 256          # threads of the clamped gradient grid
K_SUM = (1.0, 0.0, 0.0, 11 + 2 * POWF_ULP, 4.0, 3.0, 3.0)
SUM_HAS_P = (True, True, False, True, True, True, True)
K_GRAD = (10.0, 19 + 2 * POWF_ULP, 12.0)
F64_SUM = 64 * 2.0 ** -53          # torch's float64 reduction and the kernel's float64 final pass, relative to the sum


# ---- the losses -------------------------------------------------------------------------------------------------------------
def sigmoid(x):
    return torch.sigmoid(x)


def dsigmoid(x):
    """p (1 - p) without the cancellation of 1 - p: e / (1 + e)^2 with e = exp(-|x|)."""
    e = torch.exp(-x.abs())
    return e / ((1 + e) * (1 + e))


def _full(v, like, fill):
    return torch.full_like(like, fill) if v is None else torch.broadcast_to(v.to(like.dtype), like.shape)


def terms(p, t, w=None, s=None):
    """The seven per-element terms (float64 tensors of p's shape); t / w / s broadcast against p."""
    t, w, s = _full(t, p, 0.0), _full(w, p, 1.0), _full(s, p, 0.0)
    ps = p * s
    return (p * t, p, t, w * (p + SIGMA) ** GAMMA * t, w * (ALPHA * p + (1 - ALPHA) * t), w * ps * s, w * (ps + s))


def sums(p, t, w=None, s=None):
    """[7] float64."""
    return torch.stack([x.sum() for x in terms(p, t, w, s)])


def value(S, coef):
    """Loss of one head from its seven sums, the operations of ``losses._value`` in its order (float64, not yet rounded)."""
    c_dice, c_gul, c_atr = coef
    out = S.new_zeros(())
    if c_dice:
        out = out + c_dice * (1 - (2 * S[0] + 1) / (S[1] + S[2] + 1))
    if c_gul:
        out = out + c_gul * (1 - (S[3] + 1) / (S[4] + 1))
    if c_atr:
        out = out + c_atr * (1 - (S[5] + 1) / (S[6] + 1))
    return out


def value_f32(S, coef, S1=None, coef1=None):
    """What the library returns: every head rounded to f32, two heads added in f32."""
    v = value(S, coef).to(torch.float32)
    return v if S1 is None else v + value(S1, coef1).to(torch.float32)


def _ab(p, t, w, s, S, coef):
    """Per active loss: (c, a, b, which loss)."""
    S = [float(v) for v in S]
    out = []
    if coef[0]:
        A, B = 2 * S[0] + 1, S[1] + S[2] + 1
        out.append((coef[0], 2 * t / B, torch.full_like(p, A / (B * B)), 0))
    if coef[1]:
        A, B = S[3] + 1, S[4] + 1
        out.append((coef[1], GAMMA * w * t * (p + SIGMA) ** (GAMMA - 1) / B, A * ALPHA * w / (B * B), 1))
    if coef[2]:
        A, B = S[5] + 1, S[6] + 1
        out.append((coef[2], w * s * s / B, A * w * s / (B * B), 2))
    return out


def grad_pred(p, t, w, s, S, coef, scale=1.0, sum_err=None):
    """d(scale sum_k c_k loss_k)/dp in closed form from GIVEN sums S.  Returns (gradient, mag, prop): prop bounds how far the
    gradient moves when every sum S[k] moves by at most sum_err[k] (zero without sum_err): with rA = eA / (A + 1) and
    rB = eB / (B + 1), a = dA/dp / (B + 1) moves by a rB and b = (A + 1) dB/dp / (B + 1)^2 by b (rA + 2 rB), to first order;
    the factor 1.01 covers the second order for rB < 1e-3 (asserted)."""
    t, w, s = _full(t, p, 0.0), _full(w, p, 1.0), _full(s, p, 0.0)
    g, mag, prop = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    Sf = [float(v) for v in S]
    e = [0.0] * NSUMS if sum_err is None else [float(v) for v in sum_err]
    AB = ((2 * Sf[0] + 1, Sf[1] + Sf[2] + 1, 2 * e[0], e[1] + e[2]), (Sf[3] + 1, Sf[4] + 1, e[3], e[4]),
          (Sf[5] + 1, Sf[6] + 1, e[5], e[6]))
    for c, a, b, k in _ab(p, t, w, s, S, coef):
        A, B, eA, eB = AB[k]
        rA, rB = eA / A, eB / B
        assert rB < 1e-3 and rA < 1e-3, (rA, rB)
        g = g - c * (a - b)
        mag = mag + abs(c) * (a.abs() + b.abs())
        prop = prop + 1.01 * abs(c) * (a.abs() * rB + b.abs() * (rA + 2 * rB))
    return g * scale, mag * abs(scale), prop * abs(scale)


def grad_logit(x, t, w, s, S, coef, scale=1.0, sum_err=None):
    """The same with respect to the logit x (p = sigmoid(x)): (gradient, mag, prop, p, p (1 - p))."""
    p, ds = sigmoid(x), dsigmoid(x)
    g, mag, prop = grad_pred(p, t, w, s, S, coef, scale, sum_err)
    return g * ds, mag, prop * ds, p, ds


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def sum_adds(n, vec):
    """Additions one thread's accumulator takes at n elements: 4 per trip of the 16-byte path, 1 per trip of the scalar path."""
    return 4 * math.ceil((n // 4) / STRIDE) if vec else math.ceil(n / STRIDE)


def sum_depth(n, vec):
    return sum_adds(n, vec) + 6 + 3


def sum_bound(S, n, vec, logits):
    """[7] bound of |got - S| for the float64 sums S of non-negative terms: (L + K) u S, plus the two float64 summations, plus
    (logit entry) the absolute TINY per element of a p that underflowed."""
    L = sum_depth(n, vec)
    K = [k + (K_P if (logits and has_p) else 0.0) for k, has_p in zip(K_SUM, SUM_HAS_P)]
    rel = torch.tensor([(L + k) * U + F64_SUM for k in K], dtype=torch.float64, device=S.device)
    return rel * S.abs() + (n * TINY * 4 if logits else 0.0)          # (w <= 2 and p s + s <= 2: a term is at most 4 p-errors)


def ratio_err(A, eA, B, eB):
    """|(A' + 1)/(B' + 1) - (A + 1)/(B + 1)| for |A' - A| <= eA, |B' - B| <= eB < B + 1 (exact, not first order)."""
    return (eA + (A + 1) / (B + 1) * eB) / (B + 1 - eB)


def value_bound(S, eS, coef):
    """Bound of |f32 value from sums within eS of S  -  float64 value from S| for one head: the ratios' errors, one f32
    rounding of the head's value, and 1e-15 for the float64 arithmetic itself."""
    S, e = [float(v) for v in S], [float(v) for v in eS]
    d = abs(coef[0]) * ratio_err(2 * S[0], 2 * e[0], S[1] + S[2], e[1] + e[2]) if coef[0] else 0.0
    d += abs(coef[1]) * ratio_err(S[3], e[3], S[4], e[4]) if coef[1] else 0.0
    d += abs(coef[2]) * ratio_err(S[5], e[5], S[6], e[6]) if coef[2] else 0.0
    v = abs(float(value(torch.tensor(S, dtype=torch.float64), coef)))
    return d + U * (v + d) + 1e-15


def k_grad(coef):
    return max(k for k, c in zip(K_GRAD, coef) if c)


def grad_bound_pred(mag, coef):
    """|got - ref| of the probability entry: K u mag, and 8 x 2^-149 for results in the subnormal range."""
    return k_grad(coef) * U * mag + 8 * 2.0 ** -149


def grad_bound_logit(mag, p, ds, coef):
    """|got - ref| of the logit entry (derivation in the module docstring)."""
    K = k_grad(coef) + 3 + (0.3 * K_P if coef[1] else 0.0)
    return U * mag * (K * ds + K_P * p) + (1 + mag) * TINY


def storage_ulp(r, dtype):
    """Spacing of a 16-bit storage type at |r| (float64 in and out); 0 for float32, whose rounding the counts contain."""
    if dtype == torch.float32:
        return torch.zeros_like(r)
    mant, emin = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    _, e = torch.frexp(r.abs())
    e = torch.where(r == 0, torch.full_like(e, emin + 1), e).clamp(min=emin + 1)
    return torch.ldexp(torch.ones_like(r), e - mant)
