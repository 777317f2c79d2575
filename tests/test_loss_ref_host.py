"""tests/loss_ref.py (the float64 restatement the GPU loss tests compare csrc/loss.hip with) against float64 autograd of
oracle/seunet_oracle.py's dice_loss / general_union_loss_lib / atr_loss / stage_loss: two float64 evaluations of the same
graph, so they agree to 1e-10 of the largest element.  Needs no GPU."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as R  # noqa: E402
import seunet_oracle as orc  # noqa: E402

SHAPE = (2, 1, 6, 7, 9)
MIX = (0.3, 1.0, 0.5)


def close(got, want, what):
    err = float((got - want).abs().max())
    lim = 1e-10 * max(float(want.abs().max()), 1e-300)
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def inputs(label, shape=SHAPE, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, dtype=torch.float64, generator=g) * 3
    if label == "soft":
        t = torch.rand(shape, dtype=torch.float64, generator=g)
    else:
        t = (torch.rand(shape, dtype=torch.float64, generator=g) > 0.7).double()
    w = 1 + torch.rand(shape, dtype=torch.float64, generator=g)
    s = t * (torch.rand(shape, dtype=torch.float64, generator=g) > 0.5).double()
    return x, t, w, s


LOSSES = {"dice_loss": ((1.0, 0.0, 0.0), lambda p, t, w, s: orc.dice_loss(p, t)),
          "general_union_loss_lib": ((0.0, 1.0, 0.0), lambda p, t, w, s: orc.general_union_loss_lib(p, t, w)),
          "atr_loss": ((0.0, 0.0, 1.0), lambda p, t, w, s: orc.atr_loss(p, t, s, w)),
          "mix": (MIX, lambda p, t, w, s: MIX[0] * orc.dice_loss(p, t) + MIX[1] * orc.general_union_loss_lib(p, t, w)
                  + MIX[2] * orc.atr_loss(p, t, s, w))}


@pytest.mark.parametrize("label", ("binary", "soft"))
@pytest.mark.parametrize("name", list(LOSSES))
def test_probability_losses_match_oracle_autograd(name, label):
    coef, fn = LOSSES[name]
    x, t, w, s = inputs(label)
    p = torch.sigmoid(x).requires_grad_()
    loss = fn(p, t, w, s)
    (2.5 * loss).backward()
    with torch.no_grad():
        S = R.sums(p, t, w, s)
        close(R.value(S, coef), loss, name)
        g, mag, prop = R.grad_pred(p, t, w, s, S, coef, scale=2.5)
        close(g, p.grad, name + " gradient")
        assert bool((mag >= g.abs() * (1 - 1e-12)).all()) and float(prop.abs().max()) == 0.0


@pytest.mark.parametrize("label", ("binary", "soft"))
@pytest.mark.parametrize("name", list(LOSSES))
def test_logit_losses_match_oracle_autograd(name, label):
    coef, fn = LOSSES[name]
    x, t, w, s = inputs(label, seed=1)
    x.requires_grad_()
    loss = fn(torch.sigmoid(x), t, w, s)
    loss.backward()
    with torch.no_grad():
        S = R.sums(R.sigmoid(x), t, w, s)
        g, mag, _, p, ds = R.grad_logit(x, t, w, s, S, coef)
        close(R.value(S, coef), loss, name)
        close(g, x.grad, name + " gradient")
        close(ds, p * (1 - p), "p (1 - p)")


@pytest.mark.parametrize("label", ("binary", "soft"))
@pytest.mark.parametrize("stage", (1, 2, 3))
def test_stage_losses_match_oracle_autograd(stage, label):
    """Both heads, the coefficients ``fused_stage_loss`` gives them; the decoder head is head 0."""
    xe, t, w, s = inputs(label, seed=2)
    xd = (xe * 0.5 + 0.1).clone()
    xe.requires_grad_(), xd.requires_grad_()
    loss = orc.stage_loss(stage, xe, xd, t, w, s)
    loss.backward()
    cd, ce = {1: ((1.0, 0.0, 0.0), (1.0, 0.0, 0.0)), 2: ((0.0, 1.0, 0.0), (0.0, 0.5, 0.0)), 3: ((0.0, 1.0, 0.5), (0.0, 0.5, 0.5))}[stage]
    with torch.no_grad():
        Sd, Se = R.sums(R.sigmoid(xd), t, w, s), R.sums(R.sigmoid(xe), t, w, s)
        close(R.value(Sd, cd) + R.value(Se, ce), loss, f"stage {stage}")
        close(R.grad_logit(xd, t, w, s, Sd, cd)[0], xd.grad, "decoder head")
        close(R.grad_logit(xe, t, w, s, Se, ce)[0], xe.grad, "encoder head")


def test_broadcast_label_and_missing_maps():
    """A (N, 1, ...) label against a three-class prediction; weight None is 1 and skeleton None is 0."""
    x, _, w, _ = inputs("binary", shape=(2, 3, 4, 5, 6), seed=3)
    _, t, _, s = inputs("soft", shape=(2, 1, 4, 5, 6), seed=4)
    p = torch.sigmoid(x).requires_grad_()
    one, zero = torch.ones_like(p), torch.zeros_like(p)
    loss = LOSSES["mix"][1](p, t.expand_as(p), one, zero)
    loss.backward()
    with torch.no_grad():
        S = R.sums(p, t, None, None)
        close(R.value(S, MIX), loss, "mix")
        close(R.grad_pred(p, t, None, None, S, MIX)[0], p.grad, "mix gradient")
        assert float(S[5]) == 0.0 and float(S[6]) == 0.0


def test_saturated_logits_and_propagation():
    x = torch.tensor([-100.0, -40.0, -1.0, 0.0, 2.0, 40.0, 100.0], dtype=torch.float64)
    ds = R.dsigmoid(x)
    assert bool((ds > 0).all()) and abs(float(ds[6]) / math.exp(-100.0) - 1) < 1e-12 and float(ds[3]) == 0.25
    # prop is the first-order change of the gradient under a change of the sums (checked against an actual change)
    xx, t, w, s = inputs("soft", seed=5)
    p = torch.sigmoid(xx)
    S = R.sums(p, t, w, s)
    e = S * 1e-6
    g0, _, prop = R.grad_pred(p, t, w, s, S, MIX, sum_err=e)
    for sign in (torch.tensor([1, -1, 1, -1, 1, -1, 1.0]), torch.tensor([-1, 1, 1, 1, -1, -1, 1.0])):
        g1 = R.grad_pred(p, t, w, s, S + sign.double() * e, MIX)[0]
        assert bool(((g1 - g0).abs() <= prop).all())


def test_bounds_arithmetic():
    n = 4 * 128 ** 3
    assert R.sum_adds(n, True) == 32 and R.sum_adds(n, False) == 32 and R.sum_depth(n, True) == 41
    assert R.sum_adds(4 * R.STRIDE, True) == 4 and R.sum_adds(4 * R.STRIDE + 4, True) == 8 and R.sum_adds(4 * R.STRIDE - 4, True) == 4
    assert R.sum_adds(31 * 33 * 35, False) == 1 and R.sum_adds(R.GRAD_THREADS + 1, False) == 5
    assert R.k_grad((1.0, 0.0, 0.0)) == 10 and R.k_grad((0.0, 0.0, 0.5)) == 12 and R.k_grad((0.3, 1.0, 0.5)) == 19 + 2 * R.POWF_ULP
    assert R.K_P == 5.5
    # ratio_err is exact-arithmetic: the worst corner of the box attains it
    A, eA, B, eB = 1000.0, 0.5, 3000.0, 2.0
    worst = max(abs((A + da + 1) / (B + db + 1) - (A + 1) / (B + 1)) for da in (-eA, eA) for db in (-eB, eB))
    assert worst <= R.ratio_err(A, eA, B, eB) <= worst * 1.01
    r = torch.tensor([1.0, 1.5, 0.0, -260.0], dtype=torch.float64)
    assert R.storage_ulp(r, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -133, 2.0]
    assert float(R.storage_ulp(r, torch.float32).abs().max()) == 0.0


@pytest.mark.parametrize("logits", (False, True))
def test_a_float32_evaluation_is_inside_the_bounds(logits):
    """The bounds are worst cases of a correct float32 evaluation: torch's float32 evaluation of the same formulas on the CPU
    (its own libm, the same operation counts) has to be inside them, sums and gradient, with planted +-100 logits."""
    g = torch.Generator().manual_seed(7)
    n = 20000
    x = torch.randn(n, generator=g) * 3
    x[::997] = 100.0
    x[5::991] = -100.0
    t = (torch.rand(n, generator=g) > 0.9).float()
    w = 1 + torch.rand(n, generator=g)
    s = t * (torch.rand(n, generator=g) > 0.5).float()
    p32 = torch.sigmoid(x) if logits else torch.rand(n, generator=g)
    src = x if logits else p32
    S = R.sums(R.sigmoid(x.double()) if logits else p32.double(), t.double(), w.double(), s.double())
    got = torch.stack([v.sum() for v in (p32 * t, p32, t, w * (p32 + 1e-4) ** 0.7 * t, w * (0.2 * p32 + 0.8 * t), w * p32 * s * s,
                                         w * (p32 * s + s))]).double()
    assert bool(((got - S).abs() <= R.sum_bound(S, n, False, logits)).all())
    Sf = [float(v) for v in S]
    A, B = Sf[3] + 1, Sf[4] + 1
    a = torch.where(t != 0, 0.7 * w * t * (p32 + 1e-4) ** -0.3, torch.zeros(n)) * B
    g32 = -(a - A * 0.2 * w) / (B * B)
    if logits:
        g32 = g32 * (p32 * (1 - p32))
        ref, mag, _, p, ds = R.grad_logit(src.double(), t.double(), w.double(), s.double(), S, (0.0, 1.0, 0.0))
        lim = R.grad_bound_logit(mag, p, ds, (0.0, 1.0, 0.0))
        assert bool((g32[x.abs() == 100] == 0).all())
    else:
        ref, mag, _ = R.grad_pred(src.double(), t.double(), w.double(), s.double(), S, (0.0, 1.0, 0.0))
        lim = R.grad_bound_pred(mag, (0.0, 1.0, 0.0))
    assert bool(((g32.double() - ref).abs() <= lim).all()), float(((g32.double() - ref).abs() / lim).max())

