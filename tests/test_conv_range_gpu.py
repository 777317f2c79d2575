"""Every convolution kernel, forward, data gradient and weight gradient, at the two ends of its storage type's number range and
on non-finite operands, BITWISE against the exact scaled-integer reference (method and helpers: tests/range_cases.py).

  subnormal operands   the 16-bit operand that stands for a gradient is integers times the type's smallest subnormal
                       (2^-24 in fp16, 2^-133 in bf16); a kernel that flushes an operand, a product, a partial sum or a result
                       stores zeros.  In fp16 a second run shifts the operand (still subnormal) so that the results lie on both
                       sides of 2^-14.
  top of the range     fp16: results of 65520 and above must be stored as +-inf, everything below as the rounded finite value;
                       the weight gradient with BOTH operands at 2^15 (a product formed in 16 bits would be inf).
  non-finite operands  one +inf in sample 0 and one NaN in sample 1 must arrive as +-inf / NaN exactly over their tap
                       footprints, a third sample stays what it is without them.  (The x-folded forms of the streaming
                       kernel may also write NaN one column further: ``range_cases.structural_zero_reach``.)

The range does not depend on the extent, so every kernel is forced at the small shapes of tests/test_ops_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_layer_cases as L  # noqa: E402
import range_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu

# every (kernel, pass) pair the benchmark's plan routes has a case here: a kernel that is routed later fails this line until
# it gets one
assert R.COVERED == L.Config(4, 128, 1).ROUTED, (sorted(R.COVERED), sorted(L.Config(4, 128, 1).ROUTED))


@pytest.fixture(scope="module")
def S():
    return L.ops_or_skip()


def subnormal_scales(ref, dtype):
    """The type's quantum, and in fp16 the shift at which the results straddle 2^-14 (asserted on the reference)."""
    scales = [R.Q_EXP[dtype]]
    if dtype == "fp16":
        k = R.straddle_shift(ref)
        sub, nrm = R.shares_below_normal(ref, R.Q_EXP[dtype] + k, dtype)
        assert k <= 8 and sub >= 0.10 and nrm >= 0.10, (k, sub, nrm)
        if k:
            scales.append(R.Q_EXP[dtype] + k)
    return scales


# ---- subnormal operands ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FWD_CASES, ids=L.ids)
def test_forward_subnormal_operands(S, case):
    name, dtype = case
    c, dt = R.data("fwd", name)
    for s in subnormal_scales(dt["ref"], dtype):
        x = R.scaled(dt["x"], s)
        assert float(x.abs().max()) < 2.0 ** R.MIN_NORMAL_EXP[dtype]
        got, _, _ = R.run_forward(S, c, x, dt["wt"], None if dt["b"] is None else R.scaled(dt["b"], s), dtype)
        R.same_bits(got, R.expect_forward(dt, s, dtype), f"{name} forward on {c['fwd']} ({dtype}), x and bias = integers x 2^{s}")


@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=L.ids)
def test_data_gradient_subnormal_operands(S, case):
    name, dtype = case
    c, dt = R.data("dgrad", name)
    for s in subnormal_scales(dt["ref"], dtype):
        dy = R.scaled(dt["dy"], s)
        assert float(dy.abs().max()) < 2.0 ** R.MIN_NORMAL_EXP[dtype]
        for acc in (False, True):
            got = R.run_dgrad(S, c, dy, dt["wt"], R.scaled(dt["prev"], s), dtype, acc)
            R.same_bits(got, R.expect_dgrad(c, dt, s, dtype, acc),
                        f"{name} data gradient on {c['dgrad']} ({dtype}), dy = integers x 2^{s}, {'+=' if acc else 'overwrite'}")


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=L.ids)
def test_weight_gradient_subnormal_operands(S, case):
    """dy = {-1, 0, 1} x q, x integer: the f32 weight gradient is the integer one times q, bitwise (in bf16 an f32 subnormal)."""
    name, dtype = case
    c, dt = R.data("wgrad", name)
    s = R.Q_EXP[dtype]
    got = R.run_wgrad(S, c, dt["x"].float(), R.scaled(dt["dy"], s), dtype)
    R.same_bits(got, R.scaled(dt["ref"], s), f"{name} weight gradient on {c['wgrad']} ({dtype}), dy = integers x 2^{s}")


# ---- top of the range (fp16) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in R.WGRAD])
def test_weight_gradient_top_of_range(S, name):
    """x and dy are {-1, 0, 1} x 2^15: every product is +-2^30, the f32 result integers x 2^30."""
    c, dt = R.data("wgrad", name)
    got = R.run_wgrad(S, c, R.scaled(dt["x"], 15), R.scaled(dt["dy"], 15), "fp16")
    R.same_bits(got, R.scaled(dt["ref"], 30), f"{name} weight gradient on {c['wgrad']} (fp16), x and dy = integers x 2^15")


@pytest.mark.parametrize("name", [c["name"] for c in R.FWD_DGRAD])
def test_forward_top_of_range(S, name):
    c, dt = R.data("fwd", name)
    e = R.top_exponent(dt["ref"])
    share = R.overflow_share(dt["ref"], e)
    print(f"  {name} forward: e = {e}, {share:.4f} of the outputs reach 65520")
    assert 0.01 <= share <= 0.5, (e, share)
    want = R.expect_forward(dt, e, "fp16")
    assert float(want.float().isinf().double().mean()) == share and not bool(want.isnan().any())
    got, _, _ = R.run_forward(S, c, R.scaled(dt["x"], e), dt["wt"], None if dt["b"] is None else R.scaled(dt["b"], e), "fp16")
    R.same_bits(got, want, f"{name} forward on {c['fwd']} (fp16), x and bias = integers x 2^{e}")


@pytest.mark.parametrize("name", [c["name"] for c in R.FWD_DGRAD if c["dgrad"]])
def test_data_gradient_top_of_range(S, name):
    c, dt = R.data("dgrad", name)
    e = R.top_exponent(dt["ref"], dt["prev"])
    prev = R.scaled(dt["prev"], e)
    for acc in (False, True):
        share = R.overflow_share(dt["ref"], e, prev if acc else None)
        print(f"  {name} data gradient {'+=' if acc else 'overwrite'}: e = {e}, {share:.4f} of the outputs reach 65520")
        assert e <= 14 and 0.01 <= share <= 0.5, (e, share)
        want = R.expect_dgrad(c, dt, e, "fp16", acc)
        assert bool(want.isinf().any()) and not bool(want.isnan().any()) and bool(R.stored(prev, "fp16").isfinite().all())
        got = R.run_dgrad(S, c, R.scaled(dt["dy"], e), dt["wt"], prev, "fp16", acc)
        R.same_bits(got, want, f"{name} data gradient on {c['dgrad']} (fp16), dy = integers x 2^{e}, {'+=' if acc else 'overwrite'}")


# ---- non-finite operands --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FWD_CASES, ids=L.ids)
def test_forward_nonfinite_operands(S, case):
    name, dtype = case
    c, dt = R.data("fwd", name, nonfinite=True)
    want = R.expect_nonfinite(c, dt, "fwd", dtype)
    pos, neg, nan = R.footprint(c, "fwd", dt)
    assert bool(pos[0].any()) and bool(neg[0].any()) and bool(nan[1].any()) and not bool((pos | neg | nan)[2].any())
    got, part, slots = R.run_forward(S, c, R.planted(dt["x"], c, "fwd"), dt["wt"], dt["b"], dtype)
    R.same_bits(got, want, f"{name} forward on {c['fwd']} ({dtype}), +inf in sample 0 and NaN in sample 1 of x",
                nan_allowed=R.structural_zero_reach(c, "fwd"))
    clean, part0, _ = R.run_forward(S, c, dt["x"].float(), dt["wt"], dt["b"], dtype)
    R.same_bits(clean, R.stored(dt["ref"], dtype), f"{name} forward on {c['fwd']} ({dtype}), the same operands without the plants")
    # statistic partials [n, slots, C, 2]: every (sample, channel) a plant reaches is non-finite once its slots are summed
    # (each output channel sees each plant through non-zero weights), the third sample's records are the unplanted run's bits
    tot = part[:, :, :c["cout"]].sum(1).cpu()
    assert not bool(tot[:2].isfinite().any()), f"{name} {dtype}: finite statistic sums of a planted sample:\n{tot[:2]}"
    assert torch.equal(part[2].cpu().view(torch.int64), part0[2].cpu().view(torch.int64)), f"{name} {dtype}: statistics of the unplanted sample changed"


@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=L.ids)
def test_data_gradient_nonfinite_operands(S, case):
    name, dtype = case
    c, dt = R.data("dgrad", name, nonfinite=True)
    pos, neg, nan = R.footprint(c, "dgrad", dt)
    assert bool(pos[0].any()) and bool(neg[0].any()) and bool(nan[1].any()) and not bool((pos | neg | nan)[2].any())
    for acc in (False, True):
        want = R.expect_nonfinite(c, dt, "dgrad", dtype, acc)
        got = R.run_dgrad(S, c, R.planted(dt["dy"], c, "dgrad"), dt["wt"], dt["prev"].float(), dtype, acc)
        R.same_bits(got, want, f"{name} data gradient on {c['dgrad']} ({dtype}), +inf in sample 0 and NaN in sample 1 of dy, "
                               f"{'+=' if acc else 'overwrite'}", nan_allowed=R.structural_zero_reach(c, "dgrad"))


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=L.ids)
def test_weight_gradient_nonfinite_operands(S, case):
    """Every entry whose sum contains a planted dy voxel is non-finite; the output channels without a plant are the exact
    integers.  (Entries of a planted channel whose tap reads the padding at the plant are not constrained.)"""
    name, dtype = case
    c, dt = R.data("wgrad", name)
    touched = R.wgrad_touched(c, dt)
    assert bool(touched.any())
    got = R.run_wgrad(S, c, dt["x"].float(), R.planted(dt["dy"], c, "wgrad"), dtype)
    hidden = touched & got.isfinite()
    assert not bool(hidden.any()), (f"{name} weight gradient on {c['wgrad']} ({dtype}): {int(hidden.sum())} of {int(touched.sum())} entries whose sum "
                                    f"holds an inf / NaN are finite, first (co, ci, kz, ky, kx) {hidden.nonzero()[:4].tolist()}")
    keep = [co for co in range(c["cout"]) if co not in R.wgrad_plant_channels(c)]
    R.same_bits(got[keep], dt["ref"][keep], f"{name} weight gradient on {c['wgrad']} ({dtype}): output channels without a plant")
