"""Host checks of the number-range tests' own helpers and references (no GPU): what tests/test_conv_range_gpu.py and
tests/test_epilogue_range_gpu.py assume about their references holds, and each reference tells a wrong kernel from a right one
-- a flushing one, a saturating one, one that hides a non-finite value."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_layer_cases as L  # noqa: E402
import epilogue_ref as ER  # noqa: E402
import range_cases as R  # noqa: E402
import range_epilogue_cases as RE  # noqa: E402

FD = [c["name"] for c in R.FWD_DGRAD]
DG = [c["name"] for c in R.FWD_DGRAD if c["dgrad"]]
WG = [c["name"] for c in R.WGRAD]


def flushed(t, dtype):
    """What a kernel that reads or writes subnormals of the storage type as zero would make of t."""
    f = t.float()
    return torch.where(f.abs() < 2.0 ** R.MIN_NORMAL_EXP[dtype], torch.zeros_like(f), f).to(t.dtype)


def test_every_routed_kernel_and_pass_has_a_case():
    assert R.COVERED == L.Config(4, 128, 1).ROUTED
    assert R.COVERED == {(k, p) for k in ("Stream", "March", "Tiled") for p in ("fwd", "dgrad", "wgrad")} | {("Wgrad1x1", "wgrad")}


def test_bit_patterns_tell_what_equality_does_not():
    a = torch.tensor([float("inf"), float("nan"), 1.0, 0.0], dtype=torch.float16)
    assert torch.equal(R.bits(a), R.bits(a.clone()))
    assert not torch.equal(R.bits(a), R.bits(torch.tensor([65504.0, float("nan"), 1.0, 0.0], dtype=torch.float16)))
    assert not torch.equal(R.bits(a), R.bits(torch.tensor([float("inf"), 0.0, 1.0, 0.0], dtype=torch.float16)))
    assert torch.equal(R.bits(a), R.bits(torch.tensor([float("inf"), -float("nan"), 1.0, -0.0], dtype=torch.float16)))
    with pytest.raises(pytest.fail.Exception, match="bit patterns differ on 1 of 4"):
        R.same_bits(torch.tensor([65504.0, float("nan"), 1.0, 0.0], dtype=torch.float16), a, "saturated")


@pytest.mark.parametrize("kind,name", [("fwd", n) for n in FD] + [("dgrad", n) for n in DG] + [("wgrad", n) for n in WG])
def test_scaled_integer_reference_is_exact_at_every_scale_used(kind, name):
    """ldexp of the integer result (and of every operand) is exact in f32: in f32's subnormal range for bf16's quantum, at
    2^30 for the weight gradient at the top of fp16's range."""
    c, dt = R.data(kind, name)
    ref = dt["ref"]
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref, ref.round())
    scales = [R.Q_EXP["fp16"], R.Q_EXP["bf16"]] + ([30] if kind == "wgrad" else [R.Q_EXP["fp16"] + R.straddle_shift(ref), R.top_exponent(ref, dt.get("prev"))])
    for s in scales:
        R.scaled(ref, s)                                    # (asserts exactness itself)
    for dtype in L.DTYPES:                                  # the 16-bit operand at the quantum is a number of the type
        op = R.scaled(dt["x" if kind == "fwd" else "dy"], R.Q_EXP[dtype])
        assert torch.equal(R.stored(op, dtype).float(), op) and float(op.abs().max()) < 2.0 ** R.MIN_NORMAL_EXP[dtype]
        if kind != "wgrad":                                 # every non-zero result at the quantum is stored non-zero
            want = R.stored(R.scaled(ref, R.Q_EXP[dtype]), dtype)
            assert torch.equal(want.float() != 0, ref != 0)
            # a flushing kernel is told apart
            assert not torch.equal(R.bits(flushed(want, dtype)), R.bits(want))
        else:
            want = R.scaled(ref, R.Q_EXP[dtype])
            assert torch.equal(want != 0, ref != 0) and bool((ref != 0).any())
    if kind == "wgrad":
        assert torch.equal(R.stored(R.scaled(dt["dy"], 15), "fp16").float(), R.scaled(dt["dy"], 15))
        # a product formed in 16 bits would be inf
        assert bool((R.stored(R.scaled(dt["dy"], 15), "fp16") * R.stored(R.scaled(dt["dy"], 15), "fp16")).isinf().any())


@pytest.mark.parametrize("kind,name", [("fwd", n) for n in FD] + [("dgrad", n) for n in DG])
def test_fp16_reference_straddles_the_smallest_normal_and_65520(kind, name):
    c, dt = R.data(kind, name)
    ref = dt["ref"]
    # at the quantum itself every result of these layers is subnormal (the largest integer result is below 1024) ...
    assert R.shares_below_normal(ref, R.Q_EXP["fp16"], "fp16")[0] == 1.0
    # ... and at the shifted scale, with the operand still subnormal, both ranges are present
    k = R.straddle_shift(ref)
    sub, nrm = R.shares_below_normal(ref, R.Q_EXP["fp16"] + k, "fp16")
    assert 1 <= k <= 8 and sub >= 0.10 and nrm >= 0.10, (k, sub, nrm)
    assert 3 * 2.0 ** (R.Q_EXP["fp16"] + k) < 2.0 ** -14
    want = R.stored(R.scaled(ref, R.Q_EXP["fp16"] + k), "fp16")
    mag = want.float().abs()
    assert bool((mag == 2.0 ** -14).any() or ((mag < 2.0 ** -14) & (mag > 0)).any() and (mag >= 2.0 ** -14).any())
    assert not torch.equal(R.bits(flushed(want, "fp16")), R.bits(want))
    # top of the range
    prev = dt.get("prev")
    e = R.top_exponent(ref, prev)
    assert e <= 14 and float(R.scaled(torch.tensor([3.0]), e)) <= 65504
    for extra in ([None] if prev is None else [None, R.scaled(prev, e)]):
        share = R.overflow_share(ref, e, extra)
        assert 0.01 <= share <= 0.5, (e, share)
        want = R.expect_forward(dt, e, "fp16") if kind == "fwd" else R.expect_dgrad(c, dt, e, "fp16", extra is not None)
        # (the tiled kernel's staged += rounds the new value first: inf before the addition, so a few more than `share`)
        staged = kind == "dgrad" and extra is not None and L.tiled_rounds_before_it_adds(c)
        got_share = float(want.isinf().double().mean())
        assert (got_share >= share if staged else got_share == share) and not bool(want.isnan().any()), (got_share, share)
        # a kernel that saturates at 65504 is told apart
        sat = want.float().clamp(-65504, 65504).to(torch.float16)
        assert not torch.equal(R.bits(sat), R.bits(want))


@pytest.mark.parametrize("kind,name", [("fwd", n) for n in FD] + [("dgrad", n) for n in DG])
def test_nonfinite_expectation_is_the_tap_footprint(kind, name):
    """F.conv3d on the planted operands (the expectation of the GPU test) is +-inf exactly where the +inf plant arrives through
    a positive / negative weight, NaN exactly where the NaN plant arrives, and the exact integers elsewhere -- derived a second
    way, from the plants' indicators convolved with the weights."""
    c, dt = R.data(kind, name, nonfinite=True)
    assert c["dims"][0] == 3 and not bool((dt["wt"] == 0).any())
    pos, neg, nan = R.footprint(c, kind, dt)
    assert bool(pos[0].any()) and bool(neg[0].any()) and bool(nan[1].any())
    assert not bool((pos | neg)[1:].any()) and not bool(nan[0].any()) and not bool(nan[2].any())
    k = 27 if c["taps"] == 27 else 1
    assert int(nan[1, 0].sum()) < k and int((pos | neg)[0, 0].sum()) < k or k == 1        # clipped at the faces
    for dtype in L.DTYPES:
        want = R.expect_nonfinite(c, dt, kind, dtype).float()
        assert torch.equal(want == float("inf"), pos) and torch.equal(want == -float("inf"), neg) and torch.equal(want.isnan(), nan)
        plain = R.stored(dt["ref"], dtype).float()
        fin = ~(pos | neg | nan)
        assert torch.equal(want[fin], plain[fin])
        # a kernel that hides the plants (zero-skip, NaN-dropping max) is told apart
        assert not torch.equal(R.bits(R.stored(plain, dtype)), R.bits(R.stored(want, dtype)))


@pytest.mark.parametrize("name", WG)
def test_weight_gradient_entries_a_plant_reaches(name):
    """The mask of the GPU test against torch's own weight gradient of the planted operands (x without zeros here, so that
    the CPU's result is non-finite exactly where a planted product enters)."""
    c, dt = R.data("wgrad", name)
    touched = R.wgrad_touched(c, dt)
    k = 3 if c["taps"] == 27 else 1
    x = dt["x"][:, :c["cin"]].float().clone()
    x[x == 0] = 1.0
    ref = torch.nn.grad.conv3d_weight(x, (c["cout"], c["cin"], k, k, k), R.planted(dt["dy"], c, "wgrad"),
                                      padding=c["dilation"] if k == 3 else 0, dilation=c["dilation"] if k == 3 else 1)
    # (torch pads the volume with real zeros, and 0 x inf is NaN: the entries whose tap reads the padding at a plant are
    # non-finite there too, which is why the GPU test leaves them unconstrained)
    assert not bool((touched & ref.isfinite()).any())
    assert bool(ref[[co for co in range(c["cout"]) if co not in R.wgrad_plant_channels(c)]].isfinite().all())
    assert set(touched.flatten(1).any(1).nonzero().flatten().tolist()) == set(R.wgrad_plant_channels(c))


def test_x_folded_streaming_forms_are_the_only_ones_with_a_structural_zero_column():
    """``structural_zero_reach`` names exactly the forms se-unet-airseg_amd/csrc/conv_stream.hip folds x-taps for (8 -> <= 16 channels at dilation 1,
    16 -> <= 16), and there one column per plant, over the footprint's y and z extent."""
    with_mask = {(kind, c["name"]) for kind in ("fwd", "dgrad") for c in R.FWD_DGRAD if c[kind] and R.structural_zero_reach(c, kind) is not None}
    assert with_mask == {("fwd", "stream-2of8-8"), ("fwd", "stream-8-16"), ("dgrad", "stream-8-16")}
    c, _ = R.data("fwd", "stream-8-16", nonfinite=True)
    m = R.structural_zero_reach(c, "fwd")
    pos, neg, nan = R.footprint(c, "fwd", R.data("fwd", "stream-8-16", nonfinite=True)[1])
    assert int(m[:, 0].sum()) == 4 + 9 and not bool((m & (pos | neg | nan)).any()) and not bool(m[2].any())
    assert bool(m[0, :, 0, 8, 3].all()) and bool(m[1, :, 3, 3, 37].all())


# ---- the E-set recipe of the epilogue tests, on the pure-torch float64 references ------------------------------------------------
def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_reach_set_of_maxpool_routing_is_the_first_maximum_of_the_window():
    d = h = w = 4
    C = 8
    t = torch.randint(0, 3, (d, h, w, C), generator=torch.Generator().manual_seed(3)).float()      # ties
    _, first, tied = ER.pool_first_max(t)
    assert bool(tied.any())
    k = torch.arange(8)[None, :, None]
    f = lambda g0: {"s:g_in": ER.unpool_windows(torch.where(first[:, None, :] == k, g0.reshape(-1, 1, C), torch.zeros((), dtype=g0.dtype)), d, h, w)}
    g = _rand(d // 2, h // 2, w // 2, C, seed=4)
    idx = (1, 0, 1, 5)
    Eset = RE.reach_set(f, g, idx)["s:g_in"]
    x = t.permute(3, 0, 1, 2)[None].clone().requires_grad_(True)
    one = torch.zeros(1, C, d // 2, h // 2, w // 2)
    one[0, idx[3], idx[0], idx[1], idx[2]] = 1.0
    F.max_pool3d(x, 2).backward(one)
    assert int(Eset.sum()) == 1 and torch.equal(Eset, x.grad[0].permute(1, 2, 3, 0) != 0)


def test_reach_set_of_the_instance_norm_backward_is_the_whole_channel_of_the_plant():
    V, C = 96, 8
    x = _rand(V, C, seed=5)
    mean, rstd = ER.stats(x, 1e-5)
    xh = (x - mean) * rstd
    f = lambda g0: {"s:dx": ER.in_backward(g0, xh, rstd, g0.mean(0), (g0 * xh).mean(0))}
    g = _rand(V, C, seed=6)
    Eset = RE.reach_set(f, g, (17, 3))["s:dx"]
    # every voxel of the plant's own channel (the means carry it there) and no other channel; an E without that column --
    # the plant's voxel alone -- is not what the reference gives
    assert bool(Eset[:, 3].all()) and int(Eset.sum()) == V
    own_voxel_only = torch.zeros_like(Eset)
    own_voxel_only[17, 3] = True
    assert not torch.equal(Eset, own_voxel_only)
    xa = x.t().reshape(1, C, V, 1, 1).clone().requires_grad_(True)
    one = torch.zeros(1, C, V, 1, 1, dtype=torch.float64)
    one[0, 3, 17] = 1.0
    F.instance_norm(xa, eps=1e-5).backward(one)
    assert torch.equal(Eset, xa.grad[0, :, :, 0, 0].t() != 0)


def test_reach_set_of_the_upsampling_adjoint_leaves_out_a_zero_weight_tap():
    d, h, w, C = 3, 4, 5, 2
    f = lambda g0: {"s:g_in": ER.upsample(g0, transpose=True)}
    g = _rand(2 * d, 2 * h, 2 * w, C, seed=7)
    idx = RE.plant_index(g.shape)
    assert idx[2] == 0
    Eset = RE.reach_set(f, g, idx)["s:g_in"]
    # fine x = 0 sits on coarse node 0: the neighbour x = 1 has weight exactly zero and is NOT in E; z and y lie between nodes
    assert bool(Eset[:, :, 0, idx[3]].any()) and not bool(Eset[:, :, 1:, :].any()) and int(Eset.sum()) == 4
    assert not bool(Eset[..., 1 - idx[3]].any())
    y = torch.zeros(1, C, d, h, w, dtype=torch.float64, requires_grad=True)
    one = torch.zeros(1, C, 2 * d, 2 * h, 2 * w, dtype=torch.float64)
    one[0, idx[3], idx[0], idx[1], idx[2]] = 1.0
    F.interpolate(y, scale_factor=2, mode="trilinear", align_corners=True).backward(one)
    assert torch.equal(Eset, y.grad[0].permute(1, 2, 3, 0) != 0)


# ---- overflow on store in the epilogue tests: the classification and the choice of k ---------------------------------------------
def _overflow_fixture():
    """A float64 'reference' at scale 1 with a bound of 2^-11 relative (half an fp16 spacing) and a little more, floored at the
    subnormal quantum, as the element bounds of the epilogue cases are."""
    ref = _rand(4096, 8, seed=11) * 1.5
    return ref, ref.abs() * 2.0 ** -11 * 1.01 + 2.0 ** -24


def test_overflow_exponent_and_shares_come_from_the_reference_alone():
    ref, bound = _overflow_fixture()
    rec = RE.Recorder()
    rec(ref.to(torch.float16), ref, bound, "scale 1")              # (the usual bound check passes on the rounded reference)
    k = rec.exponent()
    assert 0 < k <= RE.K_MAX
    so, sf, sl = rec.shares(k)
    assert RE.shares_ok(so, sf, sl) and 0.05 <= so <= 0.30, (k, so, sf, sl)
    # one power of two less lifts fewer than the requested tenth; the cap holds
    assert rec.shares(k - 1)[0] < 0.10 <= so + sl and rec.exponent(k_max=3) == 3
    # what the scaled run then counts is what was predicted
    chk = RE.OverflowStore(k)
    chk((ref * 2.0 ** k).to(torch.float16), ref * 2.0 ** k, bound * 2.0 ** k, "scaled")
    assert max(abs(a - b) for a, b in zip(chk.shares(), (so, sf, sl))) < 1e-3
    assert not RE.shares_ok(0.005, 0.99, 0.005) and not RE.shares_ok(0.8, 0.2, 0.0) and not RE.shares_ok(0.1, 0.87, 0.03)


def test_overflow_store_tells_a_saturating_store_and_a_stray_inf():
    ref, bound = _overflow_fixture()
    ref, bound = ref * 2.0 ** 17, bound * 2.0 ** 17
    good = ref.to(torch.float16)
    assert bool(good.isinf().any()) and bool(good.isfinite().any())
    RE.OverflowStore(17)(good, ref, bound, "correct store")
    with pytest.raises(pytest.fail.Exception, match="are not \\+-inf with the reference's sign"):
        RE.OverflowStore(17)(ref.clamp(-65504, 65504).to(torch.float16), ref, bound, "saturating store")
    with pytest.raises(pytest.fail.Exception, match="are not \\+-inf with the reference's sign"):
        RE.OverflowStore(17)(-good, ref, bound, "wrong sign")
    stray = good.clone()
    stray[(ref.abs() < 1000).nonzero()[0].tolist()[0], (ref.abs() < 1000).nonzero()[0].tolist()[1]] = float("inf")
    with pytest.raises(pytest.fail.Exception, match="in-range elements are beyond the bound or not finite"):
        RE.OverflowStore(17)(stray, ref, bound, "inf where a finite value belongs")


def test_clamped_gradients_stay_finite_up_to_the_largest_scale():
    import epilogue_layer_cases as E
    g = (_rand(64, 8, seed=12) * 3).to(torch.float16)
    for clip, k in ((E.GRAD_CLIP, RE.K_MAX), (RE.GATE_CLIP, RE.GATE_K_MAX)):
        out = E.scale_grad(g, 2.0 ** k, clip)
        assert bool(out.isfinite().all()) and float(out.abs().max()) == clip * 2.0 ** k
    assert torch.equal(E.scale_grad(g, None), g)
    sub = E.scale_grad(g.clamp(-60, 60), 2.0 ** -20)
    assert float(sub.abs().max()) < 2.0 ** -14 and torch.equal((sub.double() * 2.0 ** 24).round(), sub.double() * 2.0 ** 24)
