"""Opt-in gradient with respect to the network input (SE_UNet(input_grad=True), seunet_net_backward_input).

The gate is the same-choice float64 oracle (tests/forced_oracle.py): the float64 network run with the LeakyReLU signs and
max-pool arg-maxes this forward took, with a float64 leaf as its input, gives the reference x.grad.  forced_step calls
``batch["image"].double()``, which returns a float64 leaf unchanged, so its ``.grad`` is the oracle's input gradient.
The max-pools of the input itself (pool0x / pool1x) are not imposed: the test checks that the oracle's own arg-maxes equal the
path's rule (first strict maximum of each window of the stored copy).  In bf16 / fp16 mode the input is rounded to the storage
type first, so both sides see the same values and take the same pool choices."""
import importlib

import ctypes as C
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# per-input-channel rel-L2 bars against float64 with the same choices.  Measured on MI355X (worst channel): fp32 3.4e-6 ... 4.4e-6
# at 32^3 and 40^3 (every variant below), 9.4e-5 at 1 x 64^3 (see FP32_64_TOL); bf16 1.9e-2 (2 x 32^3) / 2.4e-2 (1 x 64^3); fp16
# 2.4e-3 / 3.1e-3.  fp32 keeps the parameter gate's bar (about 7x measured); bf16 / fp16 about 2x the worst.
TOL = {"fp32": 3e-5, "bf16": 5e-2, "fp16": 6e-3}
# 1 x 64^3 in fp32 measured 9.4e-5 / 6.3e-5 (33 sign / 1 arg-max choice imposed), 25x the 32^3 figure; not explained yet
FP32_64_TOL = 3e-4
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


@pytest.fixture(scope="module")
def orc():
    import seunet_oracle
    return seunet_oracle


def _model(A, orc, inch=2, dtype="fp32", impl=0, wm=1, K=1, input_grad=True, train=False):
    m = A.SE_UNet(in_channel=inch, n_classes=K, width_mult=wm, act_dtype=dtype, conv_impl=impl, input_grad=input_grad)
    m.load_state_dict(orc.deterministic_state_dict(inch, K, wm, seed=0))
    return m.cuda().train(train)


def _batch(orc, batch, size, inch, dtype, seed, K=1):
    b = orc.synthetic_batch(batch, size, inch, seed=seed)
    if dtype in DT:        # the network computes on its rounded copy: give the oracle the same values
        b["image"] = b["image"].to(DT[dtype]).float()
    if K > 1:
        g = torch.Generator().manual_seed(7)
        lab = (torch.rand(batch, K, *size, generator=g) < 0.05).float()
        b = dict(b, label=lab, weight=torch.ones_like(lab), skel=torch.zeros_like(lab))
    return b


def _drops(orc, batch):
    g = torch.Generator().manual_seed(11)
    return (orc.drop_scale_from_uniform(torch.rand(batch, 24, 1, 1, 1, generator=g), 24),
            orc.drop_scale_from_uniform(torch.rand(batch, 12, 1, 1, 1, generator=g), 12))


def _step(A, m, b, stage=1, drops=None, x_grad=True):
    c = {k: v.cuda() for k, v in b.items()}
    x = c["image"].clone().requires_grad_(x_grad)
    e, d = m(x, drop_scales=drops)
    loss = A.fused_stage_loss(stage, e, d, c["label"], c["weight"], c["skel"])
    loss.backward()
    return x, loss


def _first_max_index(t):
    """flat arg-max index of every 2x2x2 window, first strict maximum in (z, y, x) scan order (the kernels' rule), in the
    layout of F.max_pool3d(..., return_indices=True)."""
    n, c, D, H, W = t.shape
    w = t.reshape(n, c, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(n, c, D // 2, H // 2, W // 2, 8)
    q = torch.argmax(w, dim=-1)          # (first occurrence of the maximum)
    zo = torch.arange(D // 2).view(1, 1, -1, 1, 1)
    yo = torch.arange(H // 2).view(1, 1, 1, -1, 1)
    xo = torch.arange(W // 2).view(1, 1, 1, 1, -1)
    return ((2 * zo + (q >> 2)) * H + (2 * yo + ((q >> 1) & 1))) * W + (2 * xo + (q & 1))


def _same_choice_case(A, orc, inch=2, dtype="fp32", impl=0, wm=1, size=(32, 32, 32), batch=2, stage=1, train=False, K=1, seed=3,
                      tol=None):
    import forced_oracle as FO
    b = _batch(orc, batch, size, inch, dtype, seed, K)
    m = _model(A, orc, inch, dtype, impl, wm, K)
    _, _, inter = m.forward_with_intermediates(b["image"].cuda(), FO.LRELU_ORDER)
    m.train(train)
    drops = _drops(orc, batch) if train else None
    x, loss = _step(A, m, b, stage, drops)
    signs, pools = FO.path_choices(inter)
    x64 = b["image"].double().requires_grad_(True)
    of, _, _, lf, nsf, npf = FO.forced_step(orc, dict(b, image=x64), stage, signs, pools, width_mult=wm, drops=drops, n_classes=K)
    # the oracle's own pool(x) / pool(pool(x)) choices are the path's rule on the stored copy
    x1 = F.max_pool3d(x64.detach(), 2, 2)
    for t in (x64.detach(), x1):
        assert torch.equal(F.max_pool3d(t, 2, 2, return_indices=True)[1], _first_max_index(t.float()))
    g, r = x.grad.detach().cpu().double(), x64.grad
    assert x.grad.dtype == torch.float32 and g.shape == r.shape
    errs = [float((g[:, k] - r[:, k]).norm() / r[:, k].norm()) for k in range(inch)]
    print(f"{dtype} inch={inch} impl={impl} wm={wm} {tuple(size)}x{batch} stage={stage} train={train} K={K}: x.grad rel-L2 per "
          f"channel vs same-choice float64 ({nsf} sign / {npf} arg-max choices imposed): " + " ".join("%.2e" % e for e in errs))
    assert max(errs) <= (tol or TOL[dtype]), errs
    return m, x, loss


@pytest.mark.parametrize("stage", [1, 3])
def test_input_grad_same_choice_f64_fp32(A, orc, stage):
    _same_choice_case(A, orc, stage=stage)


@pytest.mark.parametrize("variant", ["in1", "in3", "naive", "width2", "train", "classes3", "64cubed", "ragged40"])
def test_input_grad_variants_fp32(A, orc, variant):
    kw = {"in1": dict(inch=1), "in3": dict(inch=3), "naive": dict(impl=1), "width2": dict(wm=2), "train": dict(train=True),
          "classes3": dict(K=3), "64cubed": dict(batch=1, size=(64, 64, 64), tol=FP32_64_TOL), "ragged40": dict(batch=1, size=(40, 40, 40))}[variant]
    _same_choice_case(A, orc, **kw)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("batch,size", [(2, (32, 32, 32)), (1, (64, 64, 64))])
def test_input_grad_same_choice_f64_low_precision(A, orc, dtype, batch, size):
    _same_choice_case(A, orc, dtype=dtype, batch=batch, size=size)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_parameter_gradients_and_loss_identical_with_input_grad(A, orc, dtype):
    b = _batch(orc, 2, (32, 32, 32), 2, dtype, 5)
    runs = []
    for on in (False, True):
        m = _model(A, orc, dtype=dtype, input_grad=on)
        x, loss = _step(A, m, b, x_grad=on)
        assert (x.grad is not None) == on
        runs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys()
    bad = [n for n in runs[0][1] if not torch.equal(runs[0][1][n], runs[1][1][n])]
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_input_grad_deterministic_and_reads_only_written_memory(A, orc, dtype, monkeypatch):
    host = importlib.import_module("seunet_amd.SE_UNet")
    b = _batch(orc, 2, (32, 32, 32), 2, dtype, 13)
    got = []
    for fill in (None, None, 0x00, 0xFF):
        monkeypatch.setattr(host, "_DEBUG_FILL", fill)
        x, _ = _step(A, _model(A, orc, dtype=dtype), b)
        got.append(x.grad.clone())
    monkeypatch.setattr(host, "_DEBUG_FILL", None)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert torch.equal(got[0], got[1]), "x.grad differs between two identical runs"
    assert torch.equal(got[2], got[3]), "x.grad depends on the prior contents of the buffers"
    assert torch.equal(got[0], got[2])


def _prof_tags(A, fn):
    lib = A._lib.load()
    torch.cuda.synchronize()
    lib.seunet_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 16)
        lib.seunet_prof_report(buf, len(buf))
    finally:
        lib.seunet_prof_enable(0)
    return [line.split("\t")[0] for line in buf.value.decode().splitlines() if line.strip()]


@pytest.mark.parametrize("inch", [2, 3])
def test_no_input_grad_work_unless_the_input_requires_grad(A, orc, inch):
    b = _batch(orc, 2, (32, 32, 32), inch, "bf16", 21)
    ref = _model(A, orc, inch, "bf16", input_grad=False)
    _step(A, ref, b, x_grad=False)
    m = _model(A, orc, inch, "bf16", input_grad=True)
    tags = _prof_tags(A, lambda: _step(A, m, b, x_grad=False))
    assert tags and not [t for t in tags if t.startswith("input_grad:")], tags
    for (n, p), q in zip(m.named_parameters(), ref.parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), n
    # ... and with the input requiring grad the new launch groups show up in the timer
    m2 = _model(A, orc, inch, "bf16", input_grad=True)
    tags = _prof_tags(A, lambda: _step(A, m2, b))
    assert "input_grad:ec1" in tags and "input_grad:unpool1" in tags, tags


def test_fp16_overflow_zeroes_input_and_parameter_gradients(A, orc):
    b = _batch(orc, 1, (32, 32, 32), 2, "fp16", 9)
    m = _model(A, orc, dtype="fp16")
    m.loss_scale = 1e30                     # every scaled gradient leaves half precision's range
    x, _ = _step(A, m, b)
    assert int(m.overflow_steps) == 1
    assert x.grad is not None and not bool(x.grad.any())
    assert all(not bool(p.grad.any()) for p in m.parameters() if p.grad is not None)


def test_learnable_module_in_front_matches_float64(A, orc):
    """A learnable 2 -> 2 1x1x1 conv in front of the network, trained end to end: its parameter gradient is the input gradient
    pulled back through it, against the same module in front of the float64 oracle (same discrete choices)."""
    import forced_oracle as FO
    torch.manual_seed(0)
    pre = torch.nn.Conv3d(2, 2, 1).cuda()
    pre64 = torch.nn.Conv3d(2, 2, 1).double()
    pre64.load_state_dict({k: v.detach().cpu().double() for k, v in pre.state_dict().items()})
    b = orc.synthetic_batch(2, (32, 32, 32), 2, seed=23)
    m = _model(A, orc)
    c = {k: v.cuda() for k, v in b.items()}
    y = pre(c["image"])
    _, _, inter = m.forward_with_intermediates(y.detach(), FO.LRELU_ORDER)
    e, d = m(y)
    A.fused_stage_loss(1, e, d, c["label"], c["weight"], c["skel"]).backward()
    signs, pools = FO.path_choices(inter)
    y64 = pre64(b["image"].double())
    y64 = y64 + (y.detach().cpu().double() - y64).detach()       # the path's f32 values, the float64 module's gradient
    FO.forced_step(orc, dict(b, image=y64), 1, signs, pools)
    for name in ("weight", "bias"):
        g, r = getattr(pre, name).grad.detach().cpu().double(), getattr(pre64, name).grad
        err = float((g - r).norm() / r.norm())
        print(f"front conv {name} gradient rel-L2 vs same-choice float64: {err:.2e}")
        assert err <= TOL["fp32"], (name, err)


def test_full_size_bf16(A, orc):
    b = _batch(orc, 4, (128, 128, 128), 2, "bf16", 2)
    grads, gx = [], []
    for on in (False, True, True):
        m = _model(A, orc, dtype="bf16", input_grad=on)
        x, _ = _step(A, m, b, x_grad=on)
        grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
        if on:
            gx.append(x.grad.clone())
        del m, x
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in gx)
    assert torch.equal(gx[0], gx[1])
    for run in grads[1:]:
        bad = [n for n in grads[0] if not torch.equal(grads[0][n], run[n])]
        assert not bad, bad
