"""The backward walk defers each weight gradient's slab reduction into the next finalize launch (csrc/net.cpp, ``pending``;
csrc/wgrad.h, ``WgReduceJob``).  Deferred or immediate, on any stream, with any layers frozen, every gradient has the same bits.

``seunet_debug_net_wgrad_defer(on)`` (diagnostic export, not in the public header, process-global, default on) switches the
deferral: off = every weight gradient of the walk reduces its slabs at once in a launch of its own, as the op-level entry points
always do.

Which kernels a plan routes is asserted from ``SE_UNet.conv_plan`` when the module is collected (host only), so that a change of
the routing that empties a row of the table below is seen here and not as a silently weaker test."""
import importlib

import pytest
import torch

from side_stream import run_behind_delay

pytestmark = pytest.mark.gpu

GATED = ["ec1", "ec2", "ec3", "ec4", "ec5", "ec6", "ec7", "ec8", "ec9", "ec10", "ec11", "ec12", "dc1", "dc2", "dc3", "dc4", "dc5", "dc6"]
CAT = ["ec33", "ec63", "ec93", "ec123", "dc22", "dc42"]

# (batch, in_channel, edge, dtype): what the plan reaches
PLANS = [
    (1, 2, 32, "bf16"),    # Stream (ec1, ec2, ec3, dc6), March on the other dilation-2 layers, Tiled elsewhere; every finalize host
    (1, 2, 32, "fp32"),    # Tiled throughout
    (1, 2, 48, "bf16"),    # dc5's two-source weight gradient on March
    (2, 2, 128, "bf16"),   # the smallest plan that routes Wgrad1x1 (ec63)
    (1, 3, 32, "fp32"),    # materialised x-branch: two weight gradients in one op, the flush before the second
]


def _plan(batch, inch, edge, dtype):
    from seunet_amd import _lib
    from seunet_amd.SE_UNet import conv_plan, make_desc
    _lib.load()
    return {c["name"]: c for c in conv_plan(make_desc(batch, inch, 1, edge, edge, edge, 1, _lib.dtype_code(dtype), 0, 0.01))}


def _routed(plan, kernel):
    return sorted(n for n, c in plan.items() if c["wgrad"] == kernel)


def _check_routing():
    p = _plan(1, 2, 32, "bf16")
    assert sorted(p) == sorted(GATED + CAT)
    assert _routed(p, "Stream") == sorted(["ec1", "ec2", "ec3", "dc6"]), _routed(p, "Stream")
    dil2 = sorted(n for n, c in p.items() if c["dilation"] == 2 and c["wgrad"] != "Stream")
    assert dil2 == sorted(["ec5", "ec6", "ec8", "ec9"]) and _routed(p, "March") == dil2, (dil2, _routed(p, "March"))
    assert _routed(p, "Tiled") == sorted(set(GATED + CAT) - {"ec1", "ec2", "ec3", "dc6"} - set(dil2))
    # the finalize hosts: gated blocks with one gate and with two; aggregation blocks with a recomputed x-branch and with none
    assert all(p[n]["x_name"] and not p[n]["x_materialised"] for n in ("ec33", "ec63", "ec93"))
    assert all(p[n]["x_name"] is None for n in ("ec123", "dc22", "dc42"))
    p = _plan(1, 2, 32, "fp32")
    assert _routed(p, "Tiled") == sorted(GATED + CAT)
    p = _plan(1, 2, 48, "bf16")
    assert p["dc5"]["wgrad"] == "March" and len(p["dc5"]["src_c"]) == 2, p["dc5"]
    assert _plan(1, 2, 32, "bf16")["dc5"]["wgrad"] == "Tiled"               # (which the 32^3 plan does not reach)
    p = _plan(2, 2, 128, "bf16")
    assert _routed(p, "Wgrad1x1") == ["ec63"], _routed(p, "Wgrad1x1")
    assert _routed(_plan(1, 2, 128, "bf16"), "Wgrad1x1") == []               # (nor does one sample)
    p = _plan(1, 3, 32, "fp32")
    assert all(p[n]["x_materialised"] and p[n]["x_wgrad"] == "Tiled" for n in ("ec33", "ec63", "ec93")), p["ec33"]


_check_routing()


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


def build(A, orc, inch, dtype, frozen=()):
    m = A.SE_UNet(in_channel=inch, n_classes=1, act_dtype=dtype, conv_impl=0)
    m.load_state_dict(orc.deterministic_state_dict(inch, 1, 1, seed=0))
    for name in frozen:
        getattr(m, name).conv1.weight.requires_grad = False
    return m.cuda().eval()


def set_defer(A, on):
    f = A._lib.load().seunet_debug_net_wgrad_defer                 # diagnostic export, not in the public header
    return f(1 if on else 0)


def step(A, m, x, lab):
    """One forward + stage-1 loss + backward: the loss, and every gradient by parameter name."""
    for p in m.parameters():
        p.grad = None
    e, d = m(x)
    loss = A.fused_stage_loss(1, e, d, lab)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def flat(grads):
    """The whole gradient buffer: every live parameter's gradient, in parameter order."""
    return torch.cat([g.reshape(-1) for g in grads.values()])


def run(A, orc, monkeypatch, plan, defer, fill, frozen=()):
    batch, inch, edge, dtype = plan
    host = importlib.import_module("seunet_amd.SE_UNet")      # (the module; the package attribute of that name is the class)
    b = orc.synthetic_batch(batch, (edge, edge, edge), inch, seed=21)
    monkeypatch.setattr(host, "_DEBUG_FILL", fill)            # workspace, outputs and gradient buffer start as these bytes
    was = set_defer(A, defer)
    try:
        loss, grads = step(A, build(A, orc, inch, dtype, frozen), b["image"].cuda(), b["label"].cuda())
        torch.cuda.synchronize()
    finally:
        set_defer(A, was)
        monkeypatch.setattr(host, "_DEBUG_FILL", None)
    return loss, grads


def test_the_switch_is_on_by_default_and_reports_the_previous_setting(A):
    assert set_defer(A, False) == 1 and set_defer(A, True) == 0 and set_defer(A, True) == 1


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: "-".join(str(v) for v in p))
def test_deferred_equals_immediate(A, orc, monkeypatch, plan):
    """Case 1: the same step with the reductions deferred (over a 0xFF workspace) and immediate (over a 0x5A one)."""
    loss_d, g_d = run(A, orc, monkeypatch, plan, True, 0xFF)
    loss_i, g_i = run(A, orc, monkeypatch, plan, False, 0x5A)
    assert torch.isfinite(loss_d) and torch.equal(loss_d, loss_i)
    assert list(g_d) == list(g_i) and len(g_d) == 116
    fd, fi = flat(g_d), flat(g_i)
    assert fd.numel() == fi.numel() and bool(torch.isfinite(fd).all())
    bad = [n for n in g_d if not torch.equal(g_d[n], g_i[n])]
    assert torch.equal(fd, fi), bad
    assert float(g_d["dc5.conv1.weight"].abs().max()) > 0.0 and float(g_d["ec1.conv1.weight"].abs().max()) > 0.0


def test_frozen_layers_leave_the_other_gradients_as_they_are(A, orc, monkeypatch):
    """Case 2: conv1.weight frozen on every other block.  Such a block computes no weight gradient, so the job pending from
    the block before it survives the op, and the finalize launch after it has no job to carry."""
    plan = (1, 2, 32, "bf16")
    order = list(_plan(*plan))                                 # the blocks in execution order
    frozen = order[::2]
    assert {"ec1", "ec3", "dc22", "dc5"} <= set(frozen) and {"ec2", "ec33", "dc6"}.isdisjoint(frozen)   # (both block kinds, either way)
    _, g_all = run(A, orc, monkeypatch, plan, True, 0xFF)
    for defer, fill in ((True, 0x5A), (False, 0xFF)):
        _, g = run(A, orc, monkeypatch, plan, defer, fill, frozen)
        assert sorted(set(g_all) - set(g)) == sorted(n + ".conv1.weight" for n in frozen)
        bad = [n for n in g if not torch.equal(g[n], g_all[n])]
        assert not bad, (defer, bad)


def test_side_stream_equals_default_stream(A, orc):
    """Case 3: the step issued under a side stream whose inputs arrive late; every rider launches on that stream."""
    plan = (1, 2, 32, "bf16")
    real = orc.synthetic_batch(1, (32, 32, 32), 2, seed=21)
    poison = orc.synthetic_batch(1, (32, 32, 32), 2, seed=121)
    m = build(A, orc, 2, "bf16")
    torch.cuda.synchronize()
    assert set_defer(A, True) == 1
    op = lambda x, lab: step(A, m, x, lab)
    want_loss, want = op(real["image"].cuda(), real["label"].cuda())
    torch.cuda.synchronize()
    got_loss, got = run_behind_delay(lambda: [real["image"], real["label"]], lambda: [poison["image"], poison["label"]], op,
                                     no_host_sync=True, label="deferred weight gradients")
    assert torch.equal(got_loss, want_loss) and list(got) == list(want)
    assert torch.equal(flat(got), flat(want)), [n for n in want if not torch.equal(got[n], want[n])]


# ---- the reduction's own bits ------------------------------------------------------------------------------------------------
# (cin, cout, taps): two, four, eight and two (ci, co) combos of the tiled kernel, the last with channel padding
REDUCE_CHANNELS = [(32, 32, 27), (64, 64, 27), (128, 64, 27), (56, 32, 1)]
REDUCE_DIMS = [(1, 12, 16, 32), (4, 32, 32, 32)]
SLAB_PREFIX = 256                                              # bytes of the workspace in front of the slabs (wgrad.h)


def host_sum_in_kernel_order(slabs):
    """``slabs`` [combo][slab][element] f64 -> [combo][element]: the order wgrad.h documents.  Thread group p of 16 sums the slabs
    p, p + 32, ... on one chain and p + 16, p + 48, ... on a second, adds the two, and the 16 group sums are added in group order."""
    import numpy as np
    nslab = slabs.shape[1]
    groups = []
    for part in range(16):
        s0, s1 = np.zeros_like(slabs[:, 0]), np.zeros_like(slabs[:, 0])
        k = part
        while k + 16 < nslab:
            s0 = s0 + slabs[:, k]
            s1 = s1 + slabs[:, k + 16]
            k += 32
        if k < nslab:
            s0 = s0 + slabs[:, k]
        groups.append(s0 + s1)
    t = groups[0]
    for q in range(1, 16):
        t = t + groups[q]
    return t


@pytest.mark.parametrize("dims", REDUCE_DIMS, ids=lambda d: "x".join(str(v) for v in d))
@pytest.mark.parametrize("cin,cout,taps", REDUCE_CHANNELS)
def test_reduction_equals_the_f64_host_sum_in_the_documented_order(A, cin, cout, taps, dims):
    """Case 4: the tiled weight gradient through the op-level entry point over a workspace of 0xFF bytes (NaN as f32), the
    slabs it left read back, summed on the host in f64 in the documented order and scattered by the tiled kernel's map."""
    import numpy as np
    from seunet_amd import _lib, ops as S
    lib = _lib.load()
    n, d, h, w = dims
    g = torch.Generator().manual_seed(cin * 1000 + cout + d)
    cpad = (cin + 7) // 8 * 8
    x = torch.randn((n, d, h, w, cpad), generator=g).to(torch.bfloat16).cuda()
    dy = torch.randn((n, d, h, w, cout), generator=g).to(torch.bfloat16).cuda()
    k = 3 if taps == 27 else 1
    dw = torch.empty((cout, cin, k, k, k), dtype=torch.float32, device="cuda")
    nbytes = lib.seunet_conv3d_wgrad_workspace_bytes(taps, cin, cout)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    _lib.check(lib.seunet_conv3d_wgrad(_lib.BF16, _lib.CONV_TILED, taps, 1, 1, _lib.ptr_array([x]), _lib.int_array([cpad]), cin,
                                       dy.data_ptr(), cout, dw.data_ptr(), ws.data_ptr(), nbytes, S._dims_cl(dy), _lib.stream_ptr()),
               "conv3d_wgrad")
    torch.cuda.synchronize()
    f = ws[SLAB_PREFIX:SLAB_PREFIX + (nbytes - SLAB_PREFIX) // 4 * 4].view(torch.float32).cpu().numpy()
    written = ~np.isnan(f)
    total = int(written.sum())
    assert total > 0 and written[:total].all() and not written[total:].any(), "the slabs lie back to back behind the prefix"
    co_tiles = (cout + 31) // 32
    combos, per = ((cin + 31) // 32) * co_tiles, taps * 1024
    assert total % (combos * per) == 0, (total, combos, per)
    nslab = total // (combos * per)
    assert nslab >= 2                                            # (more than one slab per combo: there is something to order)
    want = host_sum_in_kernel_order(f[:total].astype(np.float64).reshape(combos, nslab, per)).astype(np.float32)
    # element e = (tap, ci, co) of a slab of the 32 x 32 combo -> dW (cout, cin, taps); channel padding dropped
    e = np.arange(per)
    ref = np.zeros((cout, cin, taps), dtype=np.float32)
    for combo in range(combos):
        tap, ci, co = e >> 10, (combo // co_tiles) * 32 + ((e >> 5) & 31), (combo % co_tiles) * 32 + (e & 31)
        keep = (ci < cin) & (co < cout)
        ref[co[keep], ci[keep], tap[keep]] = want[combo][keep]
    got = dw.cpu().numpy().reshape(cout, cin, taps)
    assert np.isfinite(got).all() and float(np.abs(got).max()) > 0.0
    diff = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    assert diff == 0, f"{diff} of {got.size} elements differ from the f64 host sum in the kernel's order"
