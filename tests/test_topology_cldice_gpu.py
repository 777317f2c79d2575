"""soft_skeleton / soft_cldice_loss / cldice_score on the GPU against tests/cldice_oracle.py.

The forward is compared bit for bit with the float32 oracle.  Every bound on a value or a gradient is made from two ORACLE runs
(float32 against float64 on the same input), never from the code under test; each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import cldice_oracle as O

pytestmark = pytest.mark.gpu

ALL_SHAPES = O.PARITY_SHAPES + O.DEGENERATE_SHAPES
TIED_SHAPES = O.PARITY_SHAPES[:2]


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def same_f32_bits(got, want):
    got = got.cpu()
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
    ne = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(ne.any()), f"{int(ne.sum())} of {ne.numel()} voxels differ, first at {tuple(int(v) for v in ne.nonzero()[0])}"


def run(A, p, t, iters, scale=None, **kw):
    """(loss, gradient) of the code under test, both on the host"""
    x = p.cuda().requires_grad_(True)
    loss = A.soft_cldice_loss(x, t.cuda(), iters, **kw)
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu(), x.grad.cpu()


def check_gradient(g, g_ref, g_f32, what):
    """max|g - g_ref| / max|g_ref| within 4x the same ratio of the float32 oracle (a different but fixed summation order)"""
    top = float(g_ref.abs().max())
    if top == 0.0:
        print(f"{what}: the oracle's gradient is zero everywhere")
        assert not bool(g.any())
        return
    ratio, allowed = O.rel_max(g, g_ref), 4 * O.rel_max(g_f32, g_ref)
    print(f"{what}: gradient ratio {ratio:.3e}, allowed {allowed:.3e}")
    assert ratio <= allowed


@pytest.mark.parametrize("iters", O.ITERS)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_forward_is_the_float32_oracle_bit_for_bit(A, shape, iters):
    p, t = O.case(shape)
    same_f32_bits(A.soft_skeleton(p.cuda(), iters), O.soft_skeleton_a(p, iters))
    same_f32_bits(A.soft_skeleton(t.cuda(), iters), O.soft_skeleton_b(t, iters))      # the binary target: ties everywhere


@pytest.mark.parametrize("shape", TIED_SHAPES)
def test_forward_on_tied_inputs(A, shape):
    binary, rounded, _ = O.tied_inputs(shape)
    for p in (binary, rounded):
        for iters in O.ITERS:
            same_f32_bits(A.soft_skeleton(p.cuda(), iters), O.soft_skeleton_b(p, iters))


@pytest.mark.parametrize("iters", O.ITERS)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_value_and_gradient_on_distinct_inputs(A, shape, iters):
    p, t = O.case(shape)
    ref = O.reference(shape, iters)
    loss, g = run(A, p, t, iters)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    err, allowed = abs(float(loss) - float(ref["l64"])), max(2.0 ** -22, 4 * abs(float(ref["l32"]) - float(ref["l64"])))
    print(f"{shape} iters={iters}: loss {float(loss):.9f}, oracle {float(ref['l64']):.9f}, error {err:.3e}, allowed {allowed:.3e}")
    assert err <= allowed
    check_gradient(g, ref["g64"], ref["g32"], f"{shape} iters={iters}")


@pytest.mark.parametrize("shape", TIED_SHAPES)
def test_gradient_on_tied_inputs_follows_the_stated_choices(A, shape):
    binary, rounded, t = O.tied_inputs(shape)
    for name, p in (("binary", binary), ("one decimal", rounded)):
        l64, g64, _ = O.loss_and_grad_b(p, t, 3, 1.0, torch.float64)
        l32, g32, _ = O.loss_and_grad_b(p, t, 3, 1.0, torch.float32)
        loss, g = run(A, p, t, 3)
        err, allowed = abs(float(loss) - float(l64)), max(2.0 ** -22, 4 * abs(float(l32) - float(l64)))
        print(f"{shape} {name}: loss error {err:.3e}, allowed {allowed:.3e}")
        assert err <= allowed
        check_gradient(g, g64, g32, f"{shape} {name}")


def test_saved_state_and_upstream_gradient(A):
    p, t = O.case((3, 5, 33, 70))
    l3, g3 = run(A, p, t, 3)
    l3b, g3b = run(A, p, t, 3)
    assert torch.equal(l3.view(torch.int32), l3b.view(torch.int32)) and torch.equal(g3.view(torch.int32), g3b.view(torch.int32))
    x6, x3 = p.cuda().requires_grad_(True), p.cuda().requires_grad_(True)
    loss6 = A.soft_cldice_loss(x6, t.cuda(), 6)                 # two graphs alive at once, each with a saved state of its own
    loss3 = A.soft_cldice_loss(x3, t.cuda(), 3)
    loss6.backward()
    loss3.backward()
    assert torch.equal(x3.grad.cpu().view(torch.int32), g3.view(torch.int32))
    _, g6 = run(A, p, t, 6)
    assert torch.equal(x6.grad.cpu().view(torch.int32), g6.view(torch.int32))
    _, g3_after = run(A, p, t, 3)                               # iters = 3 after iters = 6
    assert torch.equal(g3_after.view(torch.int32), g3.view(torch.int32))
    _, g_twice = run(A, p, t, 3, scale=2.0)
    assert torch.equal(g_twice, 2 * g3) and float(g3.abs().max()) > 0
    cached = A.soft_skeleton(t.cuda(), 3)
    lc, gc = run(A, p, t, 3, target_skeleton=cached)
    assert torch.equal(lc, l3) and torch.equal(gc.view(torch.int32), g3.view(torch.int32))


def test_batch_independence(A):
    p, _ = O.case((2, 7, 9, 11))
    whole = A.soft_skeleton(p.cuda(), 3).cpu()
    for v in range(2):
        same_f32_bits(A.soft_skeleton(p[v:v + 1].cuda(), 3), whole[v:v + 1])
    five = A.soft_skeleton(p.reshape(2, 1, 7, 9, 11).cuda(), 3)      # (batch, channel, D, H, W)
    assert five.shape == (2, 1, 7, 9, 11)
    same_f32_bits(five.reshape(2, 7, 9, 11), whole)


@pytest.mark.parametrize("shape", TIED_SHAPES)
def test_sums_are_additive_over_the_batch(A, shape):
    """what group= relies on: the all-reduced sums of the ranks' sub-batches are the sums of the whole batch"""
    from seunet_amd import losses
    p, t = (v[:2].cuda().contiguous() for v in O.case(shape))

    def sums(p, t):
        return losses._cldice_sums(losses._skeleton(p, 3, False)[0], t, losses._skeleton(t, 3, False)[0], p).cpu()
    whole, parts = sums(p, t), sums(p[:1].contiguous(), t[:1].contiguous()) + sums(p[1:].contiguous(), t[1:].contiguous())
    rel = ((whole - parts).abs() / whole.abs()).max()
    print(f"{shape}: sums {whole.tolist()}, relative difference {float(rel):.3e}")
    assert float(whole.min()) > 0 and float(rel) <= 1e-12
    sp, st = O.soft_skeleton_a(p.cpu(), 3).double(), O.soft_skeleton_a(t.cpu(), 3).double()      # float32 skeletons, float64 sums
    want = torch.stack([(sp * t.cpu().double()).sum(), sp.sum(), (st * p.cpu().double()).sum(), st.sum()])
    assert float(((whole - want).abs() / want.abs()).max()) <= 1e-12


def test_cldice_score(A):
    import skeleton_oracle as SO
    label, skel, leak, leak_skel = O.tube_case()
    got = A.cldice_score(torch.from_numpy(leak).cuda(), torch.from_numpy(label).cuda(), torch.from_numpy(leak_skel).cuda(),
                         torch.from_numpy(skel).cuda(), return_parts=True)
    assert got == O.cldice_score(leak, label, leak_skel, skel) + (O.cldice_counts(leak, label, leak_skel, skel),)
    assert A.cldice_score(leak, label, leak_skel, skel) == O.cldice_score(leak, label, leak_skel, skel)[0]      # numpy in
    # thinning the masks itself: the skeletons are tests/skeleton_oracle.py's
    p, t = O.case((2, 7, 9, 11))
    vp, vl = (p[0] > 0.6).numpy().astype(np.uint8), t[0].numpy().astype(np.uint8)
    want = O.cldice_score(vp, vl, SO.skeletonize(vp)[0], SO.skeletonize(vl)[0])
    got = A.cldice_score(torch.from_numpy(vp).cuda(), torch.from_numpy(vl).cuda(), return_parts=True)
    print("cldice_score:", got, "oracle", want)
    assert got[:3] == want and 0 < want[0] < 1
    empty = np.zeros_like(vl)
    assert A.cldice_score(empty, vl) == 0.0 and A.cldice_score(vl, empty) == 0.0


def test_through_the_network(A):
    """one stage-1 step of SE_UNet at 1x2x32^3 in fp32 with dice + 0.5 soft clDice on the decoder head, one backward()"""
    import seunet_oracle as orc
    b = orc.synthetic_batch(1, (32, 32, 32), 2, seed=5)
    grads = []
    for alpha in (0.0, 0.5):
        m = A.SE_UNet(2, 1, act_dtype="fp32")
        m.load_state_dict(orc.deterministic_state_dict(2, 1, 1, 0))
        m = m.cuda().eval()
        pred_en, pred_de = m(b["image"].cuda())
        label = b["label"].cuda()
        loss = A.fused_stage_loss(1, pred_en, pred_de, label)
        if alpha:
            loss = loss + alpha * A.soft_cldice_loss(torch.sigmoid(pred_de), label)
        loss.backward()
        grads.append({k: v.grad.detach().cpu() for k, v in m.named_parameters() if v.grad is not None})
    dice, both = grads
    assert dice.keys() == both.keys() and len(dice) > 0
    assert all(bool(torch.isfinite(g).all()) for g in both.values())
    moved = [k for k in dice if not torch.equal(dice[k], both[k])]
    print(f"{len(moved)} of {len(dice)} parameter gradients differ from the Dice-only step's")
    assert "dc5.conv1.weight" in moved and len(moved) > len(dice) // 2
