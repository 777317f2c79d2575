"""The volume operations (distance transform, preparation weights, skeleton, parsing, post- and pre-processing, input
pipeline, window loop), AdamW and the losses over dirty scratch memory, with red zones around every buffer
(tests/guarded_alloc.py).

Each operation runs three times -- scratch and outputs pre-filled with 0x00, with 0xFF and with seeded random bytes, inputs
copied into red-zoned buffers -- and must (a) leave every red zone as it was, (b) give the same bits all three times and
(c) equal the reference the suite already trusts for it (scipy, the recorded fixtures, the oracles), never another run of the
code under test.  Shapes are the smallest that cross the boundaries these kernels have: 64-voxel words, 4 words per block,
256 lines per block, extent-1 axes."""
import os

import numpy as np
import pytest
import torch

import guarded_alloc as G
from guarded_alloc import check, guard, guarded_allocations, three_fills

import parse_oracle as po  # noqa: F401  (tests/ on the path, as the other GPU files rely on)
import skeleton_oracle as so

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    """A host array or tensor on the device, inside a red-zoned buffer of the active context."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return guard(t.cuda())


def host(t):
    return t.cpu().numpy()


# ---- positive controls: torch ops only ------------------------------------------------------------------------------
def test_control_an_unwritten_buffer_is_flagged_by_the_fills(A):
    with pytest.raises(AssertionError, match="fill 0x00 against fill 0xFF"):
        three_fills(lambda: torch.empty(1000, dtype=torch.int32, device="cuda").sum(), "control")


def test_control_a_write_past_the_payload_is_flagged_by_check(A):
    with guarded_allocations("random", 7) as g:
        t = torch.empty(129, dtype=torch.int64, device="cuda")
        t.fill_(3)
        assert check() == 1
        r = g.records[0]
        past = r.base[r.off + G.RED_ZONE:].view(torch.int64)        # the test's own buffer, seen from the payload's first byte
        assert past.data_ptr() == t.data_ptr()
        past[129] = 3                                                # one element past the payload
        with pytest.raises(AssertionError, match=r"back zone, .* first at payload offset 103\d, last at payload offset 103\d"):
            check()


# ---- EDT ---------------------------------------------------------------------------------------------------------------
EDT_SHAPES = [(1, 1, 1), (7, 1, 9), (1, 30, 31), (5, 40, 37), (3, 5, 257), (2, 129, 3), (9, 10, 11)]


def _edt_volume(shape, kind):
    if kind == "lattice":
        v = np.ones(shape, np.uint8)
        v[::4, ::3, ::5] = 0
        return v
    share = {"sparse": 0.01, "half": 0.5}[kind]
    rng = np.random.default_rng(1000 * sum(shape) + int(share * 100))
    v = (rng.random(shape) >= share).astype(np.uint8)
    if v.all():
        v.flat[v.size - 1] = 0            # (the transform is undefined without a zero; (1, 1, 1) holds a zero in every kind)
    return v


@pytest.mark.parametrize("kind", ["lattice", "sparse", "half"])
@pytest.mark.parametrize("shape", EDT_SHAPES)
def test_distance_transform(A, shape, kind):
    from scipy import ndimage
    v = _edt_volume(shape, kind)
    ref_dist, ref_ind = ndimage.distance_transform_edt(v, return_indices=True)
    sq, dist, ind = three_fills(lambda: A.distance_transform_edt(dev(v), return_indices=True, return_sqdist=True), "EDT")
    assert np.array_equal(host(ind), ref_ind.astype(np.int32))
    assert np.array_equal(host(dist).view(np.int64), ref_dist.view(np.int64))
    ref_sq = ((ref_ind.astype(np.int64) - np.indices(shape)) ** 2).sum(0)
    assert np.array_equal(host(sq).astype(np.int64), ref_sq)
    only = three_fills(lambda: A.distance_transform_edt(dev(v)), "EDT")
    assert torch.equal(only, dist)


# ---- preparation weights and candidates -------------------------------------------------------------------------------------
PREP = np.load(os.path.join(GOLDEN, "prep_known.npz"))


@pytest.mark.parametrize("c", range(int(PREP["ncase"])))
def test_prep_weights_and_candidates(A, c):
    g, p = PREP, f"case{c}_"

    def op():
        label, skeleton, pred = dev(g[p + "label"]), dev(g[p + "skeleton"]), dev(g[p + "pred"])
        w, br = A.break_weight(label, pred, skeleton)
        return A.hard_mining_candidates(label, skeleton, pred), A.lib_weight(label), w, br, A.CandidateSet.from_mask(br)
    (loc_skel, loc_small), lib, w_br, _, loc_break = three_fills(op, "prep")
    for cs, ref in ((loc_skel, np.where(g[p + "loc_skeleton"])), (loc_small, np.where(g[p + "loc_small"])),
                    (loc_break, tuple(g[p + "loc_break"].astype(np.int64)))):
        assert len(cs[0]) == len(ref[0])
        assert all(np.array_equal(a, b) for a, b in zip(cs.to_numpy(), ref))
    assert lib.dtype == torch.float16 and np.array_equal(host(lib).view(np.int16), g[p + "lib"].view(np.int16))
    assert np.array_equal(host(w_br).view(np.int16), g[p + "w_br"].view(np.int16))


# ---- skeleton ------------------------------------------------------------------------------------------------------------
def _skeleton_case(name):
    if name == "dense":
        v = (np.random.default_rng(7).random((5, 6, 128)) < 0.7).astype(np.uint8)
        return (v,) + so.skeletonize(v)
    return so.solved(name)


@pytest.mark.parametrize("name", ["tree", "noise", "two", "line", "empty", "dense"])
def test_skeletonize(A, name):
    v, want, passes = _skeleton_case(name)
    got, got_passes = three_fills(lambda: A.skeletonize_3d(dev(v), return_passes=True), "skeleton")
    assert np.array_equal(host(got), want) and got_passes == passes


# ---- parsing ---------------------------------------------------------------------------------------------------------------
def _parse_cases():
    z = np.load(os.path.join(GOLDEN, "parse_known.npz"))
    return [{k[len(f"case{i}_"):]: z[k] for k in z.files if k.startswith(f"case{i}_")} for i in range(int(z["ncase"]))]


PARSE = _parse_cases()


@pytest.mark.parametrize("ci", range(len(PARSE)))
def test_parsing_stages(A, ci):
    c = PARSE[ci]
    num0 = int(c["num0"])
    lut = np.random.default_rng(5).integers(0, 3000, num0 + 1).astype(np.int32)
    parsing0 = c["parsing0"].astype(np.int32)

    def op():
        return (A.skeleton_parsing(dev(c["skeleton"])),
                A.tree_parsing_func(dev(c["skeleton_parse"]), dev(c["label"]), dev(c["cd"].astype(np.int32))),
                A.label_adjacency(dev(parsing0), num0), A.relabel(dev(parsing0), lut))
    (parse, cd, num), assigned, (counts, ad), relabelled = three_fills(op, "parsing")
    assert num == num0 and np.array_equal(host(parse), c["skeleton_parse"]) and np.array_equal(host(cd), c["cd"].astype(np.int32))
    assert np.array_equal(host(assigned), parsing0)
    assert np.array_equal(counts, c["counts0"]) and np.array_equal(ad, c["ad0"])
    assert np.array_equal(host(relabelled), lut[parsing0])


@pytest.mark.parametrize("ci", range(len(PARSE)))
def test_tree_parsing(A, ci):
    c = PARSE[ci]

    def op():
        label, skeleton = dev(c["label"]), dev(c["skeleton"])
        return A.tree_parsing(label, skeleton, return_num=True), A.tree_parsing(label, skeleton, refine=False, return_num=True)
    (got, num), (plain, num0) = three_fills(op, "parsing")
    assert num == int(c["num"]) and np.array_equal(host(got), c["parsing"].astype(np.int32))
    assert num0 == int(c["num0"]) and np.array_equal(host(plain), c["parsing0"].astype(np.int32))


# ---- post-processing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("shape", [(5, 7, 63), (5, 7, 65), (17, 3, 129)])
def test_double_threshold_iteration(A, shape, kind):
    import dti_oracle as do
    v = np.random.default_rng(sum(shape) + len(kind)).random(shape)
    if kind == "smooth":
        for ax in range(3):
            v = (v + np.roll(v, 1, ax) + np.roll(v, -1, ax)) / 3.0
        v = (v - v.min()) / max(v.max() - v.min(), 1e-9)
    for h, l in ((0.5, 0.4), (0.62, 0.37)):
        for pd in ("float64", "float32"):
            got = three_fills(lambda: A.double_threshold_iteration(dev(v), h, l, pred_dtype=pd), "double threshold")
            assert got.dtype == torch.uint8
            np.testing.assert_array_equal(host(got), do.double_threshold_iteration(v, h, l, pd).astype(np.uint8))


@pytest.mark.parametrize("kind", ["sparse", "dense", "blobs"])
@pytest.mark.parametrize("shape", [(9, 8, 63), (9, 8, 65), (17, 5, 130)])
def test_largest_component_and_maximum_3d(A, shape, kind):
    import components_oracle as co
    from test_components_gpu import _volume
    v = _volume(kind, shape, 31 * sum(shape) + len(kind))
    assert v.any()
    got = three_fills(lambda: A.largest_component(dev(v)), "components")
    np.testing.assert_array_equal(host(got), co.largest_component(v))
    try:
        want_m = co.maximum_3d(v)
    except IndexError:
        def refused():
            with pytest.raises(IndexError):
                A.maximum_3d(dev(v))
        three_fills(refused, "components")
        return
    got_m = three_fills(lambda: A.maximum_3d(dev(v)), "components")
    np.testing.assert_array_equal(host(got_m).astype(bool), want_m)


def test_evaluation_case(A):
    import components_oracle as co
    pred, label, skel, parsing = co.synthetic_tree((48, 40, 56), 7)
    got = three_fills(lambda: A.evaluation_case(dev(pred), dev(label), dev(skel), dev(parsing)), "evaluation_case")
    assert tuple(got) == tuple(co.evaluation_case(pred, label, skel, parsing))


# ---- preprocessing ------------------------------------------------------------------------------------------------------------
LUNG = np.load(os.path.join(GOLDEN, "lung_known.npz"))


def test_preprocess_ct_prepro_mode(A):
    data_cut, lung_mask, box = three_fills(lambda: A.preprocess_ct(dev(LUNG["a_ct"])), "preprocessing")
    assert np.array_equal(host(data_cut), LUNG["a_data_cut"]) and np.array_equal(host(lung_mask), LUNG["a_lung_mask"])
    assert np.array_equal(box, LUNG["a_box"])


def test_preprocess_ct_prediction_mode(A):
    """Fixture ``d`` is the one recorded in prediction mode; on ``a`` that mode is checked against tests/lung_oracle.py."""
    import lung_oracle as LO
    for key, want in (("d", LUNG["d_data_cut"]), ("a", LO.preprocess_ct(LUNG["a_ct"], mode="prediction")[0])):
        cp, m, b = three_fills(lambda: A.preprocess_ct(dev(LUNG[f"{key}_ct"]), mode="prediction"), "preprocessing")
        assert m is None and b is None and cp.dtype == torch.int16 and np.array_equal(host(cp), want)


def test_cut_mask(A):
    """``e`` is the labelled mask of fixture ``a``'s scan (same box); ``e2`` the small one."""
    assert np.array_equal(LUNG["e_box"], LUNG["a_box"])
    for key in ("e", "e2"):
        out = three_fills(lambda: A.cut_mask(dev(LUNG[f"{key}_label"]), LUNG[f"{key}_box"]), "preprocessing")
        assert out.dtype == torch.uint8 and np.array_equal(host(out), LUNG[f"{key}_mask_cut"])


def test_get_l(A):
    import lung_oracle as LO
    from test_preprocess_gpu import blob_volume
    v = blob_volume(np.random.default_rng(2), (64, 70, 12), 12)
    for T in (-950.0, -500.0, 40.0, 40.5):
        got = three_fills(lambda: A.get_l(dev(v), T, 100), "preprocessing")
        assert np.array_equal(host(got), LO.get_l(v, T, 100)), T


# ---- input pipeline -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", list(range(16)))
def test_crop_batch_axis_maps(A, code):
    import pipeline_oracle as po
    from test_pipeline_gpu import _case
    img, label, w16, skel = _case(code, (70, 66, 100))
    starts = [(3, 1, 36), (6, 2, 0)]
    got = three_fills(lambda: A.crop_batch(dev(img), starts, 64, dev(label), dev(w16), dev(skel), [code, 15 - code], u=0.37), "pipeline")
    want = po.crop_batch(img, starts, [code, 15 - code], 64, label, w16, skel, 0.37)
    for k in ("data", "label", "skel"):
        np.testing.assert_array_equal(host(got[k]), want[k], err_msg=k)
    gw, ww = host(got["weight"]), want["weight"]              # float16 power: one half ulp step, as test_pipeline_gpu.py allows
    assert np.array_equal(gw, ww) or np.abs(gw - ww).max() <= np.spacing(np.float16(ww.max())).astype(np.float32)


@pytest.mark.parametrize("dtype,f64", [(np.int16, True), (np.int16, False), (np.float32, False), (np.float32, True)])
def test_two_channel_volume(A, dtype, f64):
    import pipeline_oracle as po
    hu = np.random.default_rng(11).integers(-1500, 1700, (37, 41, 53)).astype(dtype)
    got = three_fills(lambda: A.two_channel_volume(dev(hu), f64_math=f64), "pipeline")
    c0, c1 = po.two_channel(hu) if f64 else po.process_imgmsk(hu)
    np.testing.assert_array_equal(host(got), np.stack([c0, c1])[None].astype(np.float32))


# ---- window loop ----------------------------------------------------------------------------------------------------------------
def test_sliding_window_predict(A):
    import seunet_oracle as orc
    from test_net_gpu import FP32_ATOL
    x = orc.synthetic_batch(1, (48, 32, 64), 2, seed=10)["image"]
    sd = orc.deterministic_state_dict(2, 1, 1, seed=0)

    def op():
        m = A.SE_UNet(in_channel=2, n_classes=1, width_mult=1, act_dtype="fp32")
        m.load_state_dict(sd)
        m = m.cuda().eval()
        for p in m.parameters():
            p.data = guard(p.data)
        return A.sliding_window_predict(m, dev(x), cube=32, step=16, batch=2)
    got = three_fills(op, "window loop")
    ref = orc.sliding_window_predict(orc.build_oracle(2, 1, 1, seed=0), x, cube=32, step=16)
    assert got.shape == ref.shape == (48, 32, 64)
    assert float(np.abs(got - ref).max()) < FP32_ATOL


# ---- AdamW ----------------------------------------------------------------------------------------------------------------------
def test_adamw_four_steps(A):
    import adamw_oracle as ao
    g = torch.Generator().manual_seed(7)
    shapes = [(5,), (1,), (257, 9), (1024,), (1025,), (2049,)]       # one element below, at and above the 1024-element block
    init = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    grads = [[torch.randn(s, generator=g) * 1e-3 for s in shapes] for _ in range(4)]

    def op():
        params = [torch.nn.Parameter(dev(t)) for t in init]
        opt = A.AdamW(params, lr=1e-4)
        for t in range(4):
            for p, gr in zip(params, grads[t]):
                p.grad = dev(gr)
            opt.step()
            check()                                                  # (each step's gradients, before the next replaces them)
        return [p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params]
    params, _, exp_avg_sq = three_fills(op, "AdamW")
    want = ao.run([t.numpy() for t in init], [[gr.numpy() for gr in gs] for gs in grads], [1e-4] * 4)
    for i, p in enumerate(params):
        np.testing.assert_allclose(host(p), want["params"][i], rtol=2e-7, atol=1e-9)
        np.testing.assert_allclose(host(exp_avg_sq[i]), want["exp_avg_sq"][i], rtol=2e-6, atol=3e-7 * float(np.abs(want["exp_avg_sq"][i]).max()))


def test_adamw_four_steps_gated_with_a_skip_at_step_two(A):
    """The gated step (``overflow_gate=``) over dirty scratch: the step-size table is ``torch.empty`` scratch that the prepare
    kernel writes before the main kernel reads it, the skipped-step counts are ``torch.zeros``; neither may depend on the fill,
    and nothing is written beside them, the flag or the moments.  Against the oracle run on steps one, three and four."""
    import adamw_oracle as ao
    g = torch.Generator().manual_seed(7)
    shapes = [(5,), (1,), (257, 9), (1024,), (1025,), (2049,)]       # one element below, at and above the 1024-element block
    init = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    grads = [[torch.randn(s, generator=g) * 1e-3 for s in shapes] for _ in range(4)]

    def op():
        params = [torch.nn.Parameter(dev(t)) for t in init]
        flag = dev(torch.zeros((), dtype=torch.int32))
        opt = A.AdamW(params, lr=1e-4, overflow_gate=flag)
        for t in range(4):
            for p, gr in zip(params, grads[t]):
                p.grad = dev(gr)
            if t == 1:
                flag.bitwise_or_(torch.ones_like(flag))              # (the way an overflowing backward raises it)
            opt.step()
            check()
        return ([p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params],
                [opt.state[p]["skipped"] for p in params], flag)
    params, exp_avg, exp_avg_sq, skipped, flag = three_fills(op, "AdamW gated")
    assert int(flag) == 0 and [float(v) for v in skipped] == [1.0] * len(shapes)
    want = ao.run([t.numpy() for t in init], [[gr.numpy() for gr in grads[t]] for t in (0, 2, 3)], [1e-4] * 3)
    for i, p in enumerate(params):
        np.testing.assert_allclose(host(p), want["params"][i], rtol=2e-7, atol=1e-9)
        for got, key in ((exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            np.testing.assert_allclose(host(got[i]), want[key][i], rtol=2e-6, atol=3e-7 * float(np.abs(want[key][i]).max()))


# ---- losses ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", (1, 2, 3))
def test_fused_stage_loss(A, stage):
    """Forward and backward at (2, 1, 6, 9, 40) against tests/loss_ref.py under the bounds tests/test_loss_layers_gpu.py derives
    (check_head: sums and gradient of each head; check_value: the value)."""
    import test_loss_layers_gpu as TL
    shape = (2, 1, 6, 9, 40)
    xe, t, w, s = TL.shaped(shape, shape, seed=41)
    xd = xe * 0.5 + 0.1
    xd.reshape(-1)[::4099] = -100.0

    def op():
        e, d = guard(xe).requires_grad_(), guard(xd).requires_grad_()
        loss = A.fused_stage_loss(stage, e, d, guard(t), guard(w), guard(s))
        loss.backward()
        return loss.detach(), e.grad, d.grad
    loss, ge, gd = three_fills(op, "losses")
    cd, ce = TL.STAGE_COEF[stage]
    sk = None if stage == 2 else s
    heads = [TL.check_head(gd, xd, t, w, sk, cd, True, what=f"stage {stage} decoder head") + (cd,),
             TL.check_head(ge, xe, t, w, sk, ce, True, what=f"stage {stage} encoder head") + (ce,)]
    TL.check_value(loss, heads, f"stage {stage}")


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
    print("\nguarded allocations verified, by family (operations, allocations):")
    for fam, (ops_n, allocs) in sorted(G.VERIFIED.items()):
        print(f"  {fam}: {ops_n} operations, {allocs} allocations")
