"""The backward epilogue, pooling, up-sampling and head passes on SUBNORMAL fp16 gradients, at the top of fp16's range (overflow
on store) and on a gradient with one +inf / NaN element (method of both in tests/range_epilogue_cases.py), and one
whole-network backward with a single +inf voxel in its head gradient (the convolutions' side of the same question: tests/test_conv_range_gpu.py).

fp16 training carries every activation gradient times a static loss scale of 65536; unscaled voxel gradients of 1e-9 and below
arrive in these passes as fp16 subnormals.  Every incoming gradient here -- g_e, the f32 level gradient, g_out, g_pool, the
previous gradient of a ``+=``, g_pred -- is first rounded to multiples of 2^-4 and then multiplied by 2^-20: exact multiples of
the fp16 quantum 2^-24 below 2^-14 (``epilogue_layer_cases.scale_grad`` asserts it).  The float64 references and the derived
bounds are the ones of tests/test_epilogue_layers_gpu.py, unchanged: ``element_bound`` floors the storage spacing at 2^-24 and
``sum_bound`` is linear in the magnitudes, so the bound of a stored element is about half a quantum and a pass that flushed
operands or results would miss it by orders of magnitude.  What is bitwise there is bitwise here (max-pool backward, the fused
against the split finaliser).  The largest err / bound ratio of each pass is printed.

The range does not depend on the extent: the cases are those of 2 x 2 x 32^3 at width 1 (the extent the network tests run), and
for ``upsample2_bwd`` one shape per kernel form from ``test_launch_cut_host.UP2_FORMS``."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_layer_cases as E  # noqa: E402
import range_epilogue_cases as RC  # noqa: E402
from test_launch_cut_host import UP2_FORMS  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = E.Config(2, 32, 1)
SUB = 2.0 ** -20
assert len(CFG.GATED) == 18 and len(CFG.AGG_X) == 3 and len(CFG.AGG_1) == 3 and len(CFG.POOLS) == 3 and len(CFG.UPS) == 3
fp16 = lambda cases: [c for c in cases if "fp16" in c]
# upsample2_bwd in 16-bit storage: one shape per kernel form (column 2 of the table), both shapes of the gather form
UP_FORM_SHAPES = [("march", (1, 32, 5, 7, 70)), ("tiled", (1, 16, 2, 9, 64)), ("gather", (1, 136, 2, 3, 3)), ("gather", (1, 8, 2, 3, 1))]
assert all(UP2_FORMS[s][2] == f for f, s in UP_FORM_SHAPES) and {f for f, _ in UP_FORM_SHAPES} == {r[2] for r in UP2_FORMS.values()}
UP_FORM_CASES = [(f"form-{f}", s[1], (s[0],) + s[2:], "fp16", acc) for f, s in UP_FORM_SHAPES for acc in (0, 1)]


@pytest.fixture(scope="module")
def S():
    return E.ops_or_skip()


@pytest.mark.parametrize("case", fp16(CFG.GATE_CASES), ids=E.ids)
def test_gate_backward_subnormal_gradients(S, case):
    E.gate_backward(S, CFG, case, grad_scale=SUB)


@pytest.mark.parametrize("case", fp16(CFG.X_CASES), ids=E.ids)
def test_aggregation_x_pool_backward_subnormal_gradients(S, case):
    E.aggregation_x_pool_forward_and_backward(S, CFG, case, grad_scale=SUB)


@pytest.mark.parametrize("case", fp16(CFG.AGG1_CASES), ids=E.ids)
def test_aggregation_one_branch_subnormal_gradients(S, case):
    E.aggregation_one_branch(S, CFG, case, grad_scale=SUB)


@pytest.mark.parametrize("case", fp16(CFG.POOL_BWD_CASES), ids=E.ids)
def test_maxpool_backward_subnormal_gradients(S, case):
    E.maxpool_backward(S, case, grad_scale=SUB)


@pytest.mark.parametrize("case", fp16(CFG.UP_BWD_CASES) + UP_FORM_CASES, ids=E.ids)
def test_upsample_backward_subnormal_gradients(S, case):
    E.upsample_backward(S, case, grad_scale=SUB)


@pytest.mark.parametrize("nlevels", (4, 3))
def test_head_backward_subnormal_gradients(S, nlevels):
    E.head_backward(S, CFG, nlevels, grad_scale=SUB)


# ---- overflow on store (fp16) --------------------------------------------------------------------------------------------------
# The gradients are clamped to +-15/16 (``epilogue_layer_cases.scale_grad``) and run twice: at scale 1, from whose float64
# reference k is chosen, and at 2^k, where every stored element beyond fp16's range must be +-inf and every other one within its
# existing bound (``range_epilogue_cases.OverflowStore``, which asserts the 1 % / 25 % / 2 % shares on the reference).  m1, m2 and
# the parameter gradients are f32 and keep their bounds at 2^k.
@pytest.mark.parametrize("case", fp16(CFG.GATE_CASES), ids=E.ids)
def test_gate_backward_overflow_on_store(S, case):
    RC.overflow_case(lambda scale, chk: E.gate_backward(S, CFG, case, grad_scale=scale, store_check=chk, grad_clip=RC.GATE_CLIP), RC.GATE_K_MAX)


@pytest.mark.parametrize("case", fp16(CFG.X_CASES), ids=E.ids)
def test_aggregation_x_pool_backward_overflow_on_store(S, case):
    RC.overflow_case(lambda scale, chk: E.aggregation_x_pool_forward_and_backward(S, CFG, case, grad_scale=scale, store_check=chk))


@pytest.mark.parametrize("case", fp16(CFG.AGG1_CASES), ids=E.ids)
def test_aggregation_one_branch_overflow_on_store(S, case):
    RC.overflow_case(lambda scale, chk: E.aggregation_one_branch(S, CFG, case, grad_scale=scale, store_check=chk))


@pytest.mark.parametrize("case", fp16(CFG.UP_BWD_CASES) + UP_FORM_CASES, ids=E.ids)
def test_upsample_backward_overflow_on_store(S, case):
    RC.overflow_case(lambda scale, chk: E.upsample_backward(S, case, grad_scale=scale, store_check=chk))


@pytest.mark.parametrize("case", [c for c in fp16(CFG.POOL_BWD_CASES) if c[4] == 1], ids=E.ids)
def test_maxpool_backward_overflow_on_store(S, case):
    """``+=`` only: without it the pass copies a finite fp16 number.  Bitwise as ever (the expectation rounds g + prev once, to
    inf from 65520 on); g and prev are clamped to 15/16 and scaled by 2^16, so that sums of 17/16 and above overflow."""
    shares = []
    E.maxpool_backward(S, case, grad_scale=2.0 ** RC.K_MAX, shares=shares)
    print(f"  maxpool_bwd {case}: k = {RC.K_MAX}: overflow per sample {[round(s, 4) for s in shares]}")
    assert shares and all(0.01 <= s <= 0.75 for s in shares), shares


# ---- one whole-network case ---------------------------------------------------------------------------------------------------
def test_network_one_inf_voxel_in_the_head_gradient_drops_the_step(S):
    """fp16 mode, 2 x 2 x 32^3.  A backward whose incoming head gradient has a single +inf voxel in sample 1 raises
    ``overflow_steps`` by one and leaves all-zero parameter gradients; the same call without the plant leaves the counter where
    it is, and its gradients equal those of a run made before it, bitwise."""
    from seunet_amd.SE_UNet import SE_UNet
    E._cache.clear()
    torch.cuda.empty_cache()
    with torch.random.fork_rng(devices=[]):
        torch.default_generator.manual_seed(1234)
        net = SE_UNet(2, 1, act_dtype="fp16", negative_slope=E.SLOPE)
    net = net.cuda().eval()
    assert net.loss_scale == 65536.0
    g = E.gen(E.seed_of("net", "range"))
    x = torch.randn((2, 2, 32, 32, 32), generator=g, device="cuda")
    g0 = torch.randn((2, 1, 32, 32, 32), generator=g, device="cuda") * 1e-4
    g1 = torch.randn((2, 1, 32, 32, 32), generator=g, device="cuda") * 1e-4

    def step(plant):
        for p in net.parameters():
            p.grad = None
        e, d = net(x)
        gd = g1.clone()
        if plant:
            gd[1, 0, 17, 5, 30] = float("inf")
        torch.autograd.backward([e, d], [g0, gd])
        return int(net.overflow_steps), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

    c0, before = step(False)
    assert c0 == 0 and before and all(bool(v.isfinite().all()) for v in before.values()) and any(bool(v.any()) for v in before.values())
    c1, dropped = step(True)
    assert c1 == c0 + 1, (c0, c1)
    assert set(dropped) == set(before) and all(not bool(v.any()) for v in dropped.values()), [n for n, v in dropped.items() if bool(v.any())]
    c2, after = step(False)
    assert c2 == c1, (c1, c2)
    differ = [n for n in before if not torch.equal(before[n].view(torch.int32), after[n].view(torch.int32))]
    assert not differ, differ


# ---- a non-finite incoming gradient (bf16, fp16, and fp32 where the case lists have it) ----------------------------------------
# Method and requirements: tests/range_epilogue_cases.py.


@pytest.mark.parametrize("case", CFG.GATE_CASES, ids=E.ids)
def test_gate_backward_nonfinite_gradient(S, case):
    RC.gate_backward_nonfinite(S, CFG, case)


@pytest.mark.parametrize("case", [c for c in CFG.X_CASES if c[2] == "random"], ids=E.ids)
def test_aggregation_x_pool_backward_nonfinite_gradient(S, case):
    RC.aggregation_x_pool_backward_nonfinite(S, CFG, case)


@pytest.mark.parametrize("case", CFG.AGG1_CASES, ids=E.ids)
def test_aggregation_one_branch_nonfinite_gradient(S, case):
    RC.aggregation_one_branch_nonfinite(S, CFG, case)


@pytest.mark.parametrize("case", CFG.POOL_BWD_CASES, ids=E.ids)
def test_maxpool_backward_nonfinite_gradient(S, case):
    RC.maxpool_backward_nonfinite(S, case)


@pytest.mark.parametrize("case", CFG.UP_BWD_CASES + [c[:3] + (dt, c[4]) for c in UP_FORM_CASES for dt in ("bf16", "fp16")], ids=E.ids)
def test_upsample_backward_nonfinite_gradient(S, case):
    RC.upsample_backward_nonfinite(S, case)


@pytest.mark.parametrize("nlevels", (4, 3))
def test_head_backward_nonfinite_gradient(S, nlevels):
    RC.head_backward_nonfinite(S, CFG, nlevels)
