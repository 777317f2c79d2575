"""An optimizer step behind an fp16 backward pass that overflowed changes nothing.

fp16 storage carries the activation gradients times a static loss scale; a backward pass whose scaled gradients overflow
leaves zero gradients, counts itself in ``model.overflow_steps`` and raises ``model.overflow_pending``.  Zero gradients do
not drop a step: AdamW still decays the weights, multiplies ``exp_avg`` by beta1 and ``exp_avg_sq`` by beta2, advances its
bias corrections and moves the weights along the stale momentum (0.67 lr per element after one real step).  The gated
``seunet_amd.AdamW`` (``overflow_gate=``; ``seunet_adamw_step_gated``) reads the flag on the device and must leave parameters
and both moments bit for bit, with the bias corrections of later steps counting applied steps only.

* op level: the 117 registry tensors, 6 steps, five overflow patterns, against oracle/adamw_oracle.py run on the list with
  the overflowed steps removed, under the tolerances of tests/test_optim_gpu.py (tests/overflow_step_cases.py: the host file
  shows that a zero-gradient step in place of the skipped one fails this comparison on most tensors); the ragged list with
  weight decay, maximize, other betas and a tensor that joins late against ``torch.optim.AdamW`` stepped on the applied
  steps only; a checkpoint round trip;
* nothing synchronises the host (``torch.cuda.set_sync_debug_mode("error")``);
* network: a trajectory with one overflowing step equals, bitwise, the trajectory without that step, with and without
  gradient accumulation;
* data parallel: one rank's overflow skips the step on both ranks, with the overlapped exchange (``GradSync``) and with the
  serial one (``allreduce_gradients(..., gate=model)``), and the ranks end on the bits of the two clean steps alone.
"""
import io
import os

import numpy as np
import pytest
import torch

import overflow_step_cases as OC

pytestmark = pytest.mark.gpu


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


def new_flag():
    return torch.zeros((), dtype=torch.int32, device="cuda")


def raise_flag(flag):
    """The way a backward pass does it: a device operation, sticky."""
    flag.bitwise_or_(torch.ones((), dtype=torch.int32, device=flag.device))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def snapshot(opt, params):
    """Clones of (parameter, exp_avg, exp_avg_sq) per tensor; moments that do not exist yet count as zeros."""
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append((p.detach().clone(), st["exp_avg"].clone() if "exp_avg" in st else torch.zeros_like(p),
                    st["exp_avg_sq"].clone() if "exp_avg_sq" in st else torch.zeros_like(p)))
    return out


def changed(a, b):
    """Indices of the tensors of two snapshots whose parameter or moments differ in any bit."""
    return [i for i, (u, v) in enumerate(zip(a, b)) if not all(torch.equal(bits(x), bits(y)) for x, y in zip(u, v))]


# ---- op level, against the oracle -----------------------------------------------------------------------------------------------
def registry_run(A, pattern, gated=True):
    """6 steps on the 117 registry tensors; the flag is raised before the steps of the pattern.  Returns the final state as
    ``adamw_oracle.run`` does and, per skipped step, the tensors that did not keep their bits across it."""
    init, grads = OC.registry_inputs()
    skip = OC.PATTERNS[pattern]
    params = [torch.nn.Parameter(torch.from_numpy(t).cuda()) for t in init]
    flag = new_flag()
    opt = A.AdamW(params, lr=OC.LR, overflow_gate=flag) if gated else A.AdamW(params, lr=OC.LR)
    moved = {}
    for k in range(OC.STEPS):
        for p, g in zip(params, grads[k]):
            p.grad = torch.zeros_like(p) if (k in skip and not gated) else torch.from_numpy(g).cuda()
        if k in skip:
            raise_flag(flag)
            before = snapshot(opt, params)
        opt.step()
        if k in skip:
            moved[k] = changed(before, snapshot(opt, params))
        if gated:
            assert int(flag) == 0, "step() consumes the flag"
    host = lambda ts: [t.detach().cpu().numpy() for t in ts]
    got = {"params": host(params), "exp_avg": host([opt.state[p]["exp_avg"] for p in params]),
           "exp_avg_sq": host([opt.state[p]["exp_avg_sq"] for p in params])}
    return got, moved, opt, params


@pytest.mark.parametrize("pattern", list(OC.PATTERNS))
def test_registry_tensors_against_the_oracle_with_the_overflowed_steps_removed(A, pattern):
    got, moved, opt, params = registry_run(A, pattern)
    skip = OC.PATTERNS[pattern]
    assert len(params) == 117 and sorted(moved) == sorted(skip)
    for k, idx in moved.items():
        assert not idx, f"skipped step {k + 1}: {len(idx)} of 117 tensors changed, first {idx[:5]}"
    bad = OC.failing_tensors(got, OC.registry_reference(pattern))
    assert not bad, f"{len(bad)} of 117 tensors miss the oracle, first {bad[:5]}"
    for p in params:
        assert int(opt.state[p]["step"].item()) == OC.STEPS and float(opt.state[p]["skipped"]) == len(skip)


def test_control_the_ungated_step_on_zero_gradients_fails_the_same_checks(A):
    """What an overflowing backward leaves is zero gradients; without the gate that step moves all 117 tensors and the result
    misses the oracle with the step removed on all of them (the host file shows the same with the oracle alone)."""
    got, moved, _, _ = registry_run(A, "middle", gated=False)
    assert len(moved[2]) == 117
    assert len(OC.failing_tensors(got, OC.registry_reference("middle"))) == 117


RAGGED_KW = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, maximize=True)


@pytest.mark.parametrize("pattern", list(OC.PATTERNS))
def test_ragged_list_against_torch_adamw_stepped_on_the_applied_steps_only(A, pattern):
    """weight_decay / maximize / other betas; tensor 1 has no gradient in the first two steps and keeps its own count.  Then
    the optimizer's state goes through a checkpoint into a fresh optimizer on copies of the parameters, and one more step of
    both gives the same bits."""
    skip = OC.PATTERNS[pattern]
    g = torch.Generator().manual_seed(3)
    a = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in OC.RAGGED_SHAPES]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    flag = new_flag()
    oa, ob = A.AdamW(a, overflow_gate=flag, **RAGGED_KW), torch.optim.AdamW(b, foreach=False, **RAGGED_KW)
    for t in range(OC.STEPS):
        for i, (p, q) in enumerate(zip(a, b)):
            if i == 1 and t < 2:
                p.grad = q.grad = None
                continue
            gr = torch.randn(p.shape, generator=g).cuda()
            p.grad, q.grad = gr.clone(), gr.clone()
        if t in skip:
            raise_flag(flag)
            before = snapshot(oa, a)
            oa.step()
            assert not changed(before, snapshot(oa, a)), (pattern, t)
        else:
            oa.step(); ob.step()
    for i, (p, q) in enumerate(zip(a, b)):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=2e-6, atol=1e-7)
        for k in ("exp_avg", "exp_avg_sq"):
            torch.testing.assert_close(oa.state[p][k], ob.state[q][k], rtol=2e-6, atol=1e-7)
        applied = OC.STEPS - (2 if i == 1 else 0) - sum(1 for t in skip if not (i == 1 and t < 2))
        assert int(oa.state[p]["step"].item()) - float(oa.state[p]["skipped"]) == applied == int(ob.state[q]["step"].item())
    # checkpoint -> fresh optimizer -> one more step == continuing
    buf = io.BytesIO()
    torch.save(oa.state_dict(), buf)
    buf.seek(0)
    a2 = [torch.nn.Parameter(p.detach().clone()) for p in a]
    flag2 = new_flag()
    fresh = A.AdamW(a2, overflow_gate=flag2, **RAGGED_KW)
    fresh.load_state_dict(torch.load(buf))
    for p, q in zip(a, a2):
        gr = torch.randn(p.shape, generator=g).cuda()
        p.grad, q.grad = gr.clone(), gr.clone()
    oa.step(); fresh.step()
    assert not changed(snapshot(oa, a), snapshot(fresh, a2))
    for p, q in zip(a, a2):
        assert torch.equal(oa.state[p]["skipped"], fresh.state[q]["skipped"]) and oa.state[p]["step"] == fresh.state[q]["step"]


# ---- network ---------------------------------------------------------------------------------------------------------------------
PLANT = (1, 0, 17, 5, 30)       # the voxel test_network_one_inf_voxel_in_the_head_gradient_drops_the_step plants its +inf in


def make_net(A, orc, gated=True):
    m = A.SE_UNet(2, 1, act_dtype="fp16")
    m.load_state_dict(orc.deterministic_state_dict(2, 1, 1, seed=0))
    m = m.cuda().eval()         # (no DropLayer draws: two runs see the same network)
    opt = A.AdamW(m.parameters(), lr=1e-3, overflow_gate=m) if gated else A.AdamW(m.parameters(), lr=1e-3)
    return m, opt


@pytest.fixture(scope="module")
def batches():
    """name -> (input, incoming encoder-head gradient, incoming decoder-head gradient) at 2 x 2 x 32^3, made once."""
    g = torch.Generator().manual_seed(2024)
    out = {}
    for name in ("b1", "b2", "b3", "b4", "bX", "bY"):
        out[name] = (torch.randn((2, 2, 32, 32, 32), generator=g).cuda(), (torch.randn((2, 1, 32, 32, 32), generator=g) * 1e-4).cuda(),
                     (torch.randn((2, 1, 32, 32, 32), generator=g) * 1e-4).cuda())
    return out


def net_backward(m, batch, plant):
    x, g0, g1 = batch
    e, d = m(x)
    gd = g1.clone()
    if plant:
        gd[PLANT] = float("inf")
    torch.autograd.backward([e, d], [g0, gd])


def trajectory(A, orc, batches, plan, gated=True):
    """``plan``: a list of optimizer steps, each a list of (batch name, plant) backward passes.  Returns the final snapshot,
    the overflow count, and per step that held a plant the tensors that changed across it."""
    m, opt = make_net(A, orc, gated)
    params = list(m.parameters())
    moved = {}
    for k, step in enumerate(plan):
        opt.zero_grad(set_to_none=True)
        for name, plant in step:
            net_backward(m, batches[name], plant)
        planted = any(plant for _, plant in step)
        if planted:
            before = snapshot(opt, params)
        opt.step()
        if planted:
            moved[k] = changed(before, snapshot(opt, params))
    return snapshot(opt, params), int(m.overflow_steps), moved, int(m.overflow_pending)


CLEAN = [[("b1", False)], [("b2", False)], [("b3", False)], [("b4", False)]]
PLANS = {"one-backward": CLEAN[:2] + [[("bX", True)]] + CLEAN[2:],
         "accumulation": CLEAN[:2] + [[("bX", True), ("bY", False)]] + CLEAN[2:]}


@pytest.fixture(scope="module")
def clean_trajectory(A, orc, batches):
    return trajectory(A, orc, batches, CLEAN)


@pytest.mark.parametrize("plan", list(PLANS))
def test_network_trajectory_with_an_overflowing_step_equals_the_one_without_it(A, orc, batches, clean_trajectory, plan):
    """b1, b2, [overflow], b3, b4 against b1, b2, b3, b4: every parameter and both moments bitwise, and nothing moves
    across the overflowing step.  With accumulation the FIRST of two backward passes overflows (the flag is sticky)."""
    want, n_clean, _, _ = clean_trajectory
    got, n, moved, pending = trajectory(A, orc, batches, PLANS[plan])
    assert (n, n_clean, pending) == (1, 0, 0)
    assert list(moved) == [2] and not moved[2], f"{len(moved[2])} tensors changed across the overflowing step, first {moved[2][:5]}"
    differ = changed(got, want)
    assert len(got) == 117 and not differ, f"{len(differ)} of 117 tensors differ from the clean trajectory, first {differ[:5]}"
    # the run trained: every tensor has moved its moments but the dead dc62 block's weight (no gradient) and the 18 gated blocks'
    # conv1.bias, whose gradient in front of an InstanceNorm is exactly zero
    live = [i for i, (p, m_, v) in enumerate(got) if bool(m_.any())]
    assert len(live) == 117 - 1 - 18, len(live)


def test_control_the_ungated_network_trajectory_differs_in_every_live_tensor(A, orc, batches):
    """The same plan with the optimizer as it is without ``overflow_gate``: the step on the zero gradients moves every tensor
    that has a gradient (all but the dead dc62 block's weight), and none of them ends on the clean trajectory's bits."""
    want, _, _, _ = trajectory(A, orc, batches, CLEAN, gated=False)
    got, n, moved, pending = trajectory(A, orc, batches, PLANS["one-backward"], gated=False)
    assert (n, pending) == (1, 1) and len(moved[2]) == 116
    assert sum(1 for a, b in zip(got, want) if not torch.equal(bits(a[0]), bits(b[0]))) == 116


def test_forward_loss_backward_and_gated_step_do_not_synchronise(A, orc):
    """torch.cuda.set_sync_debug_mode("error") makes every synchronising torch call raise; the mode is checked to bite first.
    One overflowing step (a +inf voxel planted into the decoder head's incoming gradient by a hook) and one clean step."""
    m, opt = make_net(A, orc)
    b = orc.synthetic_batch(2, (32, 32, 32), 2, seed=3)
    x, lab = b["image"].cuda(), b["label"].cuda()
    params = list(m.parameters())

    voxel = torch.zeros((2, 1, 32, 32, 32), dtype=torch.bool, device="cuda")
    voxel[PLANT] = True

    def plant(g):                               # (an indexed assignment of a Python scalar would synchronise by itself)
        return g.masked_fill(voxel, float("inf"))

    def step(overflow):
        opt.zero_grad(set_to_none=True)
        e, d = m(x)
        loss = A.fused_stage_loss(1, e, d, lab)
        if overflow:
            d.register_hook(plant)
        loss.backward()
        opt.step()

    step(False)                                 # (library loaded, registry checked, optimizer state made before the mode is set)
    torch.cuda.synchronize()
    s0 = snapshot(opt, params)
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            x.sum().item()
        step(True)
        s1 = snapshot(opt, params)
        step(False)
        s2 = snapshot(opt, params)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert int(m.overflow_steps) == 1 and int(m.overflow_pending) == 0
    assert not changed(s0, s1)
    assert len(changed(s1, s2)) >= 117 - 1 - 18      # (all but dc62's weight and, weight decay aside, the 18 conv1.bias tensors)


# ---- data parallel ----------------------------------------------------------------------------------------------------------------
def _dp_overflow_worker(rank, world, port, overlap, q):
    import sys as _sys
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p_ in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        if p_ not in _sys.path:
            _sys.path.insert(0, p_)
    import torch.distributed as dist
    import seunet_amd as A
    import seunet_oracle as orc
    from seunet_amd import ddp
    try:
        ddp.init_from_env("gloo")
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        data = [orc.synthetic_batch(2, (32, 32, 32), 2, seed=s) for s in (3, 4, 5)]

        def plant(g):
            g = g.clone()
            g[0, 0, 17, 5, 30] = float("inf")
            return g

        def run(steps, overflow_at):
            m, opt = make_net(A, orc)
            if overlap:
                m.grad_sync = ddp.GradSync()
            params = list(m.parameters())
            moved = None
            for k in steps:
                x, lab = data[k]["image"][rank:rank + 1].to(dev), data[k]["label"][rank:rank + 1].to(dev)
                opt.zero_grad(set_to_none=True)
                e, d = m(x)
                loss = A.fused_stage_loss(1, e, d, lab, group=True)
                if k == overflow_at and rank == 1:
                    d.register_hook(plant)
                loss.backward()
                if not overlap:
                    ddp.allreduce_gradients(m.parameters(), gate=m)
                if k == overflow_at:
                    before = snapshot(opt, params)
                    gmax = max(float(p.grad.abs().max()) for p in params if p.grad is not None)
                opt.step()
                if k == overflow_at:
                    moved = (len(changed(before, snapshot(opt, params))), gmax)
            flat = torch.cat([t.reshape(-1) for s in snapshot(opt, params) for t in s]).cpu().numpy()
            return flat, int(m.overflow_steps), moved

        with_overflow = run((0, 1, 2), 1)
        clean = run((0, 2), None)
        q.put((rank, None, with_overflow, clean))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:     # report instead of hanging the parent
        import traceback
        q.put((rank, traceback.format_exc() or repr(ex), None, None))


def spawn_dp_overflow(overlap):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000 + 307 + (24 if overlap else 0)
    procs = [ctx.Process(target=_dp_overflow_worker, args=(r, 2, port, overlap, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
    assert all(r[1] is None for r in res), [r[1] for r in res]
    return res


@pytest.mark.parametrize("exchange", ["GradSync", "allreduce_gradients"])
def test_data_parallel_overflow_on_one_rank_skips_the_step_on_both(A, exchange):
    """Two gloo ranks share the GPU, 1 x 2 x 32^3 each, fp16, three steps; rank 1's backward overflows at the second.  Both ranks
    skip it (nothing moves, gradients are zero, ``overflow_steps == 1``), end on the same bits, and those are the bits of the
    same two-rank run of steps one and three alone."""
    res = spawn_dp_overflow(exchange == "GradSync")
    for rank, _, (flat, n, moved), (flat_clean, n_clean, _) in res:
        assert (n, n_clean) == (1, 0), (rank, n, n_clean)
        assert moved == (0, 0.0), f"rank {rank}: {moved[0]} tensors changed across the overflowing step, largest gradient {moved[1]}"
        assert np.array_equal(flat.view(np.int32), flat_clean.view(np.int32)), \
            f"rank {rank}: {int((flat.view(np.int32) != flat_clean.view(np.int32)).sum())} of {flat.size} elements differ from the clean run"
    assert np.array_equal(res[0][2][0].view(np.int32), res[1][2][0].view(np.int32)), "the ranks' weights or moments differ"
