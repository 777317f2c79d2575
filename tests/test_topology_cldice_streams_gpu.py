"""soft_skeleton, soft_cldice_loss (forward and backward) and cldice_score on a side stream, behind a producer that is still busy
when the operation is called (tests/side_stream.py), as tests/test_streams_edt_sampling_gpu.py runs the EDT: the inputs hold
poison -- the same volumes turned round -- until a delayed copy on a fresh non-blocking stream delivers the real data, and the
operation is called under that stream while the delay is pending.  A launch or memset on stream 0 would see the poison.  Results
must equal the same call made beforehand on the default stream bit for bit, and the oracle (tests/cldice_oracle.py).

The clDice GPU test files are named so that they run AFTER tests/test_streams_gpu.py.  That file's first test is a positive control
in which work on the default stream must overtake a delayed side stream.  Whether it can depends on which hardware queue the
control's pool stream shares: with 4 hardware queues, a pool stream that lands on the default stream's queue runs the default-stream
work behind the delay, and the control sees the real data (measured in a fresh process with 0 .. 12 pool streams used first: 6 and
10 fail, the others pass).  Run after it, these files leave the process as it was when the control draws its stream."""
import numpy as np
import pytest
import torch

from guarded_alloc import same_bits
from side_stream import run_behind_delay, to_device

import cldice_oracle as O
from test_topology_cldice_gpu import check_gradient, same_f32_bits

pytestmark = pytest.mark.gpu

SHAPE = (3, 5, 33, 70)
ITERS = 3


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def both(real, poison, op, label, no_host_sync):
    """The side-stream result of ``op`` after asserting that it has the bits of the default-stream result (also the warm-up)."""
    want = op(*[to_device(v) for v in real])
    torch.cuda.synchronize()
    got = run_behind_delay(lambda: real, lambda: poison, op, no_host_sync=no_host_sync, label=label)
    same_bits(got, want, f"{label}: side stream against default stream")
    return got


def turned(a):
    """Poison for a volume: the same volume turned round along its last three axes (still a valid input of that shape)."""
    return torch.flip(a, (-3, -2, -1)).contiguous() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a[..., ::-1, ::-1, ::-1])


def test_soft_skeleton(A):
    p, _ = O.case(SHAPE)
    got = both([p], [turned(p)], lambda x: A.soft_skeleton(x, ITERS), "soft_skeleton", True)
    same_f32_bits(got, O.soft_skeleton_a(p, ITERS))


def test_loss_forward_and_backward(A):
    p, t = O.case(SHAPE)
    ref = O.reference(SHAPE, ITERS)

    def op(pb, tb):
        x = pb.detach().requires_grad_(True)
        loss = A.soft_cldice_loss(x, tb, ITERS)
        loss.backward()
        return loss.detach(), x.grad
    loss, g = both([p, t], [turned(p), turned(t)], op, "soft_cldice_loss", True)
    assert abs(float(loss) - float(ref["l64"])) <= max(2.0 ** -22, 4 * abs(float(ref["l32"]) - float(ref["l64"])))
    check_gradient(g.cpu(), ref["g64"], ref["g32"], "side stream")


def test_cldice_score(A):
    import skeleton_oracle as SO
    p, t = O.case(SHAPE)
    vp, vl = (p[0] > 0.6).numpy().astype(np.uint8), t[0].numpy().astype(np.uint8)
    sp, sl = SO.skeletonize(vp)[0], SO.skeletonize(vl)[0]
    want = O.cldice_score(vp, vl, sp, sl) + (O.cldice_counts(vp, vl, sp, sl),)
    real = [vp, vl, sp, sl]
    got = both(real, [turned(a) for a in real], lambda a, b, c, d: A.cldice_score(a, b, c, d, return_parts=True), "cldice_score", False)
    assert got == want
    got = both(real[:2], [turned(a) for a in real[:2]], lambda a, b: A.cldice_score(a, b, return_parts=True), "cldice_score, thinning inside",
               False)
    assert got == want
