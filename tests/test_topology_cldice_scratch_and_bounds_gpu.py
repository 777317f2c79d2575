"""soft_skeleton, soft_cldice_loss (forward and backward) and cldice_score over dirty scratch memory, with red zones around every
buffer (tests/guarded_alloc.py): three runs -- the outputs, the workspace and the saved state pre-filled with 0x00, 0xFF and
seeded random bytes, the inputs copied into red-zoned buffers -- must leave every red zone as it was, give the same bits, and
equal the oracle (tests/cldice_oracle.py), never another run of the code under test.  (2, 7, 9, 11) has rows that are no
multiple of 4 (the scalar path) and volumes smaller than a tile on every axis, (3, 5, 33, 70) rows that cross a tile end and
16-byte accesses; in both a halo read past a buffer, or into the next volume of the batch, changes the result."""
import numpy as np
import pytest
import torch

from guarded_alloc import guard, three_fills

import cldice_oracle as O
from test_topology_cldice_gpu import check_gradient, same_f32_bits

pytestmark = pytest.mark.gpu

_ORIG = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
SHAPES = O.PARITY_SHAPES[:2]
ITERS = 3


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def dev(a):
    return guard(a.cuda() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda())


@pytest.mark.parametrize("shape", SHAPES)
def test_soft_skeleton(A, shape):
    p, t = O.case(shape)
    same_f32_bits(three_fills(lambda: A.soft_skeleton(dev(p), ITERS), "soft_skeleton"), O.soft_skeleton_a(p, ITERS))
    same_f32_bits(three_fills(lambda: A.soft_skeleton(dev(t), ITERS), "soft_skeleton"), O.soft_skeleton_b(t, ITERS))


@pytest.mark.parametrize("shape", SHAPES)
def test_loss_forward_and_backward(A, shape):
    p, t = O.case(shape)
    ref = O.reference(shape, ITERS)

    def op():
        x = dev(p).requires_grad_(True)
        loss = A.soft_cldice_loss(x, dev(t), ITERS)
        loss.backward()
        return loss.detach(), x.grad
    loss, g = three_fills(op, "soft_cldice_loss")
    assert abs(float(loss) - float(ref["l64"])) <= max(2.0 ** -22, 4 * abs(float(ref["l32"]) - float(ref["l64"])))
    check_gradient(g.cpu(), ref["g64"], ref["g32"], f"{shape} under the guard")


@pytest.mark.parametrize("shape", SHAPES)
def test_cldice_score(A, shape):
    import skeleton_oracle as SO
    p, t = O.case(shape)
    vp, vl = (p[0] > 0.6).numpy().astype(np.uint8), t[0].numpy().astype(np.uint8)
    sp, sl = SO.skeletonize(vp)[0], SO.skeletonize(vl)[0]
    want = O.cldice_score(vp, vl, sp, sl) + (O.cldice_counts(vp, vl, sp, sl),)
    assert three_fills(lambda: A.cldice_score(dev(vp), dev(vl), dev(sp), dev(sl), return_parts=True), "cldice_score") == want
    assert three_fills(lambda: A.cldice_score(dev(vp), dev(vl), return_parts=True), "cldice_score, thinning inside") == want


def test_the_allocation_functions_are_restored(A):
    assert all(getattr(torch, n) is f for n, f in _ORIG.items())
