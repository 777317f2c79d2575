"""The thinning definition of DESIGN.md section 3d on the CPU: tests/skeleton_oracle.py reproduces the pinned voxel counts and
digests of the eight test volumes, keeps the topology, and is idempotent; the workspace query of the C ABI answers without a
GPU.  The oracle is the yardstick tests/test_skeleton_gpu.py compares the HIP kernels with."""
import numpy as np
import pytest

import skeleton_oracle as so


@pytest.mark.parametrize("name", so.CASES)
def test_oracle_reproduces_counts_and_digests(name):
    v, sk, passes = so.solved(name)
    n_in, n_out, dig, _ = so.EXPECTED[name]
    assert int(v.sum()) == n_in
    assert sk.dtype == np.uint8 and sk.shape == v.shape and set(np.unique(sk)) <= {0, 1}
    assert int(sk.sum()) == n_out
    assert so.digest(sk) == dig
    assert passes >= 1


@pytest.mark.parametrize("name", so.CASES)
def test_skeleton_is_a_subset_with_the_input_topology(name):
    v, sk, _ = so.solved(name)
    assert not np.any(sk.astype(bool) & ~v.astype(bool))
    triple = so.EXPECTED[name][3]
    assert so.topology(v) == triple
    assert so.topology(sk) == triple


@pytest.mark.parametrize("name", so.CASES)
def test_oracle_is_idempotent(name):
    _, sk, _ = so.solved(name)
    again, passes = so.skeletonize(sk)
    assert np.array_equal(again, sk)
    assert passes == 1


def test_the_recheck_and_its_order_matter():
    """The cases are only worth pinning if they tell the raster-order re-check from no re-check and from the reverse order."""
    for name in ("ring", "two"):
        v, sk, _ = so.solved(name)
        assert not np.array_equal(so.skeletonize(v, recheck="none")[0], sk), name
        assert not np.array_equal(so.skeletonize(v, recheck="reverse")[0], sk), name
    v, _, _ = so.solved("two")
    assert so.topology(so.skeletonize(v, recheck="none")[0])[0] != 2       # a component is lost without the re-check


def test_workspace_query_is_pure_host():
    from seunet_amd import _lib
    lib = _lib.load()
    assert lib.seunet_skeleton_workspace_bytes(20, 24, 134) > 0
    assert lib.seunet_skeleton_workspace_bytes(1, 1, 70) > 0
    assert lib.seunet_skeleton_workspace_bytes(20, 0, 134) == 0
    assert "skeleton_workspace_bytes" in _lib.last_error()
    assert lib.seunet_skeleton_workspace_bytes(2048, 2048, 512) == 0         # 2^31 voxels
    assert "skeleton_workspace_bytes" in _lib.last_error()
