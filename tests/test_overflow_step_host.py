"""Host part of the overflow-step tests (tests/overflow_step_cases.py): the oracle with skipped steps is the oracle on the
shortened list, and the GPU tests' comparison tells a skipped step from a zero-gradient step."""
import numpy as np
import pytest

import adamw_oracle as ao
import overflow_step_cases as OC


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("pattern", list(OC.PATTERNS))
def test_skipped_steps_equal_the_list_with_those_steps_removed(pattern):
    """Bitwise, with a learning rate that changes per step (the skipped step's lr goes with it) and non-default
    hyper-parameters; a skipped step leaves p, m, v untouched and does not advance t."""
    skip = OC.PATTERNS[pattern]
    rng = np.random.RandomState(11)
    shapes = OC.RAGGED_SHAPES
    init = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    grads = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(OC.STEPS)]
    lrs = [3e-3 * 0.7 ** k for k in range(OC.STEPS)]
    hyper = dict(beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=0.1)
    got = OC.run_with_skips(init, grads, lrs, skip, **hyper)
    want = ao.run(init, OC.without(grads, skip), OC.without(lrs, skip), **hyper)
    for k in ("params", "exp_avg", "exp_avg_sq"):
        for a, b in zip(got[k], want[k]):
            assert np.array_equal(_bits(a), _bits(b)), (pattern, k)
    # up to and including a skipped step nothing has moved since the step before it
    for s in skip:
        before = OC.run_with_skips(init, grads[:s], lrs[:s], skip, **hyper)
        after = OC.run_with_skips(init, grads[:s + 1], lrs[:s + 1], skip, **hyper)
        for k in ("params", "exp_avg", "exp_avg_sq"):
            for a, b in zip(before[k], after[k]):
                assert np.array_equal(_bits(a), _bits(b)), (pattern, s, k)
    if pattern == "first":      # the step after a skipped first step is step 1: m = (1 - beta1) g, v = (1 - beta2) g^2
        one = OC.run_with_skips(init, grads[:2], lrs[:2], skip, **hyper)
        np.testing.assert_allclose(one["exp_avg"][2], np.float32(1 - 0.8) * grads[1][2], rtol=1e-6)
        np.testing.assert_allclose(one["exp_avg_sq"][2], np.float32(1 - 0.95) * grads[1][2] ** 2, rtol=1e-6)


@pytest.mark.parametrize("pattern", [p for p, s in OC.PATTERNS.items() if s])
def test_a_zero_gradient_step_fails_the_gpu_comparison(pattern):
    """What the optimizer did before it was gated: the overflowing backward left zero gradients and the step was applied (weight
    decay, both moments shrunk, t advanced, a move along the stale momentum).  On the 117 registry tensors that trajectory
    must miss the skipped-step reference under the GPU tests' own tolerances on at least half of the tensors."""
    skip = OC.PATTERNS[pattern]
    init, grads = OC.registry_inputs()
    zeroed = [[np.zeros_like(g) for g in gs] if k in skip else gs for k, gs in enumerate(grads)]
    got = ao.run(init, zeroed, [OC.LR] * OC.STEPS)
    want = OC.registry_reference(pattern)
    bad = OC.failing_tensors(got, want)
    print(f"zero-gradient step(s) at {skip}: {len(bad)} of {len(init)} tensors miss the comparison")
    assert len(init) == 117 and 2 * len(bad) >= len(init), (pattern, len(bad))


def test_the_comparison_passes_on_the_reference_itself_and_fails_on_one_beta2_too_many():
    want = OC.registry_reference("middle")
    assert OC.failing_tensors(want, want) == []
    off = {k: [a.copy() for a in v] for k, v in want.items()}
    off["exp_avg_sq"][5] = off["exp_avg_sq"][5] * np.float32(0.999)         # one beta2 too many
    assert OC.failing_tensors(off, want) == [5]
