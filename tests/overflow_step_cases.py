"""Shared by tests/test_overflow_step_host.py and tests/test_overflow_step_gpu.py: the AdamW oracle over a step list with
skipped steps, the overflow patterns, the registry inputs and the one comparison both files use.

A step behind an fp16 backward pass that overflowed must be a no-op: parameters and both moments keep their bits and the bias
corrections of later steps count applied steps only.  ``run_with_skips`` states that directly (the skipped index is passed
over, ``t`` does not advance); the host file asserts that it equals ``adamw_oracle.run`` on the list with those steps removed.

``failing_tensors`` is the GPU tests' comparison with the tolerances tests/test_optim_gpu.py uses against the f32 oracle
(params ``rtol=2e-7, atol=1e-9``; moments ``rtol=2e-6, atol=3e-7 * max|ref|``), returned as a list of tensor indices so
that the host file can show that it separates: a zero-gradient step in place of the skipped one must FAIL it on at least half
of the tensors, or the GPU tests could pass on an optimizer that does not skip.

This is a plain helper module: no pytest configuration, nothing that changes how Python starts."""
import functools

import numpy as np
import torch

import adamw_oracle as ao

STEPS = 6
LR = 1e-4
# indices (from 0) of the steps whose backward pass overflowed
PATTERNS = {"first": (0,), "middle": (2,), "two-in-a-row": (2, 3), "last": (STEPS - 1,), "none": ()}
RAGGED_SHAPES = [(5,), (1,), (257, 9), (4, 4, 3, 3, 3), (2049,)]       # the list of test_matches_torch_gpu_adamw_and_edge_cases


def run_with_skips(params, grads_per_step, lrs, skip=(), **hyper):
    """``adamw_oracle.run`` with the steps whose index is in ``skip`` passed over: p, m, v untouched, ``t`` not advanced."""
    p = [a.astype(ao.F32).copy() for a in params]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    t = 0
    for k, (grads, lr) in enumerate(zip(grads_per_step, lrs)):
        if k in skip:
            continue
        t += 1
        for i in range(len(p)):
            ao.adamw_step(p[i], grads[i].astype(ao.F32), m[i], v[i], t, lr, **hyper)
    return {"params": p, "exp_avg": m, "exp_avg_sq": v}


def without(seq, skip):
    return [x for k, x in enumerate(seq) if k not in skip]


@functools.lru_cache(maxsize=None)
def registry_inputs():
    """The 117 registry shapes of test_against_oracle_on_the_network_registry (init x 0.1, gradients x 1e-3), STEPS steps."""
    import seunet_oracle as orc
    g = torch.Generator().manual_seed(7)
    shapes = [s for _, s in orc.parameter_registry(2, 1, 1)]
    init = [(torch.randn(s, generator=g) * 0.1).numpy() for s in shapes]
    grads = [[(torch.randn(s, generator=g) * 1e-3).numpy() for s in shapes] for _ in range(STEPS)]
    return init, grads


@functools.lru_cache(maxsize=None)
def registry_reference(pattern):
    """The oracle's trajectory with the pattern's steps removed (computed once per pattern; do not modify)."""
    init, grads = registry_inputs()
    skip = PATTERNS[pattern]
    return ao.run(init, without(grads, skip), [LR] * (STEPS - len(skip)))


def _close(got, ref, rtol, atol):
    return bool((np.abs(got.astype(np.float64) - ref) <= atol + rtol * np.abs(ref)).all())


def failing_tensors(got, want):
    """Indices of the tensors at which params, exp_avg or exp_avg_sq of ``got`` miss ``want`` (dicts as ``adamw_oracle.run``
    returns them) under the optimizer tests' tolerances."""
    bad = []
    for i, ref in enumerate(want["params"]):
        ok = _close(got["params"][i], ref, 2e-7, 1e-9)
        for k in ("exp_avg", "exp_avg_sq"):
            r = want[k][i]
            ok = ok and _close(got[k][i], r, 2e-6, 3e-7 * float(np.abs(r).max()))
        if not ok:
            bad.append(i)
    return bad
