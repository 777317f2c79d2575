"""Generate tests/golden/edt_sampling_known.npz: scipy's ``distance_transform_edt(volume, sampling=s, return_indices=True)`` on
small synthetic volumes, recorded from scipy itself (the fixture names the version and the machine).

Per case k: ``case{k}_vol`` uint8, ``case{k}_sampling`` float64[3], ``case{k}_indices`` int16 (3, n0, n1, n2) and ``case{k}_sha256``,
the SHA-256 of scipy's ``dist.tobytes()``.  The distances themselves are not stored: a test recomputes them from the indices with
the numpy formula of DESIGN.md section 3k and checks the hash, which pins them bit for bit in tens of kilobytes.

The shapes have an extent of 1 on each axis in turn, odd extents, a volume with a single zero voxel and one whose zeros lie in two
planes of axis 2 only, so that whole lines and whole planes have no site after the pass along axis 0.  Densities of zeros: 0.5, 0.05
and 0.005.  Samplings: (1, 1, 1), which must equal the integer EDT; (0.5, 1, 2) and (1, 2, 2), where all arithmetic is exact and ties
are frequent; (0.7, 0.7, 1.25), (2.5, 0.68, 0.68), (1/3, 0.1, 7.0) and (1, 1, 3), where rounding matters.

Usage: python scripts/make_golden_edt_sampling.py
"""
import hashlib
import os
import platform

import numpy as np
import scipy
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "edt_sampling_known.npz")

SAMPLINGS = ((1.0, 1.0, 1.0), (0.5, 1.0, 2.0), (1.0, 2.0, 2.0), (0.7, 0.7, 1.25), (2.5, 0.68, 0.68), (1.0 / 3.0, 0.1, 7.0), (1.0, 1.0, 3.0))
DENSITIES = (0.5, 0.05, 0.005)
# (shape, kind)
VOLUMES = (((1, 1, 5), "random"), ((16, 1, 3), "random"), ((1, 9, 1), "random"), ((7, 9, 11), "random"), ((13, 10, 11), "random"),
           ((6, 7, 8), "single"), ((8, 9, 10), "planes"))
CASES = 24


def volume(shape, kind, density, rng):
    """uint8, 0 = site.  Every volume has at least one zero voxel."""
    v = np.ones(shape, dtype=np.uint8)
    if kind == "single":
        v[tuple(int(rng.integers(0, n)) for n in shape)] = 0
        return v
    zeros = rng.random(shape) < density
    if kind == "planes":                                      # zeros in the planes i2 = 2 and i2 = 7 only, a few per plane
        keep = np.zeros(shape, dtype=bool)
        keep[:, :, (2, 7)] = True
        zeros = (rng.random(shape) < max(density, 0.05)) & keep
    v[zeros] = 0
    if v.all():
        v[tuple(int(rng.integers(0, n)) for n in shape)] = 0
    return v


def main():
    rng = np.random.default_rng(20241)
    out = {"scipy_version": np.array(scipy.__version__), "machine": np.array(platform.machine()), "cases": np.array(CASES)}
    for k in range(CASES):
        shape, kind = VOLUMES[k % len(VOLUMES)]
        density = DENSITIES[k % len(DENSITIES)]
        s = SAMPLINGS[(k + k // len(SAMPLINGS)) % len(SAMPLINGS)]
        v = volume(shape, kind, density, rng)
        dist, ind = ndimage.distance_transform_edt(v, sampling=s, return_indices=True)
        assert dist.dtype == np.float64 and ind.min() >= 0 and ind.max() < 32768
        out[f"case{k}_vol"] = v
        out[f"case{k}_sampling"] = np.asarray(s, dtype=np.float64)
        out[f"case{k}_indices"] = ind.astype(np.int16)
        out[f"case{k}_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(dist).tobytes()).hexdigest())
        print(k, shape, kind, density, s, int((v == 0).sum()), "zeros")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
