"""Timing of prep.skeletonize_3d on a synthetic airway-like tree at 512 x 512 x 320 (for DESIGN.md section 3d and the README).

The tree is the `tree` volume of tests/skeleton_oracle.py (integer stamping of balls along segments) with every coordinate
doubled and every squared radius multiplied by four, nine copies on a 3 x 3 grid: a trachea of radius 8.5 voxels, two
generations of branches, about the voxel count of a real airway label.  One warm-up call, then the median of five."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import seunet_amd as A
from seunet_amd import prep
from skeleton_oracle import TREE_STAMPS

SHAPE, SCALE = (512, 512, 320), 2


def stamp(v, a, b, r2):
    n = max(abs(b[i] - a[i]) for i in range(3))
    r = int(np.sqrt(r2)) + 1
    o = np.arange(-r, r + 1)
    ball = (o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) <= r2
    for t in range(n + 1):
        p = [a[i] + ((b[i] - a[i]) * t) // n for i in range(3)]
        v[p[0] - r:p[0] + r + 1, p[1] - r:p[1] + r + 1, p[2] - r:p[2] + r + 1] |= ball      # the grid keeps every ball inside


vol = np.zeros(SHAPE, dtype=bool)
for gi in range(3):
    for gj in range(3):
        off = (60 + 150 * gi, 60 + 150 * gj, 26)
        for a, b, r2 in TREE_STAMPS:
            stamp(vol, [SCALE * a[i] + off[i] for i in range(3)], [SCALE * b[i] + off[i] for i in range(3)], SCALE * SCALE * r2)
label = torch.from_numpy(vol.view(np.uint8)).cuda()
skel, passes = prep.skeletonize_3d(label, return_passes=True)       # warm-up
torch.cuda.synchronize()
times = []
for _ in range(5):
    t0 = time.perf_counter()
    again = prep.skeletonize_3d(label)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
assert torch.equal(again, skel)
launches = 3 + passes * 6 * (prep.SKELETON_ROUND_LAUNCHES + 2)      # pack, unpack, pass count; candidates + rounds + tail per sub-iteration
print("skeletonize_3d %dx%dx%d, %d -> %d voxels: passes %d, launches %d, median of 5 %.1f ms (min %.1f, max %.1f)"
      % (SHAPE + (int(vol.sum()), int(skel.sum()), passes, launches, 1e3 * float(np.median(times)), 1e3 * min(times), 1e3 * max(times))),
      flush=True)
