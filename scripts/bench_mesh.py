"""Timing of the surface meshing (seunet_amd.mesh) on the synthetic airway-like tree of scripts/bench_skeleton.py, laid out as
300 x 512 x 512 (for DESIGN.md section 3h and the README): extraction, adjacency, smoothing, STL records, and skeletonize_3d on
the same volume in the same run for scale.  One warm-up call each, then the median of five.  No time here is a pass condition."""
import io, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import seunet_amd as A
from skeleton_oracle import TREE_STAMPS

SHAPE, SCALE = (512, 512, 300), 2


def stamp(v, a, b, r2):
    n = max(abs(b[i] - a[i]) for i in range(3))
    r = int(np.sqrt(r2)) + 1
    o = np.arange(-r, r + 1)
    ball = (o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) <= r2
    for t in range(n + 1):
        p = [a[i] + ((b[i] - a[i]) * t) // n for i in range(3)]
        v[p[0] - r:p[0] + r + 1, p[1] - r:p[1] + r + 1, p[2] - r:p[2] + r + 1] |= ball      # the grid keeps every ball inside


def median_ms(fn):
    fn()                                                    # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), min(times), max(times), out


vol = np.zeros(SHAPE, dtype=bool)
for gi in range(3):
    for gj in range(3):
        off = (60 + 150 * gi, 60 + 150 * gj, 26)
        for a, b, r2 in TREE_STAMPS:
            stamp(vol, [SCALE * a[i] + off[i] for i in range(3)], [SCALE * b[i] + off[i] for i in range(3)], SCALE * SCALE * r2)
label = torch.from_numpy(np.ascontiguousarray(vol.transpose(2, 0, 1)).view(np.uint8)).cuda()       # (300, 512, 512)

rows = []
t, lo, hi, (verts, faces) = median_ms(lambda: A.marching_cubes(label))
rows.append(("marching_cubes", t, lo, hi))
V, F = int(verts.shape[0]), int(faces.shape[0])
t, lo, hi, adj = median_ms(lambda: A.mesh_adjacency(faces, V))
rows.append(("mesh_adjacency", t, lo, hi))
t, lo, hi, smooth = median_ms(lambda: A.smooth_mesh(verts, faces))
rows.append(("smooth_mesh (adjacency + 20 sweeps)", t, lo, hi))
t, lo, hi, rec = median_ms(lambda: A.stl_records(smooth, faces))
rows.append(("stl_records", t, lo, hi))
t, lo, hi, nbytes = median_ms(lambda: A.write_stl(io.BytesIO(), smooth, faces))
rows.append(("write_stl to memory (records + one copy to the host)", t, lo, hi))
t, lo, hi, skel = median_ms(lambda: A.skeletonize_3d(label))
rows.append(("skeletonize_3d (same volume, for scale)", t, lo, hi))

print("mesh %dx%dx%d, %d foreground voxels: V = %d, F = %d, boundary vertices %d, mean degree %.2f, STL %d bytes"
      % (tuple(label.shape) + (int(vol.sum()), V, F, int(adj[2].sum()), float(adj[1].numel()) / max(V, 1), nbytes)), flush=True)
for name, t, lo, hi in rows:
    print("  %-55s median of 5 %8.2f ms (min %.2f, max %.2f)" % (name, t, lo, hi), flush=True)
