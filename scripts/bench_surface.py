"""Timing of the boundary metrics (for DESIGN.md section 3m and the README), on the cases of scripts/bench_edt_sampling.py: the
synthetic airway-like tree laid out as 300 x 512 x 512 and the tube case of scripts/bench_prep.py, as label, under the sampling
(1.25, 0.7, 0.7).  The prediction is the label dilated once (``binary_dilation``) with a block of it cleared.

1. ``surface_metrics(pred, label, SPACING)``: border extraction, the two distance transforms on the bounding box, gather, summary
   and radix select (csrc/surface.hip).
2. In the same run, the composition a user could write before from public calls: ``binary_erosion`` twice,
   ``distance_transform_edt(~border, sampling=SPACING)`` twice with ``dist`` on the full volume, boolean indexing, ``torch.sort``
   of the pooled distances, then maximum, mean and the 95th percentile from the sorted vector.
Both between two events (the host waits inside each are part of what a caller pays), one warm-up call each, then the median of five;
the two are checked against each other before a time is printed.  No time here is a pass condition."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import numpy as np
import torch
import seunet_amd as A
from seunet_amd import postprocess as P
from skeleton_oracle import TREE_STAMPS

SHAPE, SCALE = (512, 512, 300), 2
SPACING = (1.25, 0.7, 0.7)                                   # (300, 512, 512): slices 1.25 apart, 0.7 in the plane
Q = 95.0


def stamp(v, a, b, r2):
    n = max(abs(b[i] - a[i]) for i in range(3))
    r = int(np.sqrt(r2)) + 1
    o = np.arange(-r, r + 1)
    ball = (o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) <= r2
    for t in range(n + 1):
        p = [a[i] + ((b[i] - a[i]) * t) // n for i in range(3)]
        v[p[0] - r:p[0] + r + 1, p[1] - r:p[1] + r + 1, p[2] - r:p[2] + r + 1] |= ball      # the grid keeps every ball inside


def synthetic_tubes(shape, seed=3):
    """scripts/bench_prep.py's case: tubes around 400 random segments."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    skel = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    hi = torch.tensor(shape, device="cuda")
    for _ in range(400):
        a, b = torch.rand(3, generator=g, device="cuda") * (hi - 1), torch.rand(3, generator=g, device="cuda") * (hi - 1)
        m = int((b - a).abs().max()) + 1
        t = torch.linspace(0, 1, m, device="cuda")[:, None]
        p = (a + (b - a) * t).round().long()
        skel[p[:, 0], p[:, 1], p[:, 2]] = 1
    return torch.nn.functional.max_pool3d(skel[None, None].float(), 5, 1, 2)[0, 0].to(torch.uint8)


def events_ms(call):
    """(median of five, min, max, last result) of one call between two events, after one warm-up call."""
    times, out = [], None
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:])), min(times[1:]), max(times[1:]), out


def composition(pred, label):
    """(hd, assd, pooled percentile, n_a, n_b) from public calls alone."""
    borders = [m & (A.binary_erosion(m) ^ 1) for m in (pred, label)]
    d_ab = A.distance_transform_edt(borders[1] ^ 1, sampling=SPACING)[borders[0] != 0]
    d_ba = A.distance_transform_edt(borders[0] ^ 1, sampling=SPACING)[borders[1] != 0]
    d, _ = torch.sort(torch.cat([d_ab, d_ba]))
    n = d.numel()
    lo, hi, g = P._percentile_ranks(n, Q)
    picks = d[torch.tensor([lo, hi, n - 1], device=d.device)].cpu().numpy()
    return float(picks[2]), float(d.sum() / n), float(P._percentile_lerp(picks[0], picks[1], g)), d_ab.numel(), d_ba.numel()


def run(name, label):
    pred = A.binary_dilation(label)
    n0, n1, n2 = pred.shape
    pred[n0 // 3:n0 // 3 + 24, n1 // 3:n1 // 3 + 64, n2 // 3:n2 // 3 + 64] = 0
    t_new, lo_n, hi_n, m = events_ms(lambda: A.surface_metrics(pred, label, SPACING, percentile=Q))
    t_old, lo_o, hi_o, c = events_ms(lambda: composition(pred, label))
    assert (m.hd, m.hd_percentile_pooled, m.n_a, m.n_b) == (c[0], c[2], c[3], c[4]), (m, c)
    assert abs(m.assd - c[1]) <= 1e-9 * c[1], (m.assd, c[1])
    union = torch.nonzero(pred | label)
    box = [(int(union[:, k].min()), int(union[:, k].max()) + 1) for k in range(3)]
    ext = tuple(h - l for l, h in box)
    print("surface metrics %s %dx%dx%d, sampling %s: %d + %d surface voxels, box %s = %dx%dx%d (%.1f %% of the volume)"
          % ((name, n0, n1, n2, SPACING, m.n_a, m.n_b, box) + ext + (100.0 * ext[0] * ext[1] * ext[2] / pred.numel(),)), flush=True)
    print("  hd %.4f, hd95 per direction %.4f, pooled %.4f, assd %.4f, nsd(1.0) %.4f" % (m.hd, m.hd_percentile, m.hd_percentile_pooled, m.assd, m.nsd[0]),
          flush=True)
    print("  surface_metrics                        median of 5 %9.3f ms (min %.3f, max %.3f)" % (t_new, lo_n, hi_n), flush=True)
    print("  composition of public calls            median of 5 %9.3f ms (min %.3f, max %.3f)" % (t_old, lo_o, hi_o), flush=True)
    print("  ratio composition / surface_metrics: %.2f" % (t_old / t_new), flush=True)


vol = np.zeros(SHAPE, dtype=bool)
for gi in range(3):
    for gj in range(3):
        off = (60 + 150 * gi, 60 + 150 * gj, 26)
        for a, b, r2 in TREE_STAMPS:
            stamp(vol, [SCALE * a[i] + off[i] for i in range(3)], [SCALE * b[i] + off[i] for i in range(3)], SCALE * SCALE * r2)
label = torch.from_numpy(vol.view(np.uint8)).cuda().permute(2, 0, 1).contiguous()   # (300, 512, 512)
run("tree", label)
del label
run("tubes", synthetic_tubes((300, 512, 512)))
