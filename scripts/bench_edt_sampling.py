"""Timing of the EDT with voxel spacing and of the per-branch wall distance (for DESIGN.md section 3k and the README), on the cases of
scripts/bench_morphometry.py: the synthetic airway-like tree laid out as 300 x 512 x 512 and the tube case of scripts/bench_prep.py.

1. ``distance_transform_edt(label, return_indices=True, sampling=SPACING)`` (dist and indices) beside the unit-sampling
   ``distance_transform_edt(label, return_indices=True)`` on the same volume in the same run: wall clock around a synchronise, and
   the library call alone between two events with the outputs and the workspace preallocated.
2. ``branch_wall_distance`` (indices given) beside ``branch_stats`` (sqdist given) on the tree labelled by ``tree_parsing`` (45
   branches) and on the tube case (1228): wall clock with the tables on the host, and ``seunet_branch_wall_stats`` /
   ``seunet_branch_stats`` alone between two events.
One warm-up call each, then the median of five.  No time here is a pass condition."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import seunet_amd as A
from seunet_amd import _lib
from skeleton_oracle import TREE_STAMPS

SHAPE, SCALE = (512, 512, 300), 2
SPACING = (1.25, 0.7, 0.7)                                   # (300, 512, 512): slices 1.25 apart, 0.7 in the plane


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


def events_ms(call):
    """The median of five of one library call between two events, after one warm-up call."""
    times = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:]))


def edt_device_ms(label, sampling):
    lib = _lib.load()
    n0, n1, n2 = label.shape
    dist = torch.empty(label.shape, dtype=torch.float64, device="cuda")
    ind = torch.empty((3,) + tuple(label.shape), dtype=torch.int32, device="cuda")
    status = torch.empty(1, dtype=torch.int32, device="cuda")
    if sampling is None:
        ws = torch.empty(lib.seunet_edt_workspace_bytes(n0, n1, n2), dtype=torch.uint8, device="cuda")
        return events_ms(lambda: _lib.check(lib.seunet_edt(label.data_ptr(), n0, n1, n2, None, dist.data_ptr(), ind.data_ptr(),
                                                           status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "edt"))
    ws = torch.empty(lib.seunet_edt_sampling_workspace_bytes(n0, n1, n2), dtype=torch.uint8, device="cuda")
    return events_ms(lambda: _lib.check(lib.seunet_edt_sampling(label.data_ptr(), n0, n1, n2, *sampling, dist.data_ptr(), ind.data_ptr(), None,
                                                                status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                                        "edt_sampling"))


def stats_device_ms(parsing, skel, sqdist, num):
    lib = _lib.load()
    rows = num + 1
    i64 = [torch.empty(rows * c, dtype=torch.int64, device="cuda") for c in (1, 3, 1, 13, 13, 1)]
    i32 = [torch.empty(rows * c, dtype=torch.int32, device="cuda") for c in (3, 3, 1, 1, 1)]
    args = (parsing.data_ptr(), skel.data_ptr(), sqdist.data_ptr(), *parsing.shape, num, i64[0].data_ptr(), i64[1].data_ptr(),
            i32[0].data_ptr(), i32[1].data_ptr(), i64[2].data_ptr(), i64[3].data_ptr(), i64[4].data_ptr(), i64[5].data_ptr(),
            i32[2].data_ptr(), i32[3].data_ptr(), i32[4].data_ptr(), _lib.stream_ptr())
    return events_ms(lambda: _lib.check(lib.seunet_branch_stats(*args), "branch_stats"))


def wall_device_ms(parsing, skel, indices, num):
    lib = _lib.load()
    rows = num + 1
    buf = torch.empty(6 * rows + 1, dtype=torch.int64, device="cuda")
    b = buf.data_ptr()
    args = (parsing.data_ptr(), skel.data_ptr(), indices.data_ptr(), *parsing.shape, num, *SPACING, b, b + 8 * rows, b + 32 * rows,
            b + 40 * rows, b + 48 * rows, _lib.stream_ptr())
    return events_ms(lambda: _lib.check(lib.seunet_branch_wall_stats(*args), "branch_wall_stats"))


def synthetic_tubes(shape, seed=3):
    """scripts/bench_prep.py's case: tubes around 400 random segments and their centre lines."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    skel = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    hi = torch.tensor(shape, device="cuda")
    for _ in range(400):
        a, b = torch.rand(3, generator=g, device="cuda") * (hi - 1), torch.rand(3, generator=g, device="cuda") * (hi - 1)
        m = int((b - a).abs().max()) + 1
        t = torch.linspace(0, 1, m, device="cuda")[:, None]
        p = (a + (b - a) * t).round().long()
        skel[p[:, 0], p[:, 1], p[:, 2]] = 1
    return torch.nn.functional.max_pool3d(skel[None, None].float(), 5, 1, 2)[0, 0].to(torch.uint8), skel


def run(name, label, skel):
    n = label.numel()
    t_unit, lo_u, hi_u, (_, ind_unit) = median_ms(lambda: A.distance_transform_edt(label, return_indices=True))
    t_samp, lo_s, hi_s, (dist, indices) = median_ms(lambda: A.distance_transform_edt(label, return_indices=True, sampling=SPACING))
    d_unit, d_samp = edt_device_ms(label, None), edt_device_ms(label, SPACING)
    moved = int((indices != ind_unit).any(dim=0).sum())
    print("edt %s %dx%dx%d, %d foreground voxels, sampling %s: the nearest zero voxel differs from the unit-sampling one at %d voxels"
          % ((name,) + tuple(label.shape) + (int((label != 0).sum()), SPACING, moved)), flush=True)
    print("  unit sampling, dist + indices     median of 5 %9.3f ms (min %.3f, max %.3f); seunet_edt alone (events) %.3f ms"
          % (t_unit, lo_u, hi_u, d_unit), flush=True)
    print("  with sampling, dist + indices     median of 5 %9.3f ms (min %.3f, max %.3f); seunet_edt_sampling alone (events) %.3f ms"
          % (t_samp, lo_s, hi_s, d_samp), flush=True)
    print("  ratio sampled / unit: %.2f (wall clock), %.2f (device)" % (t_samp / t_unit, d_samp / d_unit), flush=True)
    del ind_unit, dist
    sqdist = A.distance_transform_edt(label, return_distances=False, return_sqdist=True)
    parsing = A.tree_parsing(label, skel, refine=False)
    num = int(parsing.max())
    t_stats, lo_st, hi_st, stats = median_ms(lambda: A.branch_stats(parsing, skel, num, sqdist))
    t_wall, lo_w, hi_w, wall = median_ms(lambda: A.branch_wall_distance(parsing, skel, SPACING, num, indices=indices))
    d_stats, d_wall = stats_device_ms(parsing, skel, sqdist, num), wall_device_ms(parsing, skel, indices, num)
    assert np.array_equal(wall["wall_count"], stats["skeleton_voxels"])          # every labelled skeleton voxel has a feature
    print("wall distance %s, tree_parsing(refine=False): num = %d, %d labelled skeleton voxels, %.1f MB of skeleton"
          % (name, num, int(wall["wall_count"].sum()), 1e-6 * n), flush=True)
    print("  branch_stats (sqdist given, tables on the host)         median of 5 %9.3f ms (min %.3f, max %.3f); device alone %.3f ms"
          % (t_stats, lo_st, hi_st, d_stats), flush=True)
    print("  branch_wall_distance (indices given, tables on the host) median of 5 %9.3f ms (min %.3f, max %.3f); device alone %.3f ms"
          % (t_wall, lo_w, hi_w, d_wall), flush=True)
    print("  ratio wall / branch_stats: %.2f (wall clock), %.2f (device; branch_stats' device time holds its volume pass too)"
          % (t_wall / t_stats, d_wall / d_stats), flush=True)


vol = np.zeros(SHAPE, dtype=bool)
for gi in range(3):
    for gj in range(3):
        off = (60 + 150 * gi, 60 + 150 * gj, 26)
        for a, b, r2 in TREE_STAMPS:
            stamp(vol, [SCALE * a[i] + off[i] for i in range(3)], [SCALE * b[i] + off[i] for i in range(3)], SCALE * SCALE * r2)
tall = torch.from_numpy(vol.view(np.uint8)).cuda()                       # (512, 512, 300): the trunks along axis 2, quick to thin
skel = A.skeletonize_3d(tall).permute(2, 0, 1).contiguous()
label = tall.permute(2, 0, 1).contiguous()                              # (300, 512, 512)
run("tree", label, skel)
del tall
run("tubes", *synthetic_tubes((300, 512, 512)))
