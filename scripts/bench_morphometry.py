"""Timing of the branch morphometry (seunet_amd.branch_stats / branch_morphometry) on the two cases of scripts/bench_mesh_label.py: the
synthetic airway-like tree laid out as 300 x 512 x 512 and the tube case of scripts/bench_prep.py, each labelled by tree_parsing
without and with its refinement (for DESIGN.md section 3j and the README).  Next to them, in the same run: seunet_label_stats on the
same volume (the existing one-pass kernel over the same bytes), the device part of seunet_branch_stats alone between two events,
and the alternative there is today, a loop of masked torch reductions per label (without the links, which it has no short form
for).  Last, the contention worst case: one label over the whole all-foreground volume.
One warm-up call each, then the median of five, wall clock around a synchronise.  No time here is a pass condition."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import seunet_amd as A
from seunet_amd import _lib
from skeleton_oracle import TREE_STAMPS

SHAPE, SCALE = (512, 512, 300), 2
SPACING = (0.7, 0.7, 1.0)


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


def device_ms(parsing, skel, sqdist, num):
    """seunet_branch_stats alone: the three launches between two events, tables preallocated, nothing copied back."""
    lib = _lib.load()
    rows = num + 1
    i64 = [torch.empty(rows * c, dtype=torch.int64, device="cuda") for c in (1, 3, 1, 13, 13, 1)]     # voxels coord skv links cross r2
    i32 = [torch.empty(rows * c, dtype=torch.int32, device="cuda") for c in (3, 3, 1, 1, 1)]           # box_min box_max r2_min r2_max status
    args = (parsing.data_ptr(), skel.data_ptr(), sqdist.data_ptr(), *parsing.shape, num, i64[0].data_ptr(), i64[1].data_ptr(),
            i32[0].data_ptr(), i32[1].data_ptr(), i64[2].data_ptr(), i64[3].data_ptr(), i64[4].data_ptr(), i64[5].data_ptr(),
            i32[2].data_ptr(), i32[3].data_ptr(), i32[4].data_ptr(), _lib.stream_ptr())
    times = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.seunet_branch_stats(*args), "branch_stats")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:])), i64[0]


def loop_of_masks(parsing, skel, sqdist, num):
    """What there is without branch_stats: per label a mask and reductions over it (volume, centroid, box, skeleton voxels, radii)."""
    out = []
    for k in range(1, num + 1):
        m = parsing == k
        nz = m.nonzero()
        if nz.shape[0] == 0:
            continue
        r2 = sqdist[m & (skel != 0)]
        out.append((nz.shape[0], nz.sum(0), nz.min(0).values, nz.max(0).values, r2.numel(),
                    r2.sum() if r2.numel() else 0, r2.min() if r2.numel() else 0, r2.max() if r2.numel() else 0))
    return out


vol = np.zeros(SHAPE, dtype=bool)
for gi in range(3):
    for gj in range(3):
        off = (60 + 150 * gi, 60 + 150 * gj, 26)
        for a, b, r2 in TREE_STAMPS:
            stamp(vol, [SCALE * a[i] + off[i] for i in range(3)], [SCALE * b[i] + off[i] for i in range(3)], SCALE * SCALE * r2)
tall = torch.from_numpy(vol.view(np.uint8)).cuda()                       # (512, 512, 300): the trunks along axis 2, quick to thin
skel = A.skeletonize_3d(tall).permute(2, 0, 1).contiguous()             # any skeleton of the tree serves the labelling
label = tall.permute(2, 0, 1).contiguous()                              # (300, 512, 512)


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


def report(rows):
    for what, t, lo, hi in rows:
        print("  %-62s median of 5 %9.3f ms (min %.3f, max %.3f)" % (what, t, lo, hi), flush=True)


def run(name, label, skel):
    sqdist = A.distance_transform_edt(label, return_distances=False, return_sqdist=True)
    n = label.numel()
    for refine in (False, True):
        parsing = A.tree_parsing(label, skel, refine=refine)
        num = int(parsing.max())                              # the refinement keeps the surviving numbers: the largest label counts
        t_stats, lo_stats, hi_stats, stats = median_ms(lambda: A.branch_stats(parsing, skel, num, sqdist))
        t_tab, lo_tab, hi_tab, table = median_ms(lambda: A.branch_morphometry(parsing, skel, SPACING, num, sqdist))
        t_ls, lo_ls, hi_ls, (counts, _) = median_ms(lambda: A.prep._label_stats(parsing, num))
        t_dev, voxels_dev = device_ms(parsing, skel, sqdist, num)
        t_loop, lo_loop, hi_loop, each = median_ms(lambda: loop_of_masks(parsing, skel, sqdist, num))
        assert np.array_equal(stats["voxels"], counts[1:]) and np.array_equal(voxels_dev.cpu().numpy()[1:], counts[1:])
        assert [e[0] for e in each] == [int(v) for v in stats["voxels"] if v]
        skv = int(stats["skeleton_voxels"].sum())
        own = stats["links"].sum(axis=1)
        on = stats["skeleton_voxels"] > 0
        print("morphometry %s %dx%dx%d, %d foreground voxels, %d labelled skeleton voxels, tree_parsing(refine=%s): num = %d (%d labels "
              "with voxels), %d links + %d cross links, links - (skeleton voxels - 1) per branch in [%d, %d], total length %.1f, "
              "%d leaves, %d generations"
              % ((name,) + tuple(label.shape) + (int(stats["voxels"].sum()), skv, refine, num, table.n_branches, int(own.sum()),
                                                  int(stats["cross_links"].sum()) // 2, int((own - stats["skeleton_voxels"] + 1)[on].min()),
                                                  int((own - stats["skeleton_voxels"] + 1)[on].max()), table.total_length, table.n_leaves,
                                                  table.max_generation + 1)), flush=True)
        report((("branch_stats (tables on the host)", t_stats, lo_stats, hi_stats),
                ("branch_morphometry (skeleton and sqdist given)", t_tab, lo_tab, hi_tab),
                ("label statistics (seunet_label_stats, tables on the host)", t_ls, lo_ls, hi_ls),
                ("loop of masked torch reductions per label (no links)", t_loop, lo_loop, hi_loop)))
        print("  seunet_branch_stats on the device alone (events): %.3f ms for %.1f MB of parsing + %.1f MB of skeleton = %.2f TB/s"
              % (t_dev, 4e-6 * n, 1e-6 * n, 5e-9 * n / t_dev), flush=True)
        assert t_stats < t_loop, "the one reduction must beat the loop over the labels"


run("tree", label, skel)
run("tubes", *synthetic_tubes((300, 512, 512)))

# the contention worst case: every voxel foreground, one label, every voxel on the skeleton
ones = torch.ones((300, 512, 512), dtype=torch.int32, device="cuda")
mask = torch.ones((300, 512, 512), dtype=torch.uint8, device="cuda")
sq = torch.full((300, 512, 512), 9, dtype=torch.int32, device="cuda")
t_dev, _ = device_ms(ones, mask, sq, 1)
t_wall, lo_wall, hi_wall, stats = median_ms(lambda: A.branch_stats(ones, mask, 1, sq))
assert stats["voxels"].tolist() == [ones.numel()] and stats["links"][0, 0] == 300 * 512 * 511
print("morphometry worst case 300x512x512, one label on every voxel, every voxel on the skeleton", flush=True)
report((("branch_stats (tables on the host)", t_wall, lo_wall, hi_wall),))
print("  seunet_branch_stats on the device alone (events): %.3f ms" % t_dev, flush=True)
