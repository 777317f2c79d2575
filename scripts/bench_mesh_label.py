"""Timing of the labelled surface meshing (seunet_amd.label_meshes / branch_meshes) on the synthetic airway-like tree of
scripts/bench_skeleton.py, laid out as 300 x 512 x 512 and labelled by tree_parsing without and with its refinement (for DESIGN.md
section 3i and the README), and on the tube case of scripts/bench_prep.py, whose random segments give the labelling hundreds of
branches (the README's 1228 before and 423 after refinement); next to each the only other way to get the branches' meshes: the loop over marching_cubes(parsing == k).
One warm-up call each, then the median of five, wall clock around a synchronise.  No time here is a pass condition."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import seunet_amd as A
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


def loop_label_meshes(parsing):
    """What there is without label_meshes: one extraction, and one synchronise, per label that occurs (the reference also
    passes over the volume for the labels that do not)."""
    return {k: A.marching_cubes(parsing == k) for k in torch.unique(parsing).tolist() if k}


def loop_branch_meshes(parsing, centre):
    out = {}
    for k in torch.unique(parsing).tolist():
        if k:
            v, f = A.marching_cubes(parsing == k)
            out[k] = (A.smooth_mesh(A.transform_mesh(v, centre, SPACING), f, 20, 0.15), f)
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


def run(name, label, skel):
    centre = A.mesh.mean_coordinate(skel)
    for refine in (False, True):
        parsing, num = A.tree_parsing(label, skel, refine=refine, return_num=True)    # refinement keeps the surviving numbers
        t_new, lo_new, hi_new, m = median_ms(lambda: A.label_meshes(parsing))
        t_loop, lo_loop, hi_loop, each = median_ms(lambda: loop_label_meshes(parsing))
        assert sum(len(v) for v, _ in each.values()) == len(m.verts) and sum(len(f) for _, f in each.values()) == len(m.faces)
        assert m.num == max(each)
        for k in each:
            assert torch.equal(m.mesh(k)[0], each[k][0]) and torch.equal(m.mesh(k)[1], each[k][1])
        t_bnew, lo_bnew, hi_bnew, b = median_ms(lambda: A.branch_meshes(parsing, SPACING, centre))
        t_bloop, lo_bloop, hi_bloop, beach = median_ms(lambda: loop_branch_meshes(parsing, centre))
        for k in beach:
            assert torch.equal(b.mesh(k)[0], beach[k][0])
        print("mesh_label %s %dx%dx%d, %d foreground voxels, tree_parsing(refine=%s): num = %d (%d labels with voxels, the largest %d), V = %d, F = %d"
              % ((name,) + tuple(label.shape) + (int(label.sum()), refine, num, len(each), m.num, len(m.verts), len(m.faces))), flush=True)
        for what, t, lo, hi in (("label_meshes", t_new, lo_new, hi_new),
                                ("loop of marching_cubes(parsing == k)", t_loop, lo_loop, hi_loop),
                                ("branch_meshes (transform + adjacency + 20 sweeps)", t_bnew, lo_bnew, hi_bnew),
                                ("loop of marching_cubes, transform_mesh, smooth_mesh", t_bloop, lo_bloop, hi_bloop)):
            print("  %-55s median of 5 %9.2f ms (min %.2f, max %.2f)" % (what, t, lo, hi), flush=True)
        assert t_new < t_loop and t_bnew < t_bloop, "the one extraction must beat the loop over the labels"


run("tree", label, skel)
run("tubes", *synthetic_tubes((300, 512, 512)))
