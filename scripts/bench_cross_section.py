"""Timing of the airway cross-sections (seunet_amd.cross_sections) on the two cases of scripts/bench_morphometry.py: the synthetic
airway-like tree laid out as 300 x 512 x 512 and the tube case of scripts/bench_prep.py, each labelled by tree_parsing (for DESIGN.md
section 3p and the README).  Next to them, in the same run: the emit call alone between two events, branch_morphometry with and
without the section columns, and a torch composition of the same arithmetic -- the sample voxels of a chunk of points formed in
float64 and gathered in one batched index, then the flood fill as iterated masked max_pool2d (a 3 x 1 and a 1 x 3 window: the four
neighbours) to a fixed point -- from the tangents the call returns, so the composition does not pay for them.
One warm-up call each, then the median of five, wall clock around a synchronise.  No time here is a pass condition.

``--trace``: three calls per case and nothing else, for a kernel trace in a run of its own
(``rocprofv3 --kernel-trace --stats -- python scripts/bench_cross_section.py --trace``)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import seunet_amd as A
from seunet_amd import _lib
from skeleton_oracle import TREE_STAMPS

SHAPE, SCALE = (512, 512, 300), 2
SPACING = (1.0, 0.7, 0.7)
HALF = 31
CHUNK = 2048                                                 # points per batch of the torch composition
TRACE = "--trace" in sys.argv[1:]


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


def emit_ms(parsing, skel, num, step):
    """seunet_cross_section_emit alone: its two launches between two events, buffers preallocated, nothing copied back."""
    import ctypes as C
    lib = _lib.load()
    shape = tuple(parsing.shape)
    ws_bytes = int(lib.seunet_cross_section_workspace_bytes(*shape))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    m, status = C.c_longlong(0), C.c_int(0)
    _lib.check(lib.seunet_cross_section_count(parsing.data_ptr(), skel.data_ptr(), *shape, num, C.byref(m), C.byref(status),
                                              ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "cross_section_count")
    m = int(m.value)
    lin = torch.empty(m, dtype=torch.int32, device="cuda")
    tangent = torch.empty(3 * m, dtype=torch.float64, device="cuda")
    table = torch.empty(12 * m, dtype=torch.int32, device="cuda")
    times = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.seunet_cross_section_emit(parsing.data_ptr(), skel.data_ptr(), *shape, *SPACING, step, 4, 1, m, lin.data_ptr(),
                                                 tangent.data_ptr(), table.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()),
                   "cross_section_emit")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:])), m


def torch_sections(parsing, cs):
    """Counts of the sections by a torch composition of the same arithmetic, from the tangents of ``cs``."""
    dev = parsing.device
    s = torch.tensor(SPACING, dtype=torch.float64, device=dev)
    ext = torch.tensor(parsing.shape, dtype=torch.float64, device=dev)
    k = torch.arange(-HALF, HALF + 1, dtype=torch.float64, device=dev) * cs.step
    ih, jh = k[None, None, :, None], k[None, :, None, None]
    flat = parsing.reshape(-1)
    rows = np.flatnonzero(cs.support >= 3)
    counts = np.zeros(len(cs), np.int64)
    for at in range(0, rows.size, CHUNK):
        part = rows[at:at + CHUNK]
        t = torch.from_numpy(cs.tangent[part]).to(dev)
        coord = torch.from_numpy(cs.coord[part]).to(dev)
        label = torch.from_numpy(cs.label[part]).to(dev)
        a = t.abs().argmin(dim=1)
        w = torch.nn.functional.one_hot(a, 3).to(torch.float64) - t.gather(1, a[:, None]) * t
        u = w / w.square().sum(dim=1, keepdim=True).sqrt()
        v = torch.linalg.cross(t, u)
        x = (coord.to(torch.float64) * s)[:, None, None, :] + ih * u[:, None, None, :] + jh * v[:, None, None, :]
        f = torch.floor(x / s + 0.5)
        ok = ((f >= 0) & (f < ext)).all(dim=-1)
        vox = torch.where(ok[..., None], f, torch.zeros_like(f)).long()
        got = flat[(vox[..., 0] * parsing.shape[1] + vox[..., 1]) * parsing.shape[2] + vox[..., 2]]
        inside = (ok & (got == label[:, None, None])).to(torch.float32)[:, None]
        fill = torch.zeros_like(inside)
        fill[:, :, HALF, HALF] = inside[:, :, HALF, HALF]
        while True:
            grown = torch.maximum(torch.nn.functional.max_pool2d(fill, (3, 1), 1, (1, 0)),
                                  torch.nn.functional.max_pool2d(fill, (1, 3), 1, (0, 1))) * inside
            if torch.equal(grown, fill):
                break
            fill = grown
        counts[part] = fill.sum(dim=(1, 2, 3)).long().cpu().numpy()
    return counts


def report(rows):
    for what, t, lo, hi in rows:
        print("  %-62s median of 5 %9.3f ms (min %.3f, max %.3f)" % (what, t, lo, hi), flush=True)


def run(name, label, skel):
    parsing = A.tree_parsing(label, skel)
    num = int(parsing.max())
    if TRACE:
        for _ in range(3):
            A.cross_sections(parsing, skel, SPACING, num=num)
        torch.cuda.synchronize()
        return
    sqdist = A.distance_transform_edt(label, return_distances=False, return_sqdist=True)
    t_cs, lo_cs, hi_cs, cs = median_ms(lambda: A.cross_sections(parsing, skel, SPACING, num=num))
    t_emit, m = emit_ms(parsing, skel, num, cs.step)
    t_tab, lo_tab, hi_tab, plain = median_ms(lambda: A.branch_morphometry(parsing, skel, SPACING, num, sqdist))
    t_sec, lo_sec, hi_sec, table = median_ms(lambda: A.branch_morphometry(parsing, skel, SPACING, num, sqdist, cross_sections=True))
    t_torch, lo_torch, hi_torch, counts = median_ms(lambda: torch_sections(parsing, cs))
    assert m == len(cs)
    differ = int((counts != cs.count).sum())
    measured = table.section_count > 0
    print("cross sections %s %dx%dx%d, spacing %s, step %.2f: %d points of %d labels, %d valid, %d truncated (rim > 0), %d without a "
          "tangent; median area %.2f, median major / minor diameter %.2f / %.2f; %d of %d branches with a valid section; the torch "
          "composition's counts differ in %d rows"
          % ((name,) + tuple(label.shape) + (SPACING, cs.step, len(cs), num, int(cs.valid.sum()), int((cs.rim > 0).sum()),
                                              int((cs.support < 3).sum()), float(np.median(cs.area[cs.valid])),
                                              float(np.median(cs.diameter_major[cs.valid])), float(np.median(cs.diameter_minor[cs.valid])),
                                              int(measured.sum()), table.n_branches, differ)), flush=True)
    report((("cross_sections (columns on the host)", t_cs, lo_cs, hi_cs),
            ("branch_morphometry (skeleton and sqdist given)", t_tab, lo_tab, hi_tab),
            ("branch_morphometry(cross_sections=True)", t_sec, lo_sec, hi_sec),
            ("torch: batched gather + iterated masked max_pool2d", t_torch, lo_torch, hi_torch)))
    print("  seunet_cross_section_emit on the device alone (events): %.3f ms for %d points = %.1f ns per point, %.0f G samples/s"
          % (t_emit, m, 1e6 * t_emit / max(m, 1), 3969e-6 * m / t_emit), flush=True)


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


vol = np.zeros(SHAPE, dtype=bool)
for gi in range(3):
    for gj in range(3):
        off = (60 + 150 * gi, 60 + 150 * gj, 26)
        for a, b, r2 in TREE_STAMPS:
            stamp(vol, [SCALE * a[i] + off[i] for i in range(3)], [SCALE * b[i] + off[i] for i in range(3)], SCALE * SCALE * r2)
tall = torch.from_numpy(vol.view(np.uint8)).cuda()                       # (512, 512, 300): the trunks along axis 2, quick to thin
skel = A.skeletonize_3d(tall).permute(2, 0, 1).contiguous()             # any skeleton of the tree serves the labelling
label = tall.permute(2, 0, 1).contiguous()                              # (300, 512, 512)
run("tree", label, skel)
run("tubes", *synthetic_tubes((300, 512, 512)))
