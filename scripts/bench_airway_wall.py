"""Timing of the airway wall measurement (seunet_amd.airway_walls) on the two cases of scripts/bench_cross_section.py: the synthetic
airway-like tree laid out as 300 x 512 x 512 and the tube case, each labelled by tree_parsing, spacing (1.0, 0.7, 0.7), with a CT
painted from the mask: lumen -1000, a wall shell of 50 where the EDT of the background is at most 1.5, parenchyma -850 (int16; for
DESIGN.md section 3q and the README).  Next to the whole call, in the same run: the ray kernel alone between two events,
cross_sections on the same volume, and a torch composition of the same arithmetic -- the sample positions of a chunk of points in
float64, the eight corners and the label of every sample gathered in batched indices, the rules as masked argmax / cummax-style
reductions over the profile -- from the sections the call is given, which must agree with the kernel on every ray code.
One warm-up call each, then the median of five, wall clock around a synchronise.  No time here is a pass condition.

``--trace``: three calls per case and nothing else, for a kernel trace in a run of its own
(``rocprofv3 --kernel-trace --stats -- python scripts/bench_airway_wall.py --trace``)."""
import ctypes as C
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
WALL = 1.5
RAYS = SAMPLES = 64
CHUNK = 512                                                  # points per batch of the torch composition
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


def rows_of(cs):
    """The sections' rows as the device buffers the kernel reads: (table int32[m, 12], tangent float64[m, 3])."""
    table = np.zeros((len(cs), 12), np.int32)
    table[:, 0:3], table[:, 3], table[:, 4], table[:, 5], table[:, 6:11], table[:, 11] = cs.coord, cs.label, cs.support, cs.count, cs.moments, cs.rim
    return torch.from_numpy(table).cuda(), torch.from_numpy(cs.tangent).cuda()


def kernel_ms(ct, parsing, cs, walls):
    """seunet_airway_walls alone: its one launch between two events, buffers preallocated, nothing copied back."""
    lib = _lib.load()
    m = len(cs)
    table, tangent = rows_of(cs)
    mask = torch.empty(m, dtype=torch.int64, device="cuda")
    sums = torch.empty(6 * m, dtype=torch.float64, device="cuda")
    times = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.seunet_airway_walls(ct.data_ptr(), 0, parsing.data_ptr(), *parsing.shape, *SPACING, cs.step, walls.ray_step,
                                           walls.n_search, walls.min_contrast, 1, m, table.data_ptr(), tangent.data_ptr(), mask.data_ptr(),
                                           sums.data_ptr(), None, None, _lib.stream_ptr()), "airway_walls")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:]))


def directions():
    out = (C.c_double * 128)()
    _lib.check(_lib.load().seunet_airway_wall_directions(out), "airway_wall_directions")
    return torch.tensor(list(out), dtype=torch.float64, device="cuda").reshape(RAYS, 2)


def take(a, k):
    return a.gather(-1, k.clamp(0, SAMPLES - 1)[..., None])[..., 0]


def torch_walls(ct, parsing, cs, walls, table, tangent, d):
    """The ray codes by a torch composition of the same arithmetic, from the rows of ``cs``: (uint8[m, 64], the samples the rays
    need: min(L, k_b + 2 n + 2) for a ray with a boundary, summed over all rays)."""
    dev = parsing.device
    s = torch.tensor(SPACING, dtype=torch.float64, device=dev)
    top = torch.tensor(parsing.shape, dtype=torch.float64, device=dev) - 2.0
    n1, n2 = parsing.shape[1], parsing.shape[2]
    n, c = walls.n_search, torch.tensor(walls.min_contrast, dtype=torch.float32, device=dev)
    K = torch.arange(SAMPLES, device=dev)
    rho = K.to(torch.float64) * walls.ray_step
    flat_ct, flat_p = ct.reshape(-1), parsing.reshape(-1)
    codes = torch.full((len(cs), RAYS), 6, dtype=torch.uint8, device=dev)
    needed = torch.zeros((), dtype=torch.int64, device=dev)
    rows = torch.nonzero((table[:, 5] != 0) & (table[:, 11] <= 0))[:, 0]
    for at in range(0, rows.numel(), CHUNK):
        part = rows[at:at + CHUNK]
        t, tab = tangent[part], table[part]
        a = t.abs().argmin(dim=1)
        w = torch.nn.functional.one_hot(a, 3).to(torch.float64) - t.gather(1, a[:, None]) * t
        u = w / torch.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])[:, None]      # one operation at a time, as the kernel
        v = torch.stack([t[:, 1] * u[:, 2] - t[:, 2] * u[:, 1], t[:, 2] * u[:, 0] - t[:, 0] * u[:, 2], t[:, 0] * u[:, 1] - t[:, 1] * u[:, 0]], dim=1)
        count = tab[:, 5].to(torch.float64)
        cih, cjh = (tab[:, 6].to(torch.float64) / count * cs.step)[:, None], (tab[:, 7].to(torch.float64) / count * cs.step)[:, None]
        o = (tab[:, 0:3].to(torch.float64) * s + cih * u) + cjh * v
        e = d[None, :, 0, None] * u[:, None, :] + d[None, :, 1, None] * v[:, None, :]
        g = (o[:, None, None, :] + rho[None, None, :, None] * e[:, :, None, :]) / s
        f = torch.floor(g)
        usable = ((f >= 0) & (f <= top)).all(dim=-1)
        L = torch.where(usable.all(dim=-1), SAMPLES, usable.to(torch.uint8).argmin(dim=-1))
        wgt = (g - f).to(torch.float32)
        fi = torch.where(usable[..., None], f, torch.zeros_like(f)).long()
        base = (fi[..., 0] * n1 + fi[..., 1]) * n2 + fi[..., 2]
        one = usable.long()
        corner = [flat_ct[base + one * ((b >> 2 & 1) * n1 * n2 + (b >> 1 & 1) * n2 + (b & 1))].to(torch.float32) for b in range(8)]
        c00, c01 = corner[0] + wgt[..., 2] * (corner[1] - corner[0]), corner[2] + wgt[..., 2] * (corner[3] - corner[2])
        c10, c11 = corner[4] + wgt[..., 2] * (corner[5] - corner[4]), corner[6] + wgt[..., 2] * (corner[7] - corner[6])
        c0, c1 = c00 + wgt[..., 1] * (c01 - c00), c10 + wgt[..., 1] * (c11 - c10)
        P = c0 + wgt[..., 0] * (c1 - c0)
        near = torch.where(usable[..., None], torch.floor(g + 0.5), torch.zeros_like(g)).long()
        got = flat_p[(near[..., 0] * n1 + near[..., 1]) * n2 + near[..., 2]]
        nonzero = usable & (got != 0)
        inside = usable & (got == tab[:, 3][:, None, None])
        outside = ~inside & (K < L[..., None]) & (K >= 1)
        bounded = (L > 0) & inside[..., 0] & outside.any(dim=-1)
        kb = outside.to(torch.uint8).argmax(dim=-1)
        lo, hi = (kb - 1).clamp(min=0), torch.minimum(kb + n, L - 1)
        Pw = torch.where((K >= lo[..., None]) & (K <= hi[..., None]), P, torch.full_like(P, -torch.inf))
        Pp = Pw.max(dim=-1).values
        kp = (Pw == Pp[..., None]).to(torch.uint8).argmax(dim=-1)          # the first of the maxima
        fail2 = (kp + 1 >= L) | ((kp == hi) & (take(P, kp + 1) >= Pp))
        Pl = torch.where(K <= kp[..., None], P, torch.full_like(P, torch.inf)).min(dim=-1).values
        fail3 = (Pp - Pl) < c
        stop = torch.minimum(kp + n, L - 1)
        falls = torch.zeros_like(usable)
        falls[..., :-1] = P[..., 1:] <= P[..., :-1]
        stays = (K >= kp[..., None]) & ~((K < stop[..., None]) & falls)
        ko = stays.to(torch.uint8).argmax(dim=-1)
        fail4 = (nonzero & (K >= kb[..., None]) & (K <= ko[..., None])).any(dim=-1)
        fail5 = (Pp - take(P, ko)) < c
        code = torch.where(~bounded, 1, torch.where(fail2, 2, torch.where(fail3, 3, torch.where(fail4, 4, torch.where(fail5, 5, 0)))))
        codes[part] = code.to(torch.uint8)
        needed += torch.where(bounded, torch.minimum(L, kb + 2 * n + 2), torch.zeros_like(L)).sum()
    return codes.cpu().numpy(), int(needed)


def report(rows):
    for what, t, lo, hi in rows:
        print("  %-62s median of 5 %9.3f ms (min %.3f, max %.3f)" % (what, t, lo, hi), flush=True)


def run(name, label, skel):
    parsing = A.tree_parsing(label, skel)
    num = int(parsing.max())
    away = A.distance_transform_edt((label == 0).to(torch.uint8), sampling=SPACING)
    ct = torch.where(label != 0, -1000, torch.where(away <= WALL, 50, -850)).to(torch.int16).contiguous()
    del away
    cs = A.cross_sections(parsing, skel, SPACING, num=num)
    if TRACE:
        for _ in range(3):
            A.airway_walls(ct, parsing, None, SPACING, sections=cs)
        torch.cuda.synchronize()
        return
    t_cs, lo_cs, hi_cs, _ = median_ms(lambda: A.cross_sections(parsing, skel, SPACING, num=num))
    t_w, lo_w, hi_w, walls = median_ms(lambda: A.airway_walls(ct, parsing, None, SPACING, sections=cs))
    t_all, lo_all, hi_all, _ = median_ms(lambda: A.airway_walls(ct, parsing, skel, SPACING))
    t_rays, lo_rays, hi_rays, rays = median_ms(lambda: A.airway_walls(ct, parsing, None, SPACING, sections=cs, return_rays=True))
    t_kernel = kernel_ms(ct, parsing, cs, walls)
    table, tangent = rows_of(cs)
    d = directions()
    t_torch, lo_torch, hi_torch, (codes, needed) = median_ms(lambda: torch_walls(ct, parsing, cs, walls, table, tangent, d))
    differ = int((codes != rays.codes).sum())
    m = len(cs)
    hist = np.bincount(rays.codes.reshape(-1), minlength=7)
    rows = walls.per_branch()
    fit = walls.pi10()
    print("airway walls %s %dx%dx%d, spacing %s, ray step %.2f, n_search %d: %d points of %d labels, %d valid (>= %d rays); rays by code "
          "0..6 %s; median thickness %.3f (painted %.1f), median WA%% %.1f; %d of %d branches with a valid row; Pi10 %.3f over %d "
          "branches; the torch composition's codes differ in %d of %d rays"
          % ((name,) + tuple(label.shape) + (SPACING, walls.ray_step, walls.n_search, m, num, int(walls.valid.sum()), walls.min_rays,
                                              hist.tolist(), float(np.nanmedian(walls.wall_thickness)), WALL,
                                              float(np.nanmedian(walls.wall_area_percent)), int((rows["wall_sections"] > 0).sum()), num,
                                              fit["pi10"], fit["branches"], differ, codes.size)), flush=True)
    report((("cross_sections (columns on the host)", t_cs, lo_cs, hi_cs),
            ("airway_walls, sections given (upload, kernel, copy back)", t_w, lo_w, hi_w),
            ("airway_walls, sections given, return_rays=True", t_rays, lo_rays, hi_rays),
            ("airway_walls, sections computed from the skeleton", t_all, lo_all, hi_all),
            ("torch: batched gathers + masked reductions over the profile", t_torch, lo_torch, hi_torch)))
    # a sample the rules can ask for costs one label gather and eight corner gathers; the kernel issues more: whole groups, up to
    # the longest ray of the wave, and the label gathers of the samples before a boundary is known
    measured = int(((table[:, 5] != 0) & (table[:, 11] <= 0)).sum().item())
    print("  seunet_airway_walls on the device alone (events): %.3f ms for %d points (%d measured) = %.1f ns per point; %d samples needed "
          "(%.1f per ray of a measured point) = %.1f G gathers/s at 9 gathers per needed sample"
          % (t_kernel, m, measured, 1e6 * t_kernel / max(m, 1), needed, needed / max(64 * measured, 1), 9e-6 * needed / t_kernel), flush=True)
    return differ


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
differ = run("tree", label, skel)
differ = run("tubes", *synthetic_tubes((300, 512, 512))) or differ
assert not differ, "the torch composition and the kernel disagree on a ray code"
