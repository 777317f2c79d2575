"""Timing of the component / Betti family (for DESIGN.md section 3o and the README) at 300 x 512 x 512: the prediction of
``oracle/components_oracle.synthetic_tree`` (a tree, 2 % specks, 15 % misses) and a 0.3-density noise volume.  All in one run:

1. ``label`` at connectivity 3 beside ``largest_component``, the existing user of the same union-find on the same volume;
2. ``euler_number`` alone, with the bytes of the packed volume over its time, beside the pack pass (``seunet_mask_bits``);
3. ``betti_error`` with patches 32 and 64 beside a Python loop of ``betti_numbers`` over the same tile crops (checked to agree);
4. for context only, scipy on the host: ``ndimage.label`` and the oracle's Euler number.
Every call between two events after one warm-up call (the host waits inside a call are part of what a caller pays), median of five
(of three for the tile loops) with min and max as the run-to-run spread.  No time here is a pass condition."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
import torch
import seunet_amd as A
from seunet_amd import _lib
import betti_oracle as bo
from components_oracle import synthetic_tree

SHAPE = (300, 512, 512)


def events_ms(call, reps=5):
    """(median, min, max, last result) of one call between two events, after one warm-up call."""
    times, out = [], None
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:])), min(times[1:]), max(times[1:]), out


def line(what, t):
    print("  %-52s median %10.3f ms (min %.3f, max %.3f)" % (what, t[0], t[1], t[2]), flush=True)


def tile_loop(mask, patch, connectivity=3):
    """The loop a user could write before: betti_numbers of every tile crop, raster tile order."""
    slices, _ = bo.tile_slices(mask.shape, (patch,) * 3)
    return np.array([A.betti_numbers(mask[s].contiguous(), connectivity) for s in slices], dtype=np.int32)


def run(name, host, other):
    v, w = torch.from_numpy(host).cuda(), torch.from_numpy(other).cuda()
    n = v.numel()
    words = SHAPE[0] * SHAPE[1] * ((SHAPE[2] + 63) // 64)
    print("%s %dx%dx%d: %d foreground voxels (%.1f %%)" % ((name,) + SHAPE + (int(v.sum()), 100.0 * float(v.sum()) / n)), flush=True)
    t_lc = events_ms(lambda: A.largest_component(v))
    t_lab = events_ms(lambda: A.label(v, 3, return_num=True))
    num = int(t_lab[3][1])
    t_tab = events_ms(lambda: A.label(v, 3, return_num=True, return_table=True))
    t_rm = events_ms(lambda: A.remove_small_objects(v, 50, 3))
    line("largest_component (26 neighbours)", t_lc)
    line("label, connectivity 3 (%d components)" % num, t_lab)
    line("label with the component table", t_tab)
    line("remove_small_objects(min_size=50)", t_rm)
    print("  ratio label / largest_component: %.2f" % (t_lab[0] / t_lc[0]), flush=True)
    bits = torch.empty(n // 64, dtype=torch.int64, device="cuda")
    lib = _lib.load()
    t_pack = events_ms(lambda: _lib.check(lib.seunet_mask_bits(v.data_ptr(), n, bits.data_ptr(), _lib.stream_ptr()), "mask_bits"))
    for c in (3, 1):
        t_e = events_ms(lambda: A.euler_number(v, c))
        line("euler_number, connectivity %d (chi = %d)" % (c, t_e[3]), t_e)
        print("    packed volume %.1f MB / time = %.1f GB/s; volume bytes + packed words / time = %.1f GB/s"
              % (words * 8 / 1e6, words * 8 / t_e[0] / 1e6, (n + 2 * words * 8) / t_e[0] / 1e6), flush=True)
    line("seunet_mask_bits (the pack pass alone)", t_pack)
    print("    volume bytes / time = %.1f GB/s" % (n / t_pack[0] / 1e6), flush=True)
    t_b = events_ms(lambda: A.betti_numbers(v, 3))
    line("betti_numbers, connectivity 3 %s" % (t_b[3],), t_b)
    for patch in (32, 64):
        t_all = events_ms(lambda: A.betti_error(v, w, patch, 3))
        t_loop = events_ms(lambda: (tile_loop(v, patch), tile_loop(w, patch)), reps=3)
        got = t_all[3]
        assert np.array_equal(got.pred.cpu().numpy(), t_loop[3][0]) and np.array_equal(got.label.cpu().numpy(), t_loop[3][1])
        tiles = got.tiles[0] * got.tiles[1] * got.tiles[2]
        line("betti_error, patch %d (%d tiles, error %s)" % (patch, tiles, np.round(got.error, 3)), t_all)
        line("loop of betti_numbers over the %d crops, both masks" % tiles, t_loop)
        print("    ratio loop / betti_error: %.1f (spread of betti_error %.1f %%, of the loop %.1f %%)"
              % (t_loop[0] / t_all[0], 100.0 * (t_all[2] - t_all[1]) / t_all[0], 100.0 * (t_loop[2] - t_loop[1]) / t_loop[0]), flush=True)
    return num


def host_context(name, host, num):
    t0 = time.perf_counter()
    got = bo.label(host, 3)[1]
    t1 = time.perf_counter()
    assert got == num, (got, num)
    print("  context only, scipy on the host: ndimage.label(%s, 26 neighbours) %.1f s" % (name, t1 - t0), flush=True)


t0 = time.perf_counter()
tree = np.ascontiguousarray(synthetic_tree(SHAPE, 11)[0])
noise = bo.noise(SHAPE, 0.3, 12)
print("(the two volumes made on the host in %.1f s)" % (time.perf_counter() - t0), flush=True)
n_tree = run("tree prediction", tree, noise)
n_noise = run("noise 0.3", noise, tree)
host_context("tree prediction", tree, n_tree)
host_context("noise 0.3", noise, n_noise)
t0 = time.perf_counter()
chi = bo.euler_number(tree, 3)
print("  context only, numpy on the host: the oracle's Euler number of the tree prediction (chi = %d) %.1f s" % (chi, time.perf_counter() - t0),
      flush=True)
assert chi == A.euler_number(tree, 3)
