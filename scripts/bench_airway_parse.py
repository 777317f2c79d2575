"""Device-event times of prep.airway_parse and of its stages on a synthetic airway-like tree at 300 x 512 x 512:
the `tree` volume of tests/skeleton_oracle.py with every coordinate tripled and every squared radius multiplied by nine (the
random-segment case of scripts/bench_prep.py has no trunk the parser could orient itself by).  One warm-up call, then the minimum
of three.  The yardstick, measured in the same run, is maximum_3d + skeletonize_3d + tree_parsing_func on the same volume: the
dense stages the call cannot avoid.  Prints one JSON line.  Usage: python scripts/bench_airway_parse.py [--reps 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import seunet_amd as A  # noqa: E402
from seunet_amd import prep, topology  # noqa: E402
from skeleton_oracle import TREE_STAMPS  # noqa: E402

SHAPE, SCALE, OFFSET = (300, 512, 512), 3, (120, 200, 50)


def tree_volume():
    vol = np.zeros(SHAPE, dtype=bool)
    for a, b, r2 in TREE_STAMPS:
        a = [SCALE * a[i] + OFFSET[i] for i in range(3)]
        b = [SCALE * b[i] + OFFSET[i] for i in range(3)]
        r2 = SCALE * SCALE * r2
        n = max(abs(b[i] - a[i]) for i in range(3))
        r = int(np.sqrt(r2)) + 1
        o = np.arange(-r, r + 1)
        ball = (o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) <= r2
        for t in range(n + 1):
            p = [a[i] + ((b[i] - a[i]) * t) // n for i in range(3)]
            vol[p[0] - r:p[0] + r + 1, p[1] - r:p[1] + r + 1, p[2] - r:p[2] + r + 1] |= ball       # the offset keeps every ball inside
    return vol


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    label = torch.from_numpy(tree_volume().view(np.uint8)).cuda()
    st = prep.airway_parse_stages(label)
    r = {"shape": list(SHAPE), "label_voxels": int(label.sum()), "skeleton_voxels": int(st["skeleton"].sum()), "order": st["order"],
         "mainpart": st["mainpart"], "branches_before_merging": len(st["table1"]), "branches": len(st["merged"])}
    dilated = A.binary_dilation(label)
    filled = A.binary_fill_holes(dilated)
    closed = A.binary_closing(filled)
    lt, skel, cd, parse = st["label_trans"], st["skeleton"], st["cd"], st["skeleton_parse"]
    r["airway_parse_ms"] = timed(lambda: A.airway_parse(label), args.reps)
    r["orientation_ms"] = timed(lambda: [prep._mask_extent(label), prep._largest_in_slice(label, 100), prep._largest_in_slice(label, 400)],
                                args.reps)
    r["morphology_ms"] = timed(lambda: (A.binary_dilation(label), A.binary_closing(filled)), args.reps)
    r["fill_ms"] = timed(lambda: A.binary_fill_holes(dilated), args.reps)
    r["maximum_3d_ms"] = timed(lambda: A.maximum_3d(closed), args.reps)
    r["skeleton_ms"] = timed(lambda: A.skeletonize_3d(lt), args.reps)
    r["assign_ms"] = timed(lambda: A.tree_parsing_func(parse, label, cd), args.reps)

    def host_stage():
        coords = prep._mask_coords(skel)
        ext = prep._mask_extent(lt)
        merged, _ = topology.graph_stage(coords, SHAPE, st["order"], (ext[4], ext[5]), lambda k: prep.slice_moments(lt, k))
        lin, val = topology.branch_labels(merged, SHAPE)
        prep.scatter_labels(lin, val, SHAPE)
    host_stage()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t = time.perf_counter(); host_stage(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
    r["graph_stage_host_ms"] = min(ts)            # wall clock: skeleton download, graph stage, the two moment reads, the scatter
    r["yardstick_ms"] = r["maximum_3d_ms"] + r["skeleton_ms"] + r["assign_ms"]
    r["airway_parse_over_yardstick"] = r["airway_parse_ms"] / r["yardstick_ms"]
    r["host_share"] = r["graph_stage_host_ms"] / r["airway_parse_ms"]
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
