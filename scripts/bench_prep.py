"""Device-event times of the stage-2/3 preparation (se-unet-airseg_amd/prep.py) on a synthetic tube-tree case, next to scipy
on the host when it is installed (--scipy).  The parse leg times the ATM'22 tree parsing (whole and per entry point) on the same
case; its yardstick is edt_dist_indices_ms of the same run.  Usage: python scripts/bench_prep.py [--shapes 300x512x512,600x512x512] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seunet_amd as A  # noqa: E402


def synthetic(shape, seed=3):
    """label = tubes around random segments, skeleton = their centre lines, pred = label with pieces missing."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    skel = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    hi = torch.tensor(shape, device="cuda")
    for _ in range(400):
        a, b = torch.rand(3, generator=g, device="cuda") * (hi - 1), torch.rand(3, generator=g, device="cuda") * (hi - 1)
        m = int((b - a).abs().max()) + 1
        t = torch.linspace(0, 1, m, device="cuda")[:, None]
        p = (a + (b - a) * t).round().long()
        skel[p[:, 0], p[:, 1], p[:, 2]] = 1
    lab = torch.nn.functional.max_pool3d(skel[None, None].float(), 5, 1, 2)[0, 0].to(torch.uint8)
    keep = (torch.rand(shape, generator=g, device="cuda") > 0.3).to(torch.uint8)
    pred = lab * torch.nn.functional.max_pool3d(keep[None, None].float(), 3, 1, 1)[0, 0].to(torch.uint8)
    return lab, skel, pred


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
    ap.add_argument("--shapes", default="300x512x512,600x512x512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scipy", action="store_true", help="also time scipy on the host (tens of seconds per case)")
    args = ap.parse_args()
    for s in args.shapes.split(","):
        shape = tuple(int(v) for v in s.split("x"))
        lab, skel, pred = synthetic(shape)
        inv = 1 - skel
        r = {"shape": list(shape), "label_voxels": int(lab.sum()), "skeleton_voxels": int(skel.sum())}
        r["edt_dist_ms"] = timed(lambda: A.distance_transform_edt(inv), args.reps)
        r["edt_dist_indices_ms"] = timed(lambda: A.distance_transform_edt(inv, return_indices=True), args.reps)
        r["candidates_ms"] = timed(lambda: A.hard_mining_candidates(lab, skel, pred), args.reps)
        r["lib_weight_ms"] = timed(lambda: A.lib_weight(lab), args.reps)
        r["break_weight_ms"] = timed(lambda: A.break_weight(lab, pred, skel), args.reps)
        # parse leg: the ATM'22 tree parsing, whole and per entry point; the yardstick is edt_dist_indices_ms above
        parse, cd, num0 = A.skeleton_parsing(skel)
        plain = A.tree_parsing_func(parse, lab, cd)
        counts, adj = A.prep._label_stats(plain, num0)
        lut, num, rounds = A.prep.refine_labels(counts, adj, num0)
        r["parse_branches"], r["parse_num"], r["parse_rounds"] = num0, num, rounds
        r["parse_tree_parsing_ms"] = timed(lambda: A.tree_parsing(lab, skel), args.reps)
        r["parse_skeleton_parsing_ms"] = timed(lambda: A.skeleton_parsing(skel), args.reps)
        r["parse_tree_parsing_func_ms"] = timed(lambda: A.tree_parsing_func(parse, lab, cd), args.reps)
        r["parse_label_adjacency_ms"] = timed(lambda: A.label_adjacency(plain, num0), args.reps)
        r["parse_relabel_ms"] = timed(lambda: A.relabel(plain, lut), args.reps)
        t = time.perf_counter(); A.prep.refine_labels(counts, adj, num0); r["parse_refine_host_ms"] = (time.perf_counter() - t) * 1e3
        r["parse_over_edt_indices"] = r["parse_tree_parsing_ms"] / r["edt_dist_indices_ms"]
        if args.scipy:
            try:
                import numpy as np
                from scipy import ndimage
            except ImportError:
                r["scipy"] = "not installed"
            else:
                lh = lab.cpu().numpy()
                t = time.perf_counter(); ndimage.distance_transform_edt(lh); r["scipy_edt_s"] = time.perf_counter() - t
                t = time.perf_counter(); ndimage.distance_transform_edt(1 - skel.cpu().numpy(), return_indices=True)
                r["scipy_edt_indices_s"] = time.perf_counter() - t
                t = time.perf_counter(); ndimage.convolve(lh.astype(np.float32), np.ones((7, 7, 7), np.float32), mode="mirror")
                r["scipy_box7_s"] = time.perf_counter() - t
                sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
                import parse_oracle
                t = time.perf_counter(); parse_oracle.tree_parsing(lh, skel.cpu().numpy()); r["parse_oracle_s"] = time.perf_counter() - t
        print(json.dumps(r), flush=True)
        del lab, skel, pred, inv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
