"""Device-event times of the CT preprocessing (se-unet-airseg_amd/preprocess.py) on a synthetic chest
CT made on the device (FOV padding, body, two textured lungs, a trachea), best of --reps.
Usage: python scripts/bench_preprocess.py [--shapes 300x512x512,600x512x512] [--reps 3]
A shape is (slices, rows, columns) as in scripts/bench_prep.py; the volume is laid out (rows, columns, slices), the
reference's orientation after its transposes."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seunet_amd as A  # noqa: E402
from seunet_amd import preprocess as P  # noqa: E402


def synthetic_ct(X, Y, Z):
    dev = torch.device("cuda")
    x = torch.arange(X, device=dev, dtype=torch.float32).view(X, 1, 1)
    y = torch.arange(Y, device=dev, dtype=torch.float32).view(1, Y, 1)
    z = torch.arange(Z, device=dev, dtype=torch.float32).view(1, 1, Z)
    cx, cy = X / 2, Y / 2
    f = 0.55 + 0.45 * torch.sin(math.pi * (z + 0.5) / Z)
    ct = torch.full((X, Y, Z), -1000, dtype=torch.int16, device=dev)
    ct = torch.where((((x - cx) / (0.45 * X)) ** 2 + ((y - cy) / (0.39 * Y)) ** 2 <= 1).expand(X, Y, Z), torch.tensor(40, dtype=torch.int16, device=dev), ct)
    tex = (-1000 + 2 * ((x + y + z).to(torch.int64) % 76)).to(torch.int16).expand(X, Y, Z)
    for side in (-1, 1):
        lung = (((x - 0.47 * X) / (0.23 * X)) / f) ** 2 + (((y - cy - side * 0.2 * Y) / (0.14 * Y)) / f) ** 2 <= 1
        ct = torch.where(lung, tex, ct)
    ct = torch.where(((x - 0.2 * X) ** 2 + (y - cy) ** 2 <= 64).expand(X, Y, Z), torch.tensor(-1000, dtype=torch.int16, device=dev), ct)
    ct = torch.where(((x - cx) ** 2 + (y - cy) ** 2 > (0.49 * X) ** 2).expand(X, Y, Z), torch.tensor(-2048, dtype=torch.int16, device=dev), ct)
    return ct.contiguous()


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
    args = ap.parse_args()
    for s in args.shapes.split(","):
        d, h, w = (int(v) for v in s.split("x"))
        ct = synthetic_ct(h, w, d)
        counts = P.value_counts(ct, P.HU_SHIFT)
        hist = P.histogram_from_counts(counts)
        aaa = P.padding_value(hist)
        cp = P._shift_clamp(ct, aaa)
        T = P.threshold_from_hist(P.histogram_from_counts(P.clamped_counts(counts, aaa)))
        L = P._get_l(cp, T, P.MIN_AREA)
        L1 = A.maximum_3d(L)
        x = P._combine(L, L1, 0)
        L2 = A.maximum_3d(x)
        mask = P._combine(L1, L2, 1)
        _, _, box = A.preprocess_ct(ct)
        r = {"shape": [h, w, d], "T": float(T), "aaa": float(aaa), "lung_voxels": int(mask.sum()), "box": box[:3].tolist()}
        r["value_counts_ms"] = timed(lambda: P.value_counts(ct, P.HU_SHIFT), args.reps)
        r["shift_clamp_ms"] = timed(lambda: P._shift_clamp(ct, aaa), args.reps)
        r["get_l_ms"] = timed(lambda: P._get_l(cp, T, P.MIN_AREA), args.reps)
        r["maximum_3d_x2_ms"] = timed(lambda: (A.maximum_3d(L), A.maximum_3d(x)), args.reps)
        r["box_crop_ms"] = timed(lambda: (P._crop(cp, box), P._crop(mask, P.crop_box(*P._mask_extent(mask), mask.shape))), args.reps)
        r["preprocess_ct_ms"] = timed(lambda: A.preprocess_ct(ct), args.reps)
        r["preprocess_ct_prediction_ms"] = timed(lambda: A.preprocess_ct(ct, mode="prediction"), args.reps)
        r["cut_mask_ms"] = timed(lambda: A.cut_mask(mask, box), args.reps)
        print(json.dumps(r), flush=True)
        del ct, cp, L, L1, L2, x, mask
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
