"""Time the online-hard-mining step at the training shape (4 x 128^3) with device events on one GPU: the key pass
(``per_sample_loss``), ``OnlineHardPool.add`` with the pool full and every sample accepted, the scatter launch alone against a
device-to-device copy of the same bytes in the same process, and ``fused_stage_loss(2)`` forward as the yardstick.  Prints one
JSON line.  The figures of DESIGN.md 3f come from this script.

Usage: python scripts/bench_online_pool.py [--iters 50] [--limit 8]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seunet_amd as A  # noqa: E402
from seunet_amd import _lib  # noqa: E402


def timed(fn, iters, warmup=5):
    """Milliseconds per call: device events around ``iters`` back-to-back calls after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--limit", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, cube = 4, 128
    V = cube ** 3
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (B, 1, cube, cube, cube)
    pred_en = torch.randn(shape, device="cuda", generator=g) * 3
    pred_de = torch.randn(shape, device="cuda", generator=g) * 3
    label = (torch.rand(shape, device="cuda", generator=g) < 0.03).float()
    weight = 1 + torch.rand(shape, device="cuda", generator=g)
    data = torch.randn((B, 2, cube, cube, cube), device="cuda", generator=g)
    pool = A.OnlineHardPool(args.limit, cube=cube)
    step = [0]
    base = torch.arange(B, device="cuda", dtype=torch.float32)

    def rising_keys():                       # every key above everything stored: the pool stays full and every sample is accepted
        step[0] += 1
        return base + float(B * step[0])

    for _ in range(args.limit // B + 1):
        pool.add(rising_keys(), data, label, weight)
    assert len(pool) == args.limit
    lib = _lib.load()
    slots = torch.arange(B, device="cuda", dtype=torch.int32)

    def scatter_only():
        _lib.check(lib.seunet_pool_scatter(slots.data_ptr(), B, pool.limit, V, data.data_ptr(), label.data_ptr(), weight.data_ptr(), None,
                                           pool.data.data_ptr(), pool.label.data_ptr(), pool.weight.data_ptr(), None, _lib.stream_ptr()),
                   "pool_scatter")

    read_bytes, write_bytes = B * V * 16, B * V * 13        # in: data 8 + label 4 + weight 4 B/voxel; out: 8 + 1 + 4
    moved = read_bytes + write_bytes
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    out = {"shape": [B, cube], "limit": args.limit, "iters": args.iters}
    out["key_ms"] = timed(lambda: A.per_sample_loss(pred_de, label, weight, apply_sigmoid=True), args.iters)
    out["add_ms"] = timed(lambda: pool.add(rising_keys(), data, label, weight), args.iters)
    out["key_plus_add_ms"] = timed(lambda: pool.add(A.per_sample_loss(pred_de, label, weight, apply_sigmoid=True) + float(B * 10 ** 6 + step[0]),
                                                    data, label, weight), args.iters)
    out["stage2_loss_fwd_ms"] = timed(lambda: A.fused_stage_loss(2, pred_en, pred_de, label, weight), args.iters)
    # scatter and the copy alternate, three rounds, so that neither owns a quieter moment of a shared machine
    sc, cp = [], []
    for _ in range(3):
        sc.append(timed(scatter_only, args.iters))
        cp.append(timed(lambda: dst.copy_(src), args.iters))
    out["scatter_ms"], out["copy_ms"] = min(sc), min(cp)
    out["scatter_ms_all"], out["copy_ms_all"] = sc, cp
    out["bytes_moved"] = moved
    out["scatter_GBps"] = moved / out["scatter_ms"] / 1e6
    out["copy_GBps"] = moved / out["copy_ms"] / 1e6
    out["scatter_over_copy"] = out["copy_ms"] / out["scatter_ms"]
    assert len(pool) == args.limit
    print(json.dumps(out))


if __name__ == "__main__":
    main()
