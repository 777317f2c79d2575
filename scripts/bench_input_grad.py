"""Cost of the opt-in input gradient (SE_UNet(input_grad=True)) at the benchmark shape.

For bf16 and fp16 at B x 2 x S^3 (default 4 x 2 x 128^3): times forward + stage-1 loss + backward with the input gradient off
(x does not require grad) and on (x.requires_grad), with device events around each step, after warm-up; reports the median of
N steps and the difference, then one step's `input_grad:*` launch groups from seunet_prof_report.
Usage: python scripts/bench_input_grad.py [--batch 4] [--size 128] [--steps 20] [--warmup 5] [--dtypes bf16,fp16]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch

import seunet_amd as A
import seunet_oracle as orc
from seunet_amd import _lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,fp16")
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    b = orc.synthetic_batch(args.batch, (args.size,) * 3, 2, seed=0)
    x0, lab = b["image"].cuda(), b["label"].cuda()
    results = []
    for dtype in args.dtypes.split(","):
        m = A.SE_UNet(in_channel=2, act_dtype=dtype, input_grad=True)
        m.load_state_dict(orc.deterministic_state_dict(2, 1, 1, seed=0))
        m = m.cuda().train()

        def step(on):
            x = x0.clone().requires_grad_(on)
            for p in m.parameters():
                p.grad = None
            e, d = m(x)
            A.fused_stage_loss(1, e, d, lab).backward()
            return x

        def timed(on):
            for _ in range(args.warmup):
                step(on)
            ms = []
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(on)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return statistics.median(ms)

        # alternate off / on twice so that a drift of the clock does not land on one side only
        off1, on1 = timed(False), timed(True)
        on2, off2 = timed(True), timed(False)
        off, on = min(off1, off2), min(on1, on2)
        torch.cuda.synchronize()
        lib.seunet_prof_enable_filtered(b"input_grad:")
        step(True)
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 16)
        lib.seunet_prof_report(buf, len(buf))
        lib.seunet_prof_enable(0)
        groups = {}
        for line in buf.value.decode().splitlines():
            parts = line.split("\t")
            if len(parts) >= 2 and parts[0].startswith("input_grad:"):
                groups[parts[0]] = float(parts[1])
        r = {"dtype": dtype, "shape": [args.batch, 2, args.size, args.size, args.size], "step_ms_off": round(off, 3),
             "step_ms_on": round(on, 3), "added_ms": round(on - off, 3), "medians_off": [round(off1, 3), round(off2, 3)],
             "medians_on": [round(on1, 3), round(on2, 3)], "input_grad_groups_ms": {k: round(v, 4) for k, v in groups.items()}}
        results.append(r)
        print(json.dumps(r), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
