"""soft_cldice_loss forward + backward against the same arithmetic as a torch composition, on the GPU, in one run.

    python scripts/bench_cldice.py [--batch 4] [--size 128] [--iters 3] [--reps 20] [--warmup 5] [--step-ms 14.5]

Times ``seunet_amd.soft_cldice_loss(p, t, iters)`` + ``backward()`` with device events and, alternating with it call by call on
the same tensors, statement (a) of tests/cldice_oracle.py (the usual max_pool3d composition under autograd) run with torch's own
ops on the GPU in float32.  Prints both medians, their ratio, the fused time as a share of ``--step-ms`` (the training step the
loss would be added to) and the achieved bytes/s of the fused path from a byte count computed from the shapes: every tensor a
launch must read or write once, halo re-reads not counted.  One JSON line at the end.  Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def min_bytes(n, iters):
    """bytes the fused path must move for n voxels (float32 volumes 4n, choice bytes n)"""
    k = iters + 1
    fwd_pred = k * (4 + 4 + 4 + 1) * n + iters * 8 * n          # read E_j, write S_j, d_j, choices; read S_{j-1}, write E_{j+1}
    fwd_target = k * 8 * n + iters * 8 * n                      # read E_j, write S_j; read S_{j-1}, write E_{j+1}
    sums = 16 * n
    chain = 4 * n + k * 8 * n + iters * 4 * n                   # read t, d_j, S_{j-1}; write a_j
    stencil = k * 9 * n + iters * 4 * n + 4 * n                 # read a_j, choices, write gE; read gE; read S(t) once
    return fwd_pred + fwd_target + sums + chain + stencil


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=14.5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cldice: needs a GPU")
    import seunet_amd as A
    import cldice_oracle as O

    shape = (args.batch, 1, args.size, args.size, args.size)
    g = torch.Generator().manual_seed(0)
    t = (torch.rand(shape, generator=g) < 0.03).float()
    t = (torch.nn.functional.max_pool3d(t, 3, 1, 1) > 0).float().cuda()
    p = (0.7 * torch.nn.functional.avg_pool3d(t, 3, 1, 1) + 0.3 * torch.rand(shape, generator=g).cuda()).clamp(0, 1).contiguous()

    def fused():
        x = p.detach().requires_grad_(True)
        loss = A.soft_cldice_loss(x, t, args.iters)
        loss.backward()
        return loss.detach(), x.grad

    def composed():
        x = p.detach().requires_grad_(True)
        sp = O.soft_skeleton_a(x, args.iters)
        with torch.no_grad():
            st = O.soft_skeleton_a(t, args.iters)
        loss = O.value_from_sums((sp * t).sum(), sp.sum(), (st * x).sum(), st.sum(), 1.0)
        loss.backward()
        return loss.detach(), x.grad

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    for _ in range(args.warmup):
        fused(), composed()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(args.reps):                  # alternate, so that clocks and cache state drift over both alike
        ms, (lf, gf) = timed(fused)
        tf.append(ms)
        ms, (lc, gc) = timed(composed)
        tc.append(ms)
    fused_ms, composed_ms = statistics.median(tf), statistics.median(tc)
    n = p.numel()
    nbytes = min_bytes(n, args.iters)
    rel = float((gf - gc).abs().max() / gc.abs().max())
    out = {"shape": list(shape), "iters": args.iters, "fused_ms": round(fused_ms, 4), "fused_min_ms": round(min(tf), 4),
           "composed_ms": round(composed_ms, 4), "composed_min_ms": round(min(tc), 4), "ratio": round(composed_ms / fused_ms, 2),
           "share_of_step": round(fused_ms / args.step_ms, 4), "step_ms": args.step_ms, "min_bytes": nbytes,
           "achieved_TBps": round(nbytes / (fused_ms * 1e-3) / 1e12, 3), "loss_fused": float(lf), "loss_composed": float(lc),
           "grad_rel_diff": rel, "reps": args.reps, "warmup": args.warmup}
    print(f"fused {fused_ms:.3f} ms (min {min(tf):.3f}), torch composition {composed_ms:.3f} ms (min {min(tc):.3f}), "
          f"ratio {composed_ms / fused_ms:.2f}x, {100 * fused_ms / args.step_ms:.1f} % of a {args.step_ms} ms step, "
          f"{nbytes / 1e9:.2f} GB at {nbytes / (fused_ms * 1e-3) / 1e12:.2f} TB/s")
    print(json.dumps(out))
    if composed_ms < 3 * fused_ms:
        sys.exit("bench_cldice: the fused path is less than 3x faster than the torch composition")


if __name__ == "__main__":
    main()
