"""Child process of tests/test_streams_gpu.py: the FIRST calls this process makes into the library are a marching weight gradient
and a 1x1x1 weight gradient, issued under a side stream behind a pending delay (tests/side_stream.py).  Those kernels pad through
the per-device page of zeros, which the library makes on first need: here that happens while a non-blocking stream is current.
The channels-last operands are laid out with torch (the library's own packing would be an earlier library call); the results are
compared with F.conv3d's weight gradient in float64 under the tolerance tests/test_ops_gpu.py uses for these calls.

Prints "first use OK" and exits 0 on success."""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from side_stream import run_behind_delay  # noqa: E402
from test_ops_gpu import assert_close, gen, rnd  # noqa: E402

SHAPES = [(2, 6, 9, 40), (1, 5, 8, 31)]
CASES = [([32, 32], 32, 27), ([32, 32], 32, 1)]          # (source split, cout, taps): csrc/wgrad_march.hip, csrc/wgrad_1x1.hip


def cl(t):
    """NCDHW f32 (already rounded to bf16 values) -> channels-last bf16, the layout seunet_pack_cl writes (C a multiple of 8)."""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16)


def inputs(off):
    out = []
    for n, d, h, w in SHAPES:
        x, dy = rnd("bf16", gen(n, 64, d, h, w, seed=12 + off)), rnd("bf16", gen(n, 32, d, h, w, seed=13 + off))
        out += [cl(x[:, :32]), cl(x[:, 32:]), cl(dy)]
    return out


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    from seunet_amd import _lib, ops
    _lib.load()

    def op(*t):
        out = []
        for i in range(len(SHAPES)):
            a, b, dy = t[3 * i:3 * i + 3]
            out.append([ops.conv3d_wgrad([a, b], dy, 64, cout, taps, 1, _lib.CONV_MARCH) for _, cout, taps in CASES])
        return out
    got = run_behind_delay(lambda: inputs(0), lambda: inputs(100), op, no_host_sync=False, label="first use")
    for i, (n, d, h, w) in enumerate(SHAPES):
        x, dy = rnd("bf16", gen(n, 64, d, h, w, seed=12)).double(), rnd("bf16", gen(n, 32, d, h, w, seed=13)).double()
        for j, (_, cout, taps) in enumerate(CASES):
            k = 3 if taps == 27 else 1
            wt = torch.zeros(cout, 64, k, k, k, dtype=torch.float64, requires_grad=True)
            F.conv3d(x, wt, padding=k // 2).backward(dy)
            assert_close(got[i][j], wt.grad, "fp32", f"first use: wgrad taps {taps} at {(n, d, h, w)}")
    print("first use OK")


if __name__ == "__main__":
    main()
