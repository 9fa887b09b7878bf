#!/usr/bin/env python3
"""Time conv2d_wino, forward and bwd-data (flip), at the flagship step's three
Wino-routed shapes (GPU box): the three-launch pipeline (weight and input
transform in one launch, the frequency GEMM, slab sum in the output transform).

  python tools/wino_pipe_bench.py

Each figure is us per call from a captured graph of CALLS back-to-back calls
(as the benchmark replays them: no launch overhead between kernels), best and
median of REPS replays.
"""

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from split_learning_amd.ops.functional import native

# (B, C, H, W): Ci = Co = C, pad 1
SHAPES = [(32, 256, 8, 8), (32, 512, 4, 4), (32, 512, 2, 2)]
CALLS = 20
REPS = 15


def graph_us(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    return min(ts), statistics.median(ts)


def main():
    n = native()
    torch.manual_seed(3)
    for (B, C, H, W) in SHAPES:
        x = torch.randn(B, C, H, W, device="cuda")
        w = torch.randn(C, C, 3, 3, device="cuda") * 0.1
        bias = torch.randn(C, device="cuda")
        fb, fm = graph_us(lambda: n.conv2d_wino(x, w, bias, 1, False))
        bb, bm = graph_us(lambda: n.conv2d_wino(x, w, None, 1, True))
        print(f"pipe {B}x{C}x{H}x{W}: fwd best {fb:6.1f} med {fm:6.1f}"
              f"  flip best {bb:6.1f} med {bm:6.1f} us/call", flush=True)


if __name__ == "__main__":
    main()
