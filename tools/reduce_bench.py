#!/usr/bin/env python3
"""Time the flagship step's calls of the ops whose kernels mostly sum
(BatchNorm training forward and backward, the split-K sums behind linear_fwd,
the conv backward pairs and conv2d_wino, colsum, cross-entropy) at B=32 (GPU
box).

Each figure is us per call from a captured graph of CALLS back-to-back calls
(as the benchmark replays them: no launch overhead between kernels), median of
REPS replays; ROUNDS rounds show the round-to-round spread.  To compare two
commits, run this script from a checkout of each on one box, alternating.

  python tools/reduce_bench.py [--rounds N]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from split_learning_amd.ops.functional import native

B = 32
CALLS = 20
REPS = 15
# (C, H, pool): the BN blocks of VGG16/CIFAR10, H = W
BN_SHAPES = [(64, 32, False), (64, 32, True), (128, 16, False), (128, 16, True),
             (256, 8, False), (256, 8, True), (512, 4, False), (512, 4, True)]


def make_graph(fn):
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
    return g


def graph_us(g):
    ts = []
    for _ in range(REPS):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    return statistics.median(ts)


def cases(n):
    """(name, fn) per op call; fn's tensors stay alive in its closure."""
    out = []
    for (C, H, pool) in BN_SHAPES:
        x = torch.randn(B, C, H, H, device="cuda") * 1.5 + 0.3
        gamma = torch.rand(C, device="cuda") + 0.5
        beta = torch.randn(C, device="cuda") * 0.3
        rm = torch.zeros(C, device="cuda")
        rv = torch.ones(C, device="cuda")
        nbt = torch.zeros((), dtype=torch.long, device="cuda")
        Hg = H // 2 if pool else H
        gy = torch.randn(B, C, Hg, Hg, device="cuda")
        res = n.bn2d_train_fwd(x, gamma, beta, rm, rv, nbt, 0.1, 1e-5, True, pool)
        y, mean, invstd = res[:3]
        idx = res[3] if pool else None
        tag = f"{C}x{H}x{H}" + (" pool" if pool else "")
        out.append((f"bn fwd {tag}",
                    lambda x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, nbt=nbt,
                    pool=pool: n.bn2d_train_fwd(x, gamma, beta, rm, rv, nbt, 0.1,
                                                1e-5, True, pool)))
        out.append((f"bn bwd {tag}",
                    lambda x=x, gy=gy, gamma=gamma, mean=mean, invstd=invstd, y=y,
                    idx=idx: n.bn2d_train_bwd(x, gy, gamma, mean, invstd, y, idx)))
    xl = torch.randn(B, 4096, device="cuda")
    wl = torch.randn(10, 4096, device="cuda") * 0.02
    bl = torch.randn(10, device="cuda")
    out.append(("linear_fwd 4096->10", lambda: n.linear_fwd(xl, wl, bl)))
    for (C, H) in [(64, 32), (512, 4)]:
        gy = torch.randn(B, C, H, H, device="cuda")
        x = torch.randn(B, C, H, H, device="cuda")
        w = torch.randn(C, C, 3, 3, device="cuda") * 0.1
        out.append((f"conv2d_bwd {C}ch {H}x{H}",
                    lambda gy=gy, x=x, w=w: n.conv2d_bwd(gy, x, w, 1, 1, True, True)))
    x2 = torch.randn(B, 512, 2, 2, device="cuda")
    w2 = torch.randn(512, 512, 3, 3, device="cuda") * 0.1
    out.append(("conv2d_wino 512ch 2x2", lambda: n.conv2d_wino(x2, w2, None, 1, False)))
    g10 = torch.randn(B, 10, device="cuda")
    g4096 = torch.randn(B, 4096, device="cuda")
    out.append(("colsum 32x10", lambda: n.colsum_f32(g10)))
    out.append(("colsum 32x4096", lambda: n.colsum_f32(g4096)))
    logits = torch.randn(B, 10, device="cuda")
    labels = torch.randint(0, 10, (B,), device="cuda")
    out.append(("ce_fwd 32x10", lambda: n.ce_fwd(logits, labels)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    torch.manual_seed(3)
    cs = cases(native())
    graphs = [(name, make_graph(fn)) for name, fn in cs]
    totals = [0.0] * args.rounds
    rows = {name: [] for name, _ in cs}
    for r in range(args.rounds):
        for name, g in graphs:
            us = graph_us(g)
            rows[name].append(us)
            totals[r] += us
    for name, us in rows.items():
        print(f"{name:<26} " + "  ".join(f"{u:7.2f}" for u in us) + " us", flush=True)
    print(f"{'sum of the above':<26} " + "  ".join(f"{t:7.2f}" for t in totals)
          + " us", flush=True)


if __name__ == "__main__":
    main()
