#!/usr/bin/env python3
"""Time the conv backward (bwd-data + bwd-weight) of the flagship step's nine
paired layers at B=32 (GPU box), three ways in one process, alternating:

  separate     conv2d_bwd_data then conv2d_bwd_weight (two fused Winograd
               launches and up to two slab reduces)
  segregated   conv2d_bwd_pair, bwd-data blocks first, bwd-weight blocks behind
  interleaved  conv2d_bwd_pair, roles alternating by block index

Each figure is us per layer backward from a captured graph of CALLS
back-to-back calls (as the benchmark replays them: no launch overhead between
kernels), median of REPS replays; ROUNDS rounds show the round-to-round
spread.  The last line is the per-step total over the nine layers per round.

  python tools/conv_bwd_pair_bench.py [--rounds N]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from split_learning_amd.ops.functional import native

# (Ci, H, Co, layers per step): VGG16/CIFAR10 cut=7, 3x3 s1 p1, H = W
SHAPES = [(64, 32, 64, 1), (64, 16, 128, 1), (128, 16, 128, 1),
          (128, 8, 256, 1), (256, 8, 256, 2), (256, 4, 512, 1),
          (512, 4, 512, 2)]
B = 32
CALLS = 20
REPS = 15


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    n = native()
    torch.manual_seed(3)
    names = ("separate", "segregated", "interleaved")
    totals = [[0.0] * 3 for _ in range(args.rounds)]
    for (Ci, H, Co, layers) in SHAPES:
        gy = torch.randn(B, Co, H, H, device="cuda")
        x = torch.randn(B, Ci, H, H, device="cuda")
        w = torch.randn(Co, Ci, 3, 3, device="cuda") * 0.1
        assert n.conv_route("bwd_data", B, Ci, H, H, Co, 3, 1, 1) == "wino_fused"
        assert n.conv_route("bwd_weight", B, Ci, H, H, Co, 3, 1, 1) == "wino_bwdw_fused"

        def separate():
            n.conv2d_bwd_data(gy, w, 1, 1, H, H)
            n.conv2d_bwd_weight(gy, x, 3, 3, 1, 1)

        graphs = [make_graph(separate),
                  make_graph(lambda: n.conv2d_bwd_pair(gy, x, w, 1, 0)),
                  make_graph(lambda: n.conv2d_bwd_pair(gy, x, w, 1, 1))]
        ds, _, ws, _ = n.conv2d_bwd_pair_splits(B, Ci, H, H, Co, 1)
        for r in range(args.rounds):
            us = [graph_us(g) for g in graphs]     # alternating within a round
            for k in range(3):
                totals[r][k] += layers * us[k]
            print(f"{Ci:>3}->{Co:<3} {H:>2}x{H:<2} x{layers} splits {ds:>2}/{ws:<2} "
                  f"round {r}: " + "  ".join(f"{nm} {u:6.1f}" for nm, u in zip(names, us))
                  + " us", flush=True)
    for r in range(args.rounds):
        print(f"nine layers, round {r}: "
              + "  ".join(f"{nm} {t:7.1f}" for nm, t in zip(names, totals[r]))
              + " us/step", flush=True)


if __name__ == "__main__":
    main()
