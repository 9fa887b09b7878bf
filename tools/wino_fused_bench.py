#!/usr/bin/env python3
"""Fused-Winograd kernels at the routed flagship shapes (run on the GPU box).

Calls the exposed `conv2d_wino_fused` / `conv2d_wino_bwdw_fused` ops on every
(shape, direction) pair that conv_route.h sends to them in the VGG16/CIFAR10
batch-32 step.

  python tools/wino_fused_bench.py              # us per call, per pair
  python tools/wino_fused_bench.py --loop N     # every pair N times, bare:
                                                # the rocprofv3 --pmc target
  python tools/wino_fused_bench.py --pmc-csv counter_collection.csv
      # per-kernel sums of a --pmc run's counters + the derived ratios

The per-call time is the whole op (slab_reduce included where the op splits),
as the training step pays it.
"""

import argparse
import csv
import os
import sys
import time
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# forward shapes (B, Ci, H, W, Co), pad 1, and the directions routed fused
ROUTED = [
    ((32, 64, 32, 32, 64), ("fwd", "bwdd", "bwdw")),
    ((32, 64, 16, 16, 128), ("fwd", "bwdd", "bwdw")),
    ((32, 128, 16, 16, 128), ("fwd", "bwdd", "bwdw")),
    ((32, 128, 8, 8, 256), ("bwdd", "bwdw")),
    ((32, 256, 8, 8, 256), ("bwdd", "bwdw")),
    ((32, 256, 4, 4, 512), ("bwdd", "bwdw")),
    ((32, 512, 4, 4, 512), ("bwdd", "bwdw")),
    ((32, 512, 2, 2, 512), ("bwdw",)),
]

KERNELS = ("wino_fused_kernel<false>", "wino_fused_kernel<true>",
           "wino_bwdw_fused_kernel")


def make_calls(dev):
    import torch
    from split_learning_amd.ops.functional import native
    n = native()
    gen = torch.Generator(device="cpu").manual_seed(0)
    calls = []
    for (B, Ci, H, W, Co), dirs in ROUTED:
        x = torch.randn(B, Ci, H, W, generator=gen).to(dev)
        w = (torch.randn(Co, Ci, 3, 3, generator=gen) * 0.1).to(dev)
        gy = torch.randn(B, Co, H, W, generator=gen).to(dev)
        name = f"{B}x{Ci}x{H}x{W}->{Co}"
        for d in dirs:
            if d == "fwd":
                fn = lambda x=x, w=w: n.conv2d_wino_fused(x, w, None, 1, False)
            elif d == "bwdd":
                fn = lambda gy=gy, w=w: n.conv2d_wino_fused(gy, w, None, 1, True)
            else:
                fn = lambda gy=gy, x=x: n.conv2d_wino_bwdw_fused(gy, x, 1)
            calls.append((name, d, fn))
    return calls


def timed(fn, iters, warmup=10):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def pmc_summary(path):
    sums = defaultdict(lambda: defaultdict(float))
    calls = defaultdict(set)
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            kname = row["Kernel_Name"]
            key = next((k for k in KERNELS if k in kname), None)
            if key is None:
                continue
            sums[key][row["Counter_Name"]] += float(row["Counter_Value"])
            calls[key].add(row["Dispatch_Id"])
    for key in KERNELS:
        c = sums.get(key)
        if not c:
            continue
        print(f"{key}: {len(calls[key])} dispatches")
        for name in sorted(c):
            print(f"  {name:28s} {c[name]:16.0f}")

        def ratio(a, b):
            return c[a] / c[b] if c.get(b) else float("nan")
        print(f"  LDS_BANK_CONFLICT / LDS_IDX_ACTIVE   "
              f"{ratio('SQ_LDS_BANK_CONFLICT', 'SQ_LDS_IDX_ACTIVE'):.3f}")
        print(f"  WAIT_ANY / WAVE_CYCLES (parked)      "
              f"{ratio('SQ_WAIT_ANY', 'SQ_WAVE_CYCLES'):.3f}")
        print(f"  WAIT_INST_ANY / WAVE_CYCLES (issue)  "
              f"{ratio('SQ_WAIT_INST_ANY', 'SQ_WAVE_CYCLES'):.3f}")
        print(f"  ACTIVE_INST_ANY / WAVE_CYCLES        "
              f"{ratio('SQ_ACTIVE_INST_ANY', 'SQ_WAVE_CYCLES'):.3f}")
        # MFMA busy is counted per SIMD in cycles, BUSY_CYCLES per shader
        # engine: the share is only comparable between two runs of this tool
        print(f"  VALU_MFMA_BUSY_CYCLES / BUSY_CYCLES  "
              f"{ratio('SQ_VALU_MFMA_BUSY_CYCLES', 'SQ_BUSY_CYCLES'):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pmc-csv", default=None)
    args = ap.parse_args()
    if args.pmc_csv:
        pmc_summary(args.pmc_csv)
        return
    import torch
    dev = torch.device("cuda:0")
    calls = make_calls(dev)
    if args.loop:
        for _, _, fn in calls:
            for _ in range(args.loop):
                fn()
        torch.cuda.synchronize()
        return
    print(f"{'shape':>20} {'dir':>5} {'us/call':>9}")
    tot = defaultdict(float)
    for name, d, fn in calls:
        us = timed(fn, args.iters)
        tot[d] += us
        print(f"{name:>20} {d:>5} {us:9.1f}", flush=True)
    for d, us in tot.items():
        print(f"total {d:>5}: {us:8.1f} us")


if __name__ == "__main__":
    main()
