#!/usr/bin/env python3
"""The three Linear products at transformer shapes, three arms (run on a GPU):

  lib    today's route above _LIB_LIN_THRESH: F.linear / torch.matmul in fp32
  bf16   the bf16-operand MFMA kernels (csrc/gemm_bf16.hip), tile by the
         host rule; --tiles adds one arm per tile (t0 128x128, t1 64x128,
         t2 64x64) for settling that rule
  cast   torch.matmul on operands already cast to bf16, for orientation only;
         the two casts are timed on their own (column "cast ms")

Every arm is warmed up, then the arms take turns: ROUNDS rounds of ITERS calls
each, a device synchronise on both sides of every timed window.  Reported per
arm: the median over rounds of the time per call, its range, and
2*M*N*K / median in TFLOP/s.  One JSON line per shape and product.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from split_learning_amd.ops import native  # noqa: E402

# BERT-base at batch 32 x 128 tokens; the largest Linear of ViT (65 tokens,
# 128 -> 256) and of KWT (99 tokens, 64 -> 256) at batch 32
SHAPES = [(4096, 768, 768), (4096, 3072, 768), (4096, 768, 3072),
          (2080, 256, 128), (3168, 256, 64)]


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--tiles", action="store_true")
    args = ap.parse_args()
    dev, ext = torch.device("cuda:0"), native()
    torch.manual_seed(0)
    for M, N, K in SHAPES:
        x = torch.randn(M, K, device=dev)
        w = torch.randn(N, K, device=dev)
        b = torch.randn(N, device=dev)
        gy = torch.randn(M, N, device=dev)
        xh, wh, gh = x.bfloat16(), w.bfloat16(), gy.bfloat16()
        products = {
            "NT": ({"lib": lambda: F.linear(x, w, b),
                    "cast": lambda: F.linear(xh, wh)},
                   lambda t: ext.linear_bf16_fwd(x, w, b, t),
                   lambda: (x.bfloat16(), w.bfloat16())),
            "NN": ({"lib": lambda: torch.matmul(gy, w),
                    "cast": lambda: torch.matmul(gh, wh)},
                   lambda t: ext.linear_bf16_bwd_input(gy, w, t),
                   lambda: (gy.bfloat16(), w.bfloat16())),
            "TN": ({"lib": lambda: torch.matmul(gy.t(), x),
                    "cast": lambda: torch.matmul(gh.t(), xh)},
                   lambda t: ext.linear_bf16_bwd_weight(gy, x, t),
                   lambda: (gy.bfloat16(), x.bfloat16())),
        }
        for name, (arms, ours, casts) in products.items():
            arms = dict(arms)
            arms["bf16"] = lambda: ours(-1)
            if args.tiles:
                for t in range(3):
                    arms[f"t{t}"] = (lambda t: lambda: ours(t))(t)
            arms["cast ms"] = casts
            for fn in arms.values():
                window(fn, 5)
            times = {a: [] for a in arms}
            for _ in range(args.rounds):
                for a, fn in arms.items():
                    times[a].append(window(fn, args.iters))
            row = {"M": M, "N": N, "K": K, "product": name}
            for a, ts in times.items():
                med = statistics.median(ts)
                row[a] = {"ms": round(med * 1e3, 4),
                          "range_ms": [round(min(ts) * 1e3, 4),
                                       round(max(ts) * 1e3, 4)]}
                if a != "cast ms":
                    row[a]["tflops"] = round(2.0 * M * N * K / med / 1e12, 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
