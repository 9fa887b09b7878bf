#!/usr/bin/env python3
"""Record conv2d_wino's and conv2d_wino_bwdw's outputs as bit-exact fixtures
(run on the GPU box, at the commit whose results are the reference).

  python tools/record_wino_pipe_golden.py [out_dir]   # default tests/golden/wino_pipe_parent

One .npz per case (and direction) of tests/test_wino_pipe_gpu.py; a file that
already exists is left as it is, so only new cases are written.  Inputs come
from numpy's frozen RandomState stream of the case's seed, weights scaled by
0.1; their sha256 is stored, and the arrays themselves when they are small.  An
output above 64 K elements is stored as a fixed seeded 64 K-element sample
(`idx` holds the flat indices).
"""

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# conv2d_wino cases (B, Ci, H, W, Co, pad): each runs flip=False with bias and
# flip=True without
PIPE_CASES = [
    (2, 8, 4, 4, 16, 1),
    (2, 48, 2, 2, 32, 1),
    (3, 40, 6, 10, 24, 1),
    (3, 16, 12, 12, 80, 1),
    (2, 8, 10, 10, 32, 0),
    (2, 8, 6, 6, 32, 2),
    (2, 96, 8, 8, 64, 1),
    (4, 256, 2, 2, 256, 1),
]
# conv2d_wino_bwdw cases (B, Ci, H, W, Co, pad)
BWDW_CASES = [
    (2, 8, 4, 4, 16, 1),
    (3, 24, 6, 10, 40, 1),
    (2, 8, 10, 10, 24, 0),
    (2, 8, 6, 6, 16, 2),
    (4, 3, 32, 32, 64, 1),
]

SAMPLE = 65536          # output elements kept of a large output
STORE_INPUTS = 8192   # inputs are stored up to this many elements in all


def pipe_name(case, flip):
    B, Ci, H, W, Co, pad = case
    return f"pipe_b{B}_ci{Ci}_{H}x{W}_co{Co}_p{pad}_{'flip' if flip else 'fwd'}"


def bwdw_name(case):
    B, Ci, H, W, Co, pad = case
    return f"bwdw_b{B}_ci{Ci}_{H}x{W}_co{Co}_p{pad}"


def case_seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def pipe_inputs(case, flip):
    """x [B,Ci,H,W], w (flip: [Ci,Co,3,3], else [Co,Ci,3,3]), bias or None."""
    B, Ci, H, W, Co, pad = case
    rs = np.random.RandomState(case_seed(pipe_name(case, flip)))
    x = rs.standard_normal((B, Ci, H, W)).astype(np.float32)
    wshape = (Ci, Co, 3, 3) if flip else (Co, Ci, 3, 3)
    w = (rs.standard_normal(wshape) * 0.1).astype(np.float32)
    bias = None if flip else rs.standard_normal((Co,)).astype(np.float32)
    return x, w, bias


def bwdw_inputs(case):
    """gy [B,Co,OH,OW], x [B,Ci,H,W]."""
    B, Ci, H, W, Co, pad = case
    rs = np.random.RandomState(case_seed(bwdw_name(case)))
    gy = rs.standard_normal((B, Co, H + 2 * pad - 2, W + 2 * pad - 2)).astype(np.float32)
    x = rs.standard_normal((B, Ci, H, W)).astype(np.float32)
    return gy, x


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def sample_idx(name, numel):
    if numel <= SAMPLE:
        return None
    rs = np.random.RandomState(case_seed(name) ^ 0x5A5A5A5A)
    return np.sort(rs.choice(numel, SAMPLE, replace=False)).astype(np.int64)


def save(out_dir, name, inputs, out):
    path = os.path.join(out_dir, name + ".npz")
    if os.path.exists(path):
        print(f"{name}: exists, kept", flush=True)
        return
    rec = {"sha256": np.array(digest(inputs.values()))}
    if sum(a.size for a in inputs.values() if a is not None) <= STORE_INPUTS:
        rec.update({k: v for k, v in inputs.items() if v is not None})
    flat = out.reshape(-1)
    idx = sample_idx(name, flat.size)
    if idx is None:
        rec["out"] = out
    else:
        rec["idx"] = idx
        rec["out"] = flat[idx]
    np.savez_compressed(path, **rec)
    print(f"{name}: out {tuple(out.shape)}"
          + (f" sampled {SAMPLE}" if idx is not None else ""), flush=True)


def main():
    import torch
    from split_learning_amd.ops.functional import native
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, "tests", "golden", "wino_pipe_parent")
    os.makedirs(out_dir, exist_ok=True)
    n = native()
    dev = torch.device("cuda:0")

    def t(a):
        return None if a is None else torch.from_numpy(a).to(dev)

    for case in PIPE_CASES:
        for flip in (False, True):
            x, w, bias = pipe_inputs(case, flip)
            y = n.conv2d_wino(t(x), t(w), t(bias), case[5], flip)
            save(out_dir, pipe_name(case, flip),
                 {"x": x, "w": w, "bias": bias}, y.cpu().numpy())
    for case in BWDW_CASES:
        gy, x = bwdw_inputs(case)
        gw = n.conv2d_wino_bwdw(t(gy), t(x), case[5])
        save(out_dir, bwdw_name(case), {"gy": gy, "x": x}, gw.cpu().numpy())
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
