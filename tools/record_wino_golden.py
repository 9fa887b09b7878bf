#!/usr/bin/env python3
"""Record the fused-Winograd ops' outputs as bit-exact fixtures (run on the GPU
box, at the commit whose results are the reference).

  python tools/record_wino_golden.py [out_dir]     # default tests/golden/wino_fused_parent

One .npz per case of tests/test_wino_fused_lds_gpu.py.  Inputs come from
numpy's frozen RandomState stream of the case's seed, weights scaled by 0.1;
their sha256 is stored, and the arrays themselves when they are small.  An
output above 64 K elements is stored as a fixed seeded 64 K-element sample
(`idx` holds the flat indices).
"""

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# conv2d_wino_fused cases (B, Ci, H, W, Co, pad): each runs flip=False with
# bias and flip=True without
FUSED_CASES = [
    (2, 8, 8, 8, 32, 1),
    (2, 24, 8, 8, 64, 1),
    (4, 32, 32, 32, 128, 1),
    (8, 24, 32, 32, 128, 1),
    (32, 8, 6, 10, 32, 1),
    (2, 8, 10, 10, 32, 0),
    (2, 8, 6, 6, 32, 2),
]
# conv2d_wino_bwdw_fused cases (B, Ci, H, W, Co), pad 1
BWDW_CASES = [
    (1, 32, 6, 6, 32),
    (3, 32, 8, 8, 64),
    (8, 256, 4, 4, 512),
    (8, 64, 4, 4, 64),
]

SAMPLE = 65536          # output elements kept of a large output
STORE_INPUTS = 131072   # inputs are stored up to this many elements in all


def fused_name(case, flip):
    B, Ci, H, W, Co, pad = case
    return f"fused_b{B}_ci{Ci}_{H}x{W}_co{Co}_p{pad}_{'flip' if flip else 'fwd'}"


def bwdw_name(case):
    B, Ci, H, W, Co = case
    return f"bwdw_b{B}_ci{Ci}_{H}x{W}_co{Co}"


def case_seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def fused_inputs(case, flip):
    """x [B,Ci,H,W], w (flip: [Ci,Co,3,3], else [Co,Ci,3,3]), bias or None."""
    B, Ci, H, W, Co, pad = case
    rs = np.random.RandomState(case_seed(fused_name(case, flip)))
    x = rs.standard_normal((B, Ci, H, W)).astype(np.float32)
    wshape = (Ci, Co, 3, 3) if flip else (Co, Ci, 3, 3)
    w = (rs.standard_normal(wshape) * 0.1).astype(np.float32)
    bias = None if flip else rs.standard_normal((Co,)).astype(np.float32)
    return x, w, bias


def bwdw_inputs(case):
    """gy [B,Co,H,W], x [B,Ci,H,W] (pad 1: same spatial size)."""
    B, Ci, H, W, Co = case
    rs = np.random.RandomState(case_seed(bwdw_name(case)))
    gy = rs.standard_normal((B, Co, H, W)).astype(np.float32)
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
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **rec)
    print(f"{name}: out {tuple(out.shape)}"
          + (f" sampled {SAMPLE}" if idx is not None else ""), flush=True)


def main():
    import torch
    from split_learning_amd.ops.functional import native
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, "tests", "golden", "wino_fused_parent")
    os.makedirs(out_dir, exist_ok=True)
    n = native()
    dev = torch.device("cuda:0")

    def t(a):
        return None if a is None else torch.from_numpy(a).to(dev)

    for case in FUSED_CASES:
        for flip in (False, True):
            x, w, bias = fused_inputs(case, flip)
            y = n.conv2d_wino_fused(t(x), t(w), t(bias), case[5], flip)
            save(out_dir, fused_name(case, flip),
                 {"x": x, "w": w, "bias": bias}, y.cpu().numpy())
    for case in BWDW_CASES:
        gy, x = bwdw_inputs(case)
        gw = n.conv2d_wino_bwdw_fused(t(gy), t(x), 1)
        save(out_dir, bwdw_name(case), {"gy": gy, "x": x}, gw.cpu().numpy())
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
