#!/usr/bin/env python3
"""Record the outputs of the reduction kernels (BatchNorm statistics and
backward sums, split-K slab sums, colsum, cross-entropy) as bit-exact fixtures
(run on the GPU box, at the commit whose results are the reference).

  python tools/record_reduce_golden.py [out_dir]   # default tests/golden/reduce_parent

One .npz per family (bn, linear, conv_bwd, colsum, ce), keys "<case>/<array>".
Inputs are not stored: they come from an integer hash of the flat index
(`hashed`), so they are the same on any machine.  An output of at most 64 KB
is stored in full, as its bytes' integer view so that NaN payloads and the
sign of a zero take part in the comparison; a larger one as the SHA-256 of the
same bytes
("<case>/<array>.sha256").  tests/test_reduce_batched_gpu.py runs the same
cases (`CASES`) and compares with `compare`.
"""

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL_BYTES = 65536
MOM, EPS = 0.1, 1e-5


def hashed(shape, seed, scale=1.0, shift=0.0):
    """float32 values in [-0.5, 0.5) * scale + shift from a hash of the flat
    index: exact integer arithmetic, then one exact conversion."""
    n = int(np.prod(shape))
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed)) \
        & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)          # one mixing round: the plain Weyl sequence
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)   # is a sawtooth
    h ^= h >> np.uint64(12)
    v = (h >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5
    return (v * scale + shift).astype(np.float32).reshape(shape)


# ---- BatchNorm -------------------------------------------------------------
# [B, C, H, W]; every shape runs unpooled and, H and W even, pooled
BN_SHAPES = [(4, 3, 4, 6), (32, 8, 2, 2), (3, 5, 34, 34), (1, 2, 1, 8191),
             (2, 3, 64, 66), (5, 2, 40, 42)]
# channel properties; a shape with C < 4 runs a second variant that carries the
# properties its first variant has no channel for
PROPS = ("mean30", "nan", "closed", "negzero")


def bn_variants(C):
    return (0,) if C >= 4 else (0, 1)


def bn_name(shape, pool, variant):
    return "x".join(map(str, shape)) + ("_pool" if pool else "") + f"_v{variant}"


def bn_cases():
    for shape in BN_SHAPES:
        for pool in (False, True):
            if pool and (shape[2] % 2 or shape[3] % 2):
                continue
            for v in bn_variants(shape[1]):
                yield shape, pool, v


def bn_inputs(shape, pool, variant):
    B, C, H, W = shape
    seed = 1000 * (BN_SHAPES.index(shape) + 1) + 10 * variant + int(pool)
    x = hashed(shape, seed, 3.0, 0.3)
    gamma = hashed((C,), seed + 1, 1.0, 1.0)
    beta = hashed((C,), seed + 2, 0.6)
    gshape = (B, C, H // 2, W // 2) if pool else shape
    gy = hashed(gshape, seed + 3, 2.0)
    for c in range(min(C, 4)):
        prop = PROPS[(c + variant * C) % 4]
        xc = x[:, c].reshape(-1)            # a copy: channel c is strided
        if prop == "mean30":                # the double branch of the finalize
            xc += 30.0
        elif prop == "nan":
            xc[min(5, xc.size - 1)] = np.nan
        elif prop == "closed":              # every ReLU mask closed
            xc[:] = -np.abs(xc) - 0.125
            beta[c] = -100.0
        else:
            xc[::3] = -0.0
            gc = gy[:, c].reshape(-1)
            gc[::5] = -0.0
            gy[:, c] = gc.reshape(gy[:, c].shape)
        x[:, c] = xc.reshape(x[:, c].shape)
    return x, gamma, beta, gy


def run_bn(n, t, shape, pool, variant):
    import torch
    x, gamma, beta, gy = (t(a) for a in bn_inputs(shape, pool, variant))
    C = shape[1]
    rm = t(hashed((C,), 77, 1.0))
    rv = t(hashed((C,), 78, 1.0, 1.0))
    nbt = torch.tensor(3, dtype=torch.long, device=x.device)
    out = n.bn2d_train_fwd(x, gamma, beta, rm, rv, nbt, MOM, EPS, True, pool)
    y, mean, invstd = out[:3]
    idx = out[3] if pool else None
    gx, gg, gb = n.bn2d_train_bwd(x, gy, gamma, mean, invstd, y, idx)
    res = dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv,
               num_batches_tracked=nbt, gx=gx, ggamma=gg, gbeta=gb)
    if pool:
        res["idx"] = idx
    return res


def run_bn_eval(n, t):
    shape = (4, 3, 4, 6)
    x = t(hashed(shape, 9001, 3.0, 0.3))
    gy = t(hashed(shape, 9002, 2.0))
    ry = t(hashed(shape, 9003, 2.0))
    gx, gg, gb = n.bn2d_bwd_eval(x, gy, t(hashed((3,), 9004, 1.0, 1.0)),
                                 t(hashed((3,), 9005, 1.0)),
                                 t(hashed((3,), 9006, 1.0, 1.5)), ry)
    return dict(gx=gx, ggamma=gg, gbeta=gb)


# ---- split-K sums ------------------------------------------------------------
LINEAR_CASES = [(32, 4096, 10), (32, 512, 10), (5, 1030, 7)]      # (M, K, N)
# (B, Ci, H, W, Co) of tests/test_conv_bwd_pair_gpu.py: both sides split,
# both sides split, the weight side a single slice
CONV_BWD_CASES = [(2, 32, 8, 8, 64), (4, 64, 16, 16, 128), (32, 512, 4, 4, 512)]
COLSUM_CASES = [(32, 4096), (3, 7)]
# (B, C, row holding a NaN or None)
CE_CASES = [(32, 10, None), (7, 3, 4), (5, 64, None), (4, 130, None)]


def run_linear(n, t, case):
    M, K, N = case
    s = 2000 + K
    return dict(y=n.linear_fwd(t(hashed((M, K), s, 2.0)),
                               t(hashed((N, K), s + 1, 0.2)),
                               t(hashed((N,), s + 2, 1.0))))


def run_conv_bwd(n, t, case):
    B, Ci, H, W, Co = case
    s = 3000 + Ci + 7 * Co + H
    gx, gw = n.conv2d_bwd(t(hashed((B, Co, H, W), s, 2.0)),
                          t(hashed((B, Ci, H, W), s + 1, 2.0)),
                          t(hashed((Co, Ci, 3, 3), s + 2, 0.2)), 1, 1, True, True)
    return dict(gx=gx, gw=gw)


def run_colsum(n, t, case):
    return dict(out=n.colsum_f32(t(hashed(case, 4000 + case[1], 2.0))))


def run_ce(n, t, case):
    import torch
    B, C, nan_row = case
    logits = hashed((B, C), 5000 + C, 8.0)
    if nan_row is not None:
        logits[nan_row, C // 2] = np.nan
    labels = (np.arange(B, dtype=np.int64) * 7 + 3) % C
    loss, probs = n.ce_fwd(t(logits), torch.from_numpy(labels).to("cuda"))
    gl = n.ce_bwd(probs, torch.from_numpy(labels).to("cuda"),
                  t(np.array(1.5, dtype=np.float32)))
    return dict(loss=loss, probs=probs, glogits=gl)


def families():
    """family -> list of (case name, runner(n, t) -> {array name: tensor})."""
    fam = {"bn": [], "linear": [], "conv_bwd": [], "colsum": [], "ce": []}
    for shape, pool, v in bn_cases():
        fam["bn"].append((bn_name(shape, pool, v),
                          lambda n, t, a=(shape, pool, v): run_bn(n, t, *a)))
    fam["bn"].append(("eval_4x3x4x6", run_bn_eval))
    for c in LINEAR_CASES:
        fam["linear"].append(("x".join(map(str, c)),
                              lambda n, t, c=c: run_linear(n, t, c)))
    for c in CONV_BWD_CASES:
        fam["conv_bwd"].append(("x".join(map(str, c)),
                                lambda n, t, c=c: run_conv_bwd(n, t, c)))
    for c in COLSUM_CASES:
        fam["colsum"].append(("x".join(map(str, c)),
                              lambda n, t, c=c: run_colsum(n, t, c)))
    for c in CE_CASES:
        fam["ce"].append((f"{c[0]}x{c[1]}", lambda n, t, c=c: run_ce(n, t, c)))
    return fam


CASES = [(f, name) for f, cs in families().items() for name, _ in cs]


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def run_case(family, name):
    from split_learning_amd.ops.functional import native
    runner = dict(families()[family])[name]
    return {k: v.detach().cpu().numpy() for k, v in
            runner(native(), to_device).items()}


def bits(a):
    """the array's bytes as unsigned integers of its item size: NaN payloads
    and the sign of a zero take part in the comparison"""
    a = np.ascontiguousarray(a).reshape(-1)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.itemsize])


def pack(name, arrays):
    rec = {}
    for k, a in arrays.items():
        if a.nbytes <= FULL_BYTES:
            rec[f"{name}/{k}"] = bits(a)
        else:
            rec[f"{name}/{k}.sha256"] = np.array(
                hashlib.sha256(bits(a).tobytes()).hexdigest())
    return rec


def compare(name, arrays, golden):
    """what differs from the recording, one line per array; empty if nothing"""
    bad = []
    for k, a in arrays.items():
        u = bits(a)
        if f"{name}/{k}" in golden:
            g = golden[f"{name}/{k}"]
            if u.shape != g.shape or u.dtype != g.dtype:
                bad.append(f"{k}: shape or type")
            elif not np.array_equal(u, g):
                bad.append(f"{k}: {int((u != g).sum())} of {u.size} elements")
        elif str(golden[f"{name}/{k}.sha256"]) != \
                hashlib.sha256(u.tobytes()).hexdigest():
            bad.append(f"{k}: digest")
    return bad


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, "tests", "golden", "reduce_parent")
    os.makedirs(out_dir, exist_ok=True)
    for family, cs in families().items():
        rec = {}
        for name, _ in cs:
            rec.update(pack(name, run_case(family, name)))
        np.savez_compressed(os.path.join(out_dir, family + ".npz"), **rec)
        print(f"{family}: {len(cs)} cases, {len(rec)} arrays", flush=True)


if __name__ == "__main__":
    main()
