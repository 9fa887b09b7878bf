"""Fused Winograd kernels after the LDS-layout change: every path the new
operand layout can break, against torch (atol = rtol = 2e-4, as
test_conv2d_wino_fused_direct_and_split) and bit-for-bit against the outputs
the previous kernels produced (tests/golden/wino_fused_parent, written by
tools/record_wino_golden.py on the parent commit)."""

import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_wino_golden as rec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "wino_fused_parent")
TOL = dict(atol=2e-4, rtol=2e-4)

# (B, Ci, H, W, Co, pad)
FUSED_CASES = [
    (2, 8, 8, 8, 32, 1),       # one block, one K-step, no split
    (2, 24, 8, 8, 64, 1),      # ci-split into 3 slabs, one step per slice
    (4, 32, 32, 32, 128, 1),   # 128 base blocks -> 2 slices of 2 K-steps
    (8, 24, 32, 32, 128, 1),   # 256 base blocks -> no split, 3 K-steps
    (32, 8, 6, 10, 32, 1),     # non-square tiles, T = 480
    (2, 8, 10, 10, 32, 0),     # T = 32, no padding
    (2, 8, 6, 6, 32, 2),       # T = 32, pad 2 (bwd-data form of a pad-0 layer)
]
# (B, Ci, H, W, Co), pad 1
BWDW_CASES = [
    (1, 32, 6, 6, 32),     # T = 9: second slice holds one valid tile
    (3, 32, 8, 8, 64),     # T = 48: six one-step slices
    (8, 256, 4, 4, 512),   # 128 base blocks -> 2 slices of 2 steps
    (8, 64, 4, 4, 64),     # T = 32, 2x2 block grid, four distinct wave quadrants
]


def test_case_tables_match_recorder():
    assert FUSED_CASES == rec.FUSED_CASES and BWDW_CASES == rec.BWDW_CASES


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


@functools.lru_cache(maxsize=None)
def _fused(case, flip):
    from split_learning_amd.ops.functional import native
    x, w, bias = rec.fused_inputs(case, flip)
    y = native().conv2d_wino_fused(_dev(x), _dev(w), _dev(bias), case[5], flip)
    return (x, w, bias), y


@functools.lru_cache(maxsize=None)
def _bwdw(case):
    from split_learning_amd.ops.functional import native
    gy, x = rec.bwdw_inputs(case)
    return (gy, x), native().conv2d_wino_bwdw_fused(_dev(gy), _dev(x), 1)


def _check_golden(name, inputs, out):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert str(g["sha256"]) == rec.digest(inputs), "inputs differ from the recorded ones"
    for key, a in zip(("x", "w", "bias") if name.startswith("fused") else ("gy", "x"),
                      inputs):
        if key in g.files:
            assert np.array_equal(g[key], a)
    got = out.cpu().numpy().reshape(-1)
    if "idx" in g.files:
        got = got[g["idx"]]
    assert np.array_equal(got, g["out"].reshape(-1)), (
        f"{name}: {np.count_nonzero(got != g['out'].reshape(-1))} of {got.size} "
        f"elements differ from the parent's output")


@pytest.mark.parametrize("flip", [False, True], ids=["fwd", "flip"])
@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_matches_torch(case, flip):
    B, Ci, H, W, Co, pad = case
    (x, w, bias), y = _fused(case, flip)
    if not flip:
        ref = F.conv2d(_dev(x), _dev(w), _dev(bias), 1, pad)
    else:
        # the op computes the data gradient of a layer Co -> Ci with padding
        # 2 - pad, whose output gradient is x
        OH, OW = H + 2 * pad - 2, W + 2 * pad - 2
        a = torch.zeros(B, Co, OH, OW, device="cuda", requires_grad=True)
        z = F.conv2d(a, _dev(w), None, 1, 2 - pad)
        (ref,) = torch.autograd.grad(z, a, _dev(x))
    torch.testing.assert_close(y, ref, **TOL)


@pytest.mark.parametrize("flip", [False, True], ids=["fwd", "flip"])
@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_bit_identical_to_parent(case, flip):
    inputs, y = _fused(case, flip)
    _check_golden(rec.fused_name(case, flip), inputs, y)


@pytest.mark.parametrize("case", BWDW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bwdw_matches_torch(case):
    B, Ci, H, W, Co = case
    (gy, x), gw = _bwdw(case)
    wr = torch.zeros(Co, Ci, 3, 3, device="cuda", requires_grad=True)
    F.conv2d(_dev(x), wr, None, 1, 1).backward(_dev(gy))
    torch.testing.assert_close(gw, wr.grad, **TOL)


@pytest.mark.parametrize("case", BWDW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bwdw_bit_identical_to_parent(case):
    inputs, gw = _bwdw(case)
    _check_golden(rec.bwdw_name(case), inputs, gw)
