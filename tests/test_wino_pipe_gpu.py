"""conv2d_wino as a three-launch pipeline (both operand transforms in one
launch, the frequency GEMM, split-K slabs summed in the output transform):
tile grids, paddings, K tails and slab counts at their smallest instances,
against torch (atol = rtol = 1e-4, as test_conv2d_winograd) and bit-for-bit
against the outputs the five-launch pipeline produced
(tests/golden/wino_pipe_parent, written by tools/record_wino_pipe_golden.py
on the parent commit).

Second family: conv2d_wino_bwdw, the unfused bwd-weight pipeline, against
torch's conv weight gradient (atol = rtol = 2e-4, as test_bwdw_matches_torch
of test_wino_fused_lds_gpu.py; the recording commit passes it at all five
cases, worst error 0.2 of the bound at the stem shape) and bit-for-bit
against the outputs recorded before its transform kernels moved onto the
shared definitions of csrc/wino_math.h (two recordings held equal arrays)."""

import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_wino_pipe_golden as rec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "wino_pipe_parent")
TOL = dict(atol=1e-4, rtol=1e-4)

# (B, Ci, H, W, Co, pad) -> split-K slabs of the frequency GEMM (K = Ci, the
# same in both directions)
PIPE_CASES = [
    (2, 8, 4, 4, 16, 1),       # T = 8, one K-step with a K tail (8 of 16), no split
    (2, 48, 2, 2, 32, 1),      # one tile per image, every tap row/col padded; 2 slabs
    (3, 40, 6, 10, 24, 1),     # T = 45 non-square; 2 slabs, second with a K tail of 8
    (3, 16, 12, 12, 80, 1),    # T = 108: two N tiles (second partial), two M tiles
    (2, 8, 10, 10, 32, 0),     # pad 0: no tap masked
    (2, 8, 6, 6, 32, 2),       # pad 2 (bwd-data form of a pad-0 layer)
    (2, 96, 8, 8, 64, 1),      # 3 slabs, as the 256ch 8x8 layer
    (4, 256, 2, 2, 256, 1),    # 8 slabs with T = B, the 2x2 tail at a quarter width
]
SLABS = [1, 2, 2, 1, 1, 1, 3, 8]

_ids = lambda c: "x".join(map(str, c))  # noqa: E731


def test_case_table_matches_recorder():
    assert PIPE_CASES == rec.PIPE_CASES


@pytest.mark.parametrize("case,slabs", list(zip(PIPE_CASES, SLABS)),
                         ids=[_ids(c) for c in PIPE_CASES])
def test_slab_counts(case, slabs):
    from split_learning_amd.ops.functional import native
    B, Ci, H, W, Co, pad = case
    T = B * ((H + 2 * pad - 2) // 2) * ((W + 2 * pad - 2) // 2)
    assert native().conv2d_wino_slabs(Co, Ci, T) == slabs


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


@functools.lru_cache(maxsize=None)
def _run(case, flip):
    from split_learning_amd.ops.functional import native
    x, w, bias = rec.pipe_inputs(case, flip)
    y = native().conv2d_wino(_dev(x), _dev(w), _dev(bias), case[5], flip)
    return (x, w, bias), y


@pytest.mark.parametrize("flip", [False, True], ids=["fwd", "flip"])
@pytest.mark.parametrize("case", PIPE_CASES, ids=_ids)
def test_matches_torch(case, flip):
    B, Ci, H, W, Co, pad = case
    (x, w, bias), y = _run(case, flip)
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
@pytest.mark.parametrize("case", PIPE_CASES, ids=_ids)
def test_bit_identical_to_parent(case, flip):
    inputs, y = _run(case, flip)
    name = rec.pipe_name(case, flip)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert str(g["sha256"]) == rec.digest(inputs), "inputs differ from the recorded ones"
    for key, a in zip(("x", "w", "bias"), inputs):
        if key in g.files:
            assert np.array_equal(g[key], a)
    got = y.cpu().numpy().reshape(-1)
    if "idx" in g.files:
        got = got[g["idx"]]
    want = g["out"].reshape(-1)
    assert np.array_equal(got, want), (
        f"{name}: {np.count_nonzero(got != want)} of {got.size} elements "
        f"differ from the parent's output")


# ---- conv2d_wino_bwdw: gy transform, input transform, frequency GEMM over
# the tile axis (matmul_f32's fixed-order split-K), gw transform.  The route
# of the layers whose channel counts are no multiples of 32.
# (B, Ci, H, W, Co, pad)
BWDW_CASES = [
    (2, 8, 4, 4, 16, 1),       # T = 8, one K-step, every patch touches padding
    (3, 24, 6, 10, 40, 1),     # non-square tiles, T = 45 (K tail), channels not multiples of 32
    (2, 8, 10, 10, 24, 0),     # pad 0: no tap masked
    (2, 8, 6, 6, 16, 2),       # pad 2
    (4, 3, 32, 32, 64, 1),     # the stem: T = 1024, the GEMM's K splits and its slab reduce runs
]
BWDW_TOL = dict(atol=2e-4, rtol=2e-4)   # as test_bwdw_matches_torch


def test_bwdw_case_table_matches_recorder():
    assert BWDW_CASES == rec.BWDW_CASES


@functools.lru_cache(maxsize=None)
def _run_bwdw(case):
    from split_learning_amd.ops.functional import native
    gy, x = rec.bwdw_inputs(case)
    return (gy, x), native().conv2d_wino_bwdw(_dev(gy), _dev(x), case[5])


@pytest.mark.parametrize("case", BWDW_CASES, ids=_ids)
def test_bwdw_matches_torch(case):
    B, Ci, H, W, Co, pad = case
    (gy, x), gw = _run_bwdw(case)
    wr = torch.zeros(Co, Ci, 3, 3, device="cuda", requires_grad=True)
    F.conv2d(_dev(x), wr, None, 1, pad).backward(_dev(gy))
    print(f"bwdw {_ids(case)}: max |gw - torch| = "
          f"{float((gw - wr.grad).abs().max()):.3e}, "
          f"max |torch| = {float(wr.grad.abs().max()):.3e}")
    torch.testing.assert_close(gw, wr.grad, **BWDW_TOL)


@pytest.mark.parametrize("case", BWDW_CASES, ids=_ids)
def test_bwdw_bit_identical_to_parent(case):
    inputs, gw = _run_bwdw(case)
    name = rec.bwdw_name(case)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert str(g["sha256"]) == rec.digest(inputs), "inputs differ from the recorded ones"
    for key, a in zip(("gy", "x"), inputs):
        if key in g.files:
            assert np.array_equal(g[key], a)
    got = gw.cpu().numpy().reshape(-1)
    if "idx" in g.files:
        got = got[g["idx"]]
    want = g["out"].reshape(-1)
    assert np.array_equal(got, want), (
        f"{name}: {np.count_nonzero(got != want)} of {got.size} elements "
        f"differ from the parent's output")
