"""The reduction kernels keep the parent's bits.

BatchNorm statistics and backward sums, the split-K slab sums behind
linear_fwd and conv2d_bwd, colsum and the cross-entropy forward issue the
loads of several iterations ahead of their use; the arithmetic, its order and
the thread that does it are what they were, so every output must equal, bit
for bit, what the commit before that change produced
(tests/golden/reduce_parent, written there by tools/record_reduce_golden.py,
which also defines the cases and their inputs).  The comparison is on the
raw bits: a NaN's sign and payload and the sign of a zero count.
"""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_reduce_golden as rec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "reduce_parent")
_golden = {}


def _family(family):
    if family not in _golden:
        with np.load(os.path.join(GOLDEN, family + ".npz")) as z:
            _golden[family] = {k: z[k] for k in z.files}
    return _golden[family]


def _native():
    from split_learning_amd.ops.functional import native
    return native()


@pytest.mark.parametrize("family,name", rec.CASES,
                         ids=[f"{f}-{n}" for f, n in rec.CASES])
def test_outputs_equal_the_parents_bits(family, name):
    golden = _family(family)
    out = rec.run_case(family, name)
    recorded = {k.split("/")[1].replace(".sha256", "") for k in golden
                if k.startswith(name + "/")}
    assert recorded == set(out), "the recording holds other arrays"
    assert rec.compare(name, out, golden) == []


def test_cases_carry_what_they_are_for():
    """every BN shape sees all four channel properties; the NaN reaches the
    statistics; the closed channel's masks are closed"""
    for shape in rec.BN_SHAPES:
        seen = set()
        for v in rec.bn_variants(shape[1]):
            seen |= {rec.PROPS[(c + v * shape[1]) % 4]
                     for c in range(min(shape[1], 4))}
        assert seen == set(rec.PROPS), shape
    out = rec.run_case("bn", rec.bn_name((4, 3, 4, 6), False, 0))
    assert abs(out["mean"][0] - 30.3) < 0.5            # mean30
    assert np.isnan(out["mean"][1]) and np.isnan(out["gx"][:, 1]).all()
    assert not out["y"][:, 2].any() and not out["gx"][:, 2].any()   # closed
    assert out["ggamma"][2] == 0.0 and out["gbeta"][2] == 0.0
    x, _, _, gy = rec.bn_inputs((32, 8, 2, 2), False, 0)
    assert np.signbit(x[:, 3][x[:, 3] == 0]).any()     # -0.0
    assert np.signbit(gy[:, 3][gy[:, 3] == 0]).any()


@pytest.mark.parametrize("case", rec.LINEAR_CASES)
def test_linear_cases_run_the_slab_sum(case):
    M, K, N = case
    assert _native().matmul_f32_slab_count(1, M, N, K) > 1


def test_conv_cases_split_as_intended():
    n = _native()
    splits = [n.conv2d_bwd_pair_splits(B, Ci, H, W, Co, 1)
              for (B, Ci, H, W, Co) in rec.CONV_BWD_CASES]
    assert all(ds > 1 and ws > 1 for ds, _, ws, _ in splits[:2])
    ds, _, ws, _ = splits[2]
    assert ds > 1 and ws == 1                  # the weight side a single slice
