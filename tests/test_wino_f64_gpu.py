"""The Winograd F(2x2, 3x3) kernels (csrc/wino.hip, csrc/wino_math.h) against
float64 at their edges: the five entries conv2d_wino (forward and flip),
conv2d_wino_bwdw, conv2d_wino_fused (forward and flip), conv2d_wino_bwdw_fused
and conv2d_bwd_pair called directly, and once more through the routed wrappers
conv2d_fwd, conv2d_bwd_data, conv2d_bwd_weight and conv2d_bwd.

Reference: tests/f64_reference.py.  R.conv2d, R.conv2d_bwd_data and
R.conv2d_bwd_weight are the tap-by-tap definitions in double; R.wino_conv2d
and R.wino_conv2d_bwd_weight are the kernels' algorithm in plain torch, in
float32 here.  The flip form (the backward-data convolution) has no reference
of its own: it is the forward form on the rotated, channel-transposed weight.

exact    integers from [-4, 4] in every operand ([-2, 2] where the shape needs
         it).  G holds halves, so every intermediate is a dyadic rational with
         at most two fractional bits, and fp32 and the MFMA accumulate lose
         nothing while the largest partial sum stays below 2^22.  Each case
         asserts that from its own shape before it runs, with amp the largest
         magnitude drawn: a frequency of G g G^T is at most 9/4 amp, one of
         B^T d B at most 4 amp, their Ci products sum to at most 9 amp^2 Ci and
         A^T M A multiplies by at most 9: 81 amp^2 Ci (144 * Ci * 9 at amp 4),
         plus the bias.  For the weight gradient A gy A^T and B^T d B are both
         at most 4 amp, T tiles are summed and G^T dU G multiplies by at most
         4: 64 amp^2 T (256 * T * 4 at amp 4).  The kernel must EQUAL the
         float64 reference: this finds an indexing, tile-decode, tap-rotation,
         slab or tail-mask fault.
randn    the rule of tests/f64_compare.py with the plain fp32 Winograd as the
         comparison implementation (torch's GPU conv is another algorithm;
         its error is printed in the same line and asserts nothing):
         e_kernel <= 4 * e_wino32 + 4 * eps32 * max|ref|.  And for every
         element |kernel - ref| <= (K + 16 + 1) * 2^-23 * abs64, abs64 the
         |.| form of the Winograd reference (|B^T|, |G|, |A| applied to |x|,
         |w|, |gy|) and K the reduction length: Ci forward, Co under flip, T
         for the weight gradient.  The roundings next to the K of the product
         chain, recounted from wino_math.h: forward 2 (B^T d B: one
         subtraction or addition per half) + 4 (G g G^T: two additions per
         half, the halving is exact) + 4 (A^T M A: two per half) + 1 (bias)
         = 11; weight gradient 2 (A gy A^T) + 2 (B^T d B) + 4 (G^T dU G: two
         per half) = 8.  A ci- or tile-split moves roundings of the chain
         into the slab sum and adds none beyond the slice count.  16 covers
         both counts.

What each case is there for is asserted from the extension's own arithmetic
(conv2d_wino_slabs, conv2d_wino_fused_splits, conv2d_bwd_pair_splits,
matmul_f32_slab_count) in the test_*_cases_reach_* tests.  Five cases make a
capped grid-stride loop run a second pass, which no other test or benchmark
does: wino_out_kernel (Co * T > 2^19), wino_in_body through conv2d_wino and
through conv2d_wino_bwdw (Ci * T > 2^21), wino_gyA_kernel (Co * T > 2^21),
wino_wt_body in both instantiations (Co * Ci > 2^18) and wino_gw_kernel
(Co * Ci > 2^20).

NaN and inf.  The NaN tests assert placement directly, not through cmp: the
plain Winograd reference multiplies by the zeros of its matrices, which the
kernels' written-out transforms do not, so its NaN set is wider than the
algorithm's.  Forward and flip: the kernel's NaN set is the direct conv's and
every other element carries the bits of the clean run.  Weight gradient: a
NaN in gy[b0, co0] turns gw[co0] NaN and nothing else; a NaN in x[b0, c0]
turns all of gw[:, c0] NaN, a superset of the direct conv's set at a border
(G^T mixes the taps), and nothing else.  An inf in x makes the direct conv's
non-finite set non-finite, as NaN where A^T meets +inf and -inf.

The refusal tests check the host entries' operand checks.  Without its check
each refused call would read outside a tensor; they run only against a build
that has the checks.

Measured on an MI355X: per family the number of randn comparisons and the one
that used most of its bound, then the largest share of the |.| ceiling any
element used:

family                   n  worst case                    e_kernel  e_wino32  e_torch  bound    k/bound  ceiling
conv2d_wino fwd         20  b2_ci33_4x4_co8_p1 no bias    1.1e-05   8.3e-06   1.1e-05  5.2e-05  0.21     0.023
conv2d_wino flip        18  b2_ci3_6x8_co5_p0 no bias     3.6e-06   2.6e-06   4.8e-07  1.7e-05  0.21     0.008
conv2d_wino_fused fwd   18  b2_ci8_8x8_co32_p1 no bias    5.8e-06   5.8e-06   5.4e-06  3.7e-05  0.16     0.009
conv2d_wino_fused flip  18  b32_ci8_2x2_co32_p1 no bias   4.5e-06   4.5e-06   5.7e-06  2.8e-05  0.16     0.009
conv2d_wino_bwdw         7  b7_ci15_6x6_co63_p1           1.4e-05   2.1e-05   1.5e-05  1.1e-04  0.13     0.007
conv2d_wino_bwdw_fused   7  b4_ci512_4x4_co512_p1         1.0e-05   1.0e-05   8.8e-06  5.9e-05  0.17     0.031

Over all 88 comparisons e_kernel / e_wino32 lies between 0.36 and 1.39: the
kernels err as the plain fp32 Winograd does, and the 4x rule needed no
widening.  Against torch's direct conv the same errors reach 7.5 x e_torch
(conv2d_wino flip, b2_ci3_6x8_co5_p0), which is the algorithm's price and why
torch is not the yardstick here.  The |.| ceiling is loose for Winograd (every
transform sums magnitudes where the signed one cancels), so the shares are
small; it stands as the bound that needs no second implementation.  Every exact
comparison held, the five second passes of the capped grids included: no
indexing, tile-decode, tap-rotation, slab or tail-mask fault was found, every
NaN and inf sat where the algebra puts it, and no kernel was changed.  What
was corrected is on the host: the entries now check the operands they used to
take on trust (see the refusal tests).
"""

import pytest
import torch
import torch.nn.functional as F

import f64_reference as R
from f64_compare import _ceiling, _draw, _gen, cmp, exact

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
KINDS = ["exact", "randn"]
LIMIT = 2 ** 22


def _native():
    from split_learning_amd.ops import native
    return native()


def _small(shape, g):
    """integers from [-2, 2], for the shapes whose bound needs it"""
    return torch.randint(-2, 3, shape, generator=g).float()


def _out(H, W, pad):
    return H + 2 * pad - 2, W + 2 * pad - 2


def _tiles(case):
    B, Ci, H, W, Co, pad = case
    OH, OW = _out(H, W, pad)
    return B * (OH // 2) * (OW // 2)


def _id(case):
    return "b{}_ci{}_{}x{}_co{}_p{}".format(*case)


def _fwd_bound(K, amp=4):
    """largest partial sum of the forward or flip form over K channels, bias
    (10 amp) included; 144 * K * 9 at amp 4"""
    return 81 * amp * amp * K + 10 * amp


def _bwdw_bound(T, amp=4):
    """the same for the weight gradient over T tiles; 256 * T * 4 at amp 4"""
    return 64 * amp * amp * T


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# ---------------- forward and flip ----------------
# A case is (B, Ci, H, W, Co, pad) in the ENTRY's roles: x has Ci channels, the
# result Co.  Under flip the weight is the layer's, [Ci, Co, 3, 3], and the
# entry computes that layer's data gradient at padding 2 - pad.

def _conv_operands(case, kind, flip, seed=51):
    B, Ci, H, W, Co, pad = case
    g = _gen(seed)
    x = _draw(kind, (B, Ci, H, W), g)
    w = _draw(kind, (Ci, Co, 3, 3) if flip else (Co, Ci, 3, 3), g)
    return x, w, 10 * _draw(kind, (Co,), g)


def _as_fwd(w, flip):
    """the weight the entry convolves x with"""
    return w.flip(2, 3).transpose(0, 1) if flip else w


def _conv_ref(x, w, bias, pad, flip):
    if not flip:
        return R.conv2d(x, w, bias, 1, pad)
    OH, OW = _out(x.shape[2], x.shape[3], pad)
    gx = R.conv2d_bwd_data(x, w, 1, 2 - pad, OH, OW)
    return gx if bias is None else gx + bias.double().reshape(1, -1, 1, 1)


def _check_conv(entry, case, kind, flip, operands=None):
    """with and without bias; operands: device tensors or views to use in
    place of the drawn ones (the strided tests)"""
    B, Ci, H, W, Co, pad = case
    family = f"{entry} {'flip' if flip else 'fwd'}"
    x, w, bias = operands or _conv_operands(case, kind, flip)
    if kind == "exact":
        assert _fwd_bound(Ci) < LIMIT, f"{_id(case)}: not exact in fp32"
    fn = getattr(_native(), entry)
    for b in (bias, None):
        y = fn(*_dev(x, w, b), pad, flip)
        torch.cuda.synchronize()
        assert y.shape == (B, Co) + _out(H, W, pad)
        ref = _conv_ref(x, w, b, pad, flip)
        what = _id(case) + ("" if b is not None else " no bias")
        if kind == "exact":
            exact(y, ref, f"{family} {what}")
            continue
        wf = _as_fwd(w, flip)
        t32 = F.conv2d(*_dev(x, wf, b), padding=pad)
        cmp(family, what, y, R.wino_conv2d(x, wf, b, pad, torch.float32), ref,
            yard="wino32", also={"torch": t32})
        _ceiling(family, what, y, ref, R.wino_conv2d_abs(x, wf, b, pad), Ci + 16)


WINO_CASES = [
    (1, 1, 2, 2, 1, 1),       # T = 1: one tile, every patch row and column padded
    (7, 15, 6, 6, 63, 1),     # Ci 15, Co 63, T 63
    (4, 16, 8, 8, 64, 1),     # Ci 16, Co 64, T 64
    (5, 17, 2, 26, 65, 1),    # Ci 17, Co 65, T 65; H != W, tW = 13
    (2, 3, 6, 8, 5, 0),       # pad 0: nothing masked; tW = 3
    (2, 5, 2, 4, 3, 2),       # pad 2, tW = 3
    (1, 2, 2, 4, 3, 3),       # pad 3 (forward only): outputs made of padding alone
    (2, 33, 4, 4, 8, 1),      # 2 slabs: 32 + 1
    (2, 65, 4, 4, 8, 1),      # 3 slabs: 32 + 32 + 1
    (1, 250, 2, 2, 8, 1),     # 8 slabs, the last short (26 of 32)
]
WINO_RUNS = [(c, f) for c in WINO_CASES for f in (False, True)
             if not (f and c[5] > 2)]
_run_id = lambda r: _id(r[0]) + ("_flip" if r[1] else "_fwd")  # noqa: E731


def test_wino_cases_reach_what_they_are_for():
    n = _native()
    slabs = {c: n.conv2d_wino_slabs(c[4], c[1], _tiles(c)) for c in WINO_CASES}
    assert set(slabs.values()) == {1, 2, 3, 8}
    assert slabs[(2, 33, 4, 4, 8, 1)] == 2 and slabs[(2, 65, 4, 4, 8, 1)] == 3
    assert slabs[(1, 250, 2, 2, 8, 1)] == 8 and 250 % 32 != 0
    assert {1, 63, 64, 65} <= {_tiles(c) for c in WINO_CASES}
    assert {15, 16, 17} <= {c[1] for c in WINO_CASES}
    assert {63, 64, 65} <= {c[4] for c in WINO_CASES}
    assert {c[5] for c in WINO_CASES} == {0, 1, 2, 3}
    assert {c[5] for c, f in WINO_RUNS if f} == {0, 1, 2}
    assert all(c[1] != c[4] for c in WINO_CASES[1:])      # Co != Ci under flip


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("run", WINO_RUNS, ids=_run_id)
def test_wino(run, kind):
    _check_conv("conv2d_wino", run[0], kind, run[1])


# conv2d_wino_fused needs Co % 32 == 0, T % 32 == 0, Ci % 8 == 0
FUSED_CASES = [
    (2, 8, 8, 8, 32, 1),      # Ci 8: one K step, one block
    (2, 16, 8, 8, 32, 1),     # ci-split 2 x 8: one step per slice
    (4, 40, 16, 16, 256, 1),  # ci-split 16 + 16 + 8: a short last slice
    (4, 16, 32, 32, 256, 1),  # 256 blocks: no split, two K steps
    (32, 8, 2, 2, 32, 1),     # a 32-tile block over 32 images
    (32, 8, 6, 10, 32, 1),    # tW = 5, 15 tiles an image: block seams inside images
    (2, 8, 10, 10, 32, 0),    # pad 0
    (2, 8, 6, 6, 32, 2),      # pad 2
    (2, 24, 8, 8, 64, 1),     # ci-split 3 x 8, two co blocks
]
FUSED_RUNS = [(c, f) for c in FUSED_CASES for f in (False, True)]


def test_fused_cases_reach_what_they_are_for():
    n = _native()
    sp = {c: tuple(n.conv2d_wino_fused_splits(c[4], c[1], _tiles(c)))
          for c in FUSED_CASES}
    assert sp[(2, 8, 8, 8, 32, 1)] == (1, 8)
    assert sp[(2, 16, 8, 8, 32, 1)] == (2, 8)
    assert sp[(4, 40, 16, 16, 256, 1)] == (3, 16)            # 16 + 16 + 8
    assert sp[(4, 16, 32, 32, 256, 1)] == (1, 16)
    assert sp[(2, 24, 8, 8, 64, 1)] == (3, 8)
    assert _tiles((32, 8, 2, 2, 32, 1)) == 32
    assert _tiles((32, 8, 6, 10, 32, 1)) == 15 * 32 and 32 % 15 != 0
    assert {c[5] for c in FUSED_CASES} == {0, 1, 2}
    assert all(c[1] != c[4] for c in FUSED_CASES)            # the CW stride


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("run", FUSED_RUNS, ids=_run_id)
def test_wino_fused(run, kind):
    """the biased, split cases are exact only if slice 0 alone adds the bias"""
    _check_conv("conv2d_wino_fused", run[0], kind, run[1])


# ---------------- weight gradient ----------------
# (B, Ci, H, W, Co, pad) of the layer: x [B, Ci, H, W], gy [B, Co, OH, OW]

def _bwdw_operands(case, kind, seed=52, draw=None):
    B, Ci, H, W, Co, pad = case
    g = _gen(seed)
    draw = draw or (lambda s: _draw(kind, s, g))
    return draw((B, Co) + _out(H, W, pad)), draw((B, Ci, H, W))


def _torch_gw(gy, x, Co, Ci, pad):
    gyd, xd = _dev(gy, x)
    w = torch.zeros(Co, Ci, 3, 3, device=DEV, requires_grad=True)
    F.conv2d(xd, w, None, padding=pad).backward(gyd)
    return w.grad


def _check_bwdw(entry, case, kind, operands=None, amp=4):
    B, Ci, H, W, Co, pad = case
    gy, x = operands or _bwdw_operands(case, kind)
    T = _tiles(case)
    if kind == "exact":
        assert _bwdw_bound(T, amp) < LIMIT, f"{_id(case)}: not exact in fp32"
    gw = getattr(_native(), entry)(*_dev(gy, x), pad)
    torch.cuda.synchronize()
    assert gw.shape == (Co, Ci, 3, 3)
    ref = R.conv2d_bwd_weight(gy, x, 3, 3, 1, pad)
    if kind == "exact":
        exact(gw, ref, f"{entry} {_id(case)}")
        return
    cmp(entry, _id(case), gw, R.wino_conv2d_bwd_weight(gy, x, pad, torch.float32),
        ref, yard="wino32", also={"torch": _torch_gw(gy, x, Co, Ci, pad)})
    _ceiling(entry, _id(case), gw, ref, R.wino_conv2d_bwd_weight_abs(gy, x, pad),
             T + 16)


BWDW_CASES = [
    (1, 1, 2, 2, 1, 1),       # T = 1
    (7, 15, 6, 6, 63, 1),     # Ci 15, Co 63, T 63: the tile axis in 2 slabs
    (4, 16, 8, 8, 64, 1),     # Ci 16, Co 64, T 64
    (5, 17, 2, 26, 65, 1),    # Ci 17, Co 65, T 65: 3 slabs; H != W, tW = 13
    (2, 3, 6, 8, 5, 0),       # pad 0, T 12: no split
    (2, 5, 2, 4, 3, 2),       # pad 2
    (8, 3, 16, 16, 4, 1),     # T 512: 16 slabs
]


def test_bwdw_cases_reach_what_they_are_for():
    n = _native()
    slabs = {c: n.matmul_f32_slab_count(16, c[4], c[1], _tiles(c)) for c in BWDW_CASES}
    assert slabs[(1, 1, 2, 2, 1, 1)] == 1 and slabs[(2, 3, 6, 8, 5, 0)] == 1
    assert slabs[(7, 15, 6, 6, 63, 1)] == 2 and slabs[(5, 17, 2, 26, 65, 1)] == 3
    assert slabs[(8, 3, 16, 16, 4, 1)] == 16
    assert {1, 63, 64, 65} <= {_tiles(c) for c in BWDW_CASES}
    assert {c[5] for c in BWDW_CASES} == {0, 1, 2}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BWDW_CASES, ids=_id)
def test_wino_bwdw(case, kind):
    _check_bwdw("conv2d_wino_bwdw", case, kind)


# conv2d_wino_bwdw_fused needs Co % 32 == 0 and Ci % 32 == 0; it stages 8
# tiles a step
BWDW_FUSED_CASES = [
    (1, 32, 2, 2, 32, 1),     # T = 1: 7 of 8 staged tiles masked
    (1, 32, 6, 6, 32, 1),     # T = 9: slices 8 + 1
    (2, 64, 6, 6, 64, 1),     # 2x2 blocks, T 18: slices 8 + 8 + 2
    (4, 512, 4, 4, 512, 1),   # 256 blocks: no split, T 16 in two steps
    (2, 32, 6, 8, 32, 0),     # pad 0, H != W, tW = 3
    (2, 32, 2, 4, 32, 2),     # pad 2, H != W
    (1, 32, 4, 10, 64, 1),    # T 10, tW = 5, Co != Ci
]


def test_bwdw_fused_cases_reach_what_they_are_for():
    # wino_bwdw_split: splits = min(ceil(256 / blocks), ceil(T / 8)), t_per =
    # T / splits rounded up to 8, slices = ceil(T / t_per); every case here but
    # the 256-block one sits at the cap, t_per 8
    def slices(case):
        B, Ci, H, W, Co, pad = case
        T, blocks = _tiles(case), (Co // 32) * (Ci // 32)
        splits = min(-(-256 // blocks) if blocks < 256 else 1, -(-T // 8))
        t_per = max(8, -(-(T // splits) // 8) * 8)
        return -(-T // t_per), t_per
    assert slices((1, 32, 2, 2, 32, 1)) == (1, 8)
    assert slices((1, 32, 6, 6, 32, 1)) == (2, 8)
    assert slices((2, 64, 6, 6, 64, 1)) == (3, 8)
    assert slices((4, 512, 4, 4, 512, 1)) == (1, 16)
    # the same arithmetic is the extension's: at shapes the pair binding takes
    n = _native()
    for case in [(2, 32, 8, 8, 64, 1), (6, 64, 8, 8, 64, 1), (32, 512, 4, 4, 512, 1),
                 (10, 192, 8, 8, 192, 1)]:
        assert tuple(n.conv2d_bwd_pair_splits(*case)[2:]) == slices(case), case
    assert {c[5] for c in BWDW_FUSED_CASES} == {0, 1, 2}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BWDW_FUSED_CASES, ids=_id)
def test_wino_bwdw_fused(case, kind):
    _check_bwdw("conv2d_wino_bwdw_fused", case, kind)


# ---------------- the pair ----------------

@pytest.mark.parametrize("interleave", [0, 1], ids=["segregated", "interleaved"])
@pytest.mark.parametrize("case", [(2, 32, 8, 8, 64, 1), (6, 64, 8, 8, 64, 1)], ids=_id)
def test_bwd_pair_exact(case, interleave):
    B, Ci, H, W, Co, pad = case
    assert _fwd_bound(Co) < LIMIT and _bwdw_bound(_tiles(case)) < LIMIT
    gy, x = _bwdw_operands(case, "exact")
    w = _draw("exact", (Co, Ci, 3, 3), _gen(53))
    gx, gw = _native().conv2d_bwd_pair(*_dev(gy, x, w), pad, interleave)
    torch.cuda.synchronize()
    exact(gx, R.conv2d_bwd_data(gy, w, 1, pad, H, W), f"pair gx {_id(case)}")
    exact(gw, R.conv2d_bwd_weight(gy, x, 3, 3, 1, pad), f"pair gw {_id(case)}")


# ---------------- grid caps ----------------
# One exact case each makes a capped grid-stride loop take a second pass.  The
# other dimensions are minimal, so the float64 side stays a few million
# products a tap.

def test_out_kernel_grid_cap():
    """wino_out_kernel: 8192 blocks of 64 (co, t) pairs"""
    case = (2, 1, 128, 128, 65, 1)
    assert case[4] * _tiles(case) > 8192 * 64
    _check_conv("conv2d_wino", case, "exact", False)


def test_in_body_grid_cap():
    """wino_in_body: 8192 blocks of 256 (ci, t) pairs, in wino_wt_in_kernel
    (conv2d_wino) and in wino_in_kernel (conv2d_wino_bwdw)"""
    case = (2, 257, 128, 128, 1, 1)
    assert case[1] * _tiles(case) > 8192 * 256
    _check_conv("conv2d_wino", case, "exact", False)
    g = _gen(54)
    _check_bwdw("conv2d_wino_bwdw", case, "exact", amp=2,
                operands=_bwdw_operands(case, "exact", draw=lambda s: _small(s, g)))


def test_gyA_kernel_grid_cap():
    """wino_gyA_kernel: 8192 blocks of 256 (co, t) pairs"""
    case = (2, 1, 128, 128, 257, 1)
    assert case[4] * _tiles(case) > 8192 * 256
    g = _gen(55)
    _check_bwdw("conv2d_wino_bwdw", case, "exact", amp=2,
                operands=_bwdw_operands(case, "exact", draw=lambda s: _small(s, g)))


@pytest.mark.parametrize("flip", [False, True], ids=["fwd", "flip"])
def test_wt_body_grid_cap(flip):
    """wino_wt_body: 4096 blocks of 256 threads, four to a (co, ci) pair"""
    case = (1, 513, 2, 2, 512, 1)
    assert case[1] * case[4] * 4 > 4096 * 256
    _check_conv("conv2d_wino", case, "exact", flip)


def test_gw_kernel_grid_cap():
    """wino_gw_kernel: 4096 blocks of 256 (co, ci) pairs"""
    case = (1, 1025, 2, 2, 1024, 1)
    assert case[1] * case[4] > 4096 * 256
    _check_bwdw("conv2d_wino_bwdw", case, "exact")


# ---------------- routed wrappers ----------------
# the smallest layers the default routing sends to each Winograd form, at pad
# 0, 1 and 2 (bwd-data runs the flip form at padding 2 - pad);
# (B, Ci, H, W, Co, pad) -> routes of fwd, bwd_data, bwd_weight
ROUTED = [
    ((1, 256, 2, 2, 256, 1), ("wino", "wino", "wino_bwdw_fused")),
    ((1, 256, 4, 4, 256, 0), ("wino", "wino", "wino_bwdw_fused")),
    ((1, 256, 2, 2, 256, 2), ("wino", "wino", "wino_bwdw_fused")),
    ((4, 8, 32, 32, 256, 1), ("wino_fused", "direct", "direct")),
    ((4, 8, 34, 34, 256, 0), ("wino_fused", "direct", "direct")),
    ((4, 8, 30, 30, 256, 2), ("wino_fused", "direct", "direct")),
    ((8, 64, 16, 16, 32, 1), ("direct", "wino_fused", "wino_bwdw_fused")),  # the pair
    ((8, 64, 16, 16, 32, 0), ("direct", "wino_fused", "wino_bwdw_fused")),
    ((8, 64, 16, 16, 32, 2), ("direct", "wino_fused", "wino_bwdw_fused")),
    ((1, 8, 2, 2, 8, 1), ("direct", "direct", "wino_bwdw")),
    ((1, 8, 6, 6, 8, 0), ("direct", "direct", "wino_bwdw")),
    ((1, 8, 2, 2, 8, 2), ("direct", "direct", "wino_bwdw")),
]


def test_routed_cases_reach_every_form():
    for k, forms in enumerate((("wino", "wino_fused"), ("wino", "wino_fused"),
                               ("wino_bwdw", "wino_bwdw_fused"))):
        for form in forms:
            assert {c[5] for c, r in ROUTED if r[k] == form} == {0, 1, 2}, (k, form)


@pytest.mark.parametrize("case,routes", ROUTED, ids=[_id(c) for c, _ in ROUTED])
def test_routed_wrappers_exact(case, routes):
    B, Ci, H, W, Co, pad = case
    n = _native()
    for op, route in zip(("fwd", "bwd_data", "bwd_weight"), routes):
        assert n.conv_route(op, B, Ci, H, W, Co, 3, 1, pad) == route, op
    assert max(_fwd_bound(Ci), _fwd_bound(Co), _bwdw_bound(_tiles(case))) < LIMIT
    gy, x = _bwdw_operands(case, "exact", seed=56)
    g = _gen(57)
    w, bias = _draw("exact", (Co, Ci, 3, 3), g), 10 * _draw("exact", (Co,), g)
    gyd, xd, wd, bd = _dev(gy, x, w, bias)
    y = n.conv2d_fwd(xd, wd, bd, 1, pad)
    gx = n.conv2d_bwd_data(gyd, wd, 1, pad, H, W)
    gw = n.conv2d_bwd_weight(gyd, xd, 3, 3, 1, pad)
    gx2, gw2 = n.conv2d_bwd(gyd, xd, wd, 1, pad, True, True)
    torch.cuda.synchronize()
    rx = R.conv2d_bwd_data(gy, w, 1, pad, H, W)
    rw = R.conv2d_bwd_weight(gy, x, 3, 3, 1, pad)
    exact(y, R.conv2d(x, w, bias, 1, pad), f"{_id(case)} conv2d_fwd")
    exact(gx, rx, f"{_id(case)} conv2d_bwd_data")
    exact(gw, rw, f"{_id(case)} conv2d_bwd_weight")
    exact(gx2, rx, f"{_id(case)} conv2d_bwd gx")
    exact(gw2, rw, f"{_id(case)} conv2d_bwd gw")


# ---------------- strided operands ----------------
# every entry copies what is not contiguous; one shape per entry, exact

def _channels_last(t):
    v = t.to(DEV).contiguous(memory_format=torch.channels_last)
    assert not v.is_contiguous()
    return v


def _expanded(t):
    """t drawn with batch 1, expanded over batch 2 (stride 0)"""
    return t.to(DEV).expand(2, -1, -1, -1)


def _slice_of_larger(w, g):
    big = _draw("exact", (w.shape[0] + 2, w.shape[1] + 3, 3, 3), g).to(DEV)
    big[1:-1, 2:-1] = w.to(DEV)
    v = big[1:-1, 2:-1]
    assert not v.is_contiguous() and v.shape == w.shape
    return v


def _hw_transposed(t):
    v = t.to(DEV).transpose(2, 3).contiguous().transpose(2, 3)
    assert not v.is_contiguous() and v.shape == t.shape
    return v


@pytest.mark.parametrize("flip", [False, True], ids=["fwd", "flip"])
@pytest.mark.parametrize("entry,case", [("conv2d_wino", (2, 5, 4, 6, 7, 1)),
                                        ("conv2d_wino_fused", (2, 8, 8, 8, 32, 1))])
def test_conv_strided_operands(entry, case, flip):
    x, w, bias = _conv_operands(case, "exact", flip, seed=58)
    for xv, wv in ((_channels_last(x), w), (_expanded(x[:1]), w),
                   (x, _slice_of_larger(w, _gen(59))), (_hw_transposed(x), w)):
        _check_conv(entry, case, "exact", flip, operands=(xv, wv, bias))


@pytest.mark.parametrize("entry,case", [("conv2d_wino_bwdw", (2, 5, 4, 6, 7, 1)),
                                        ("conv2d_wino_bwdw_fused", (2, 32, 4, 6, 32, 1))])
def test_bwdw_strided_operands(entry, case):
    gy, x = _bwdw_operands(case, "exact", seed=60)
    for gv, xv in ((gy, _channels_last(x)), (gy, _expanded(x[:1])),
                   (_hw_transposed(gy), x), (_expanded(gy[:1]), _hw_transposed(x)),
                   (_channels_last(gy), x)):
        _check_bwdw(entry, case, "exact", operands=(gv, xv))


def test_pair_strided_operands():
    case = (2, 32, 8, 8, 64, 1)
    B, Ci, H, W, Co, pad = case
    gy, x = _bwdw_operands(case, "exact", seed=61)
    w = _draw("exact", (Co, Ci, 3, 3), _gen(62))
    rx = R.conv2d_bwd_data(gy, w, 1, pad, H, W)
    rw = R.conv2d_bwd_weight(gy, x, 3, 3, 1, pad)
    for gv, xv, wv in ((_hw_transposed(gy), _channels_last(x), _slice_of_larger(w, _gen(63))),
                       (_channels_last(gy), _hw_transposed(x), w.to(DEV))):
        gx, gw = _native().conv2d_bwd_pair(gv, xv, wv, pad, -1)
        torch.cuda.synchronize()
        exact(gx, rx, "pair gx, strided operands")
        exact(gw, rw, "pair gw, strided operands")


# ---------------- NaN and inf ----------------

def _bits_equal_outside(y, clean, mask, what):
    a, b = y.cpu().view(torch.int32), clean.cpu().view(torch.int32)
    assert torch.equal(a[~mask], b[~mask]), f"{what}: a clean element moved"


# (entry, case, positions (b, c, i, j) of the non-finite value in x)
NONFINITE_FWD = [
    # corner; the seam of tiles (0, 0) and (0, 1), (1, 0), (1, 1); image 1
    ("conv2d_wino", (2, 5, 4, 6, 7, 1), [(0, 0, 0, 0), (0, 4, 1, 2), (1, 2, 3, 5)]),
    ("conv2d_wino", (2, 3, 6, 8, 5, 0), [(1, 2, 0, 0), (0, 1, 2, 3), (1, 0, 5, 7)]),
    ("conv2d_wino", (2, 5, 2, 4, 3, 2), [(0, 0, 0, 0), (1, 4, 1, 3)]),
    # tiles 31 and 32 (two 32-tile blocks of the fused kernel, and inside one
    # 64-pair block of wino_out_kernel) are tiles 1 and 2 of image 2: patch
    # columns 1..4 and 3..6, so column 3 feeds both; tiles 63 and 64 are 3 and
    # 4 of image 4: columns 5..8 and 7..10
    ("conv2d_wino", (32, 8, 6, 10, 32, 1), [(2, 7, 0, 3), (4, 0, 1, 7)]),
    ("conv2d_wino_fused", (32, 8, 6, 10, 32, 1),
     [(0, 0, 0, 0), (2, 7, 0, 3), (4, 0, 1, 7), (31, 3, 5, 9)]),
    ("conv2d_wino_fused", (2, 16, 8, 8, 32, 1), [(0, 15, 0, 0), (1, 8, 3, 4)]),
    ("conv2d_wino_fused", (2, 8, 10, 10, 32, 0), [(0, 0, 0, 0), (1, 7, 9, 9), (0, 3, 4, 5)]),
    ("conv2d_wino_fused", (2, 8, 6, 6, 32, 2), [(1, 0, 0, 0), (0, 5, 2, 3)]),
]
_nf_ids = [f"{e}-{_id(c)}" for e, c, _ in NONFINITE_FWD]


@pytest.mark.parametrize("flip", [False, True], ids=["fwd", "flip"])
@pytest.mark.parametrize("entry,case,spots", NONFINITE_FWD, ids=_nf_ids)
def test_conv_nan_and_inf_stay_in_their_receptive_field(entry, case, spots, flip):
    """one NaN in x: exactly the direct conv's NaN set, every other element
    with the bits of the clean run.  One inf in x: the same set non-finite
    (NaN where A^T meets +inf and -inf; wino.hip's header says why)."""
    B, Ci, H, W, Co, pad = case
    x, w, bias = _conv_operands(case, "randn", flip, seed=64)
    w[w == 0] = 1.0
    fn = getattr(_native(), entry)
    clean = fn(*_dev(x, w, bias), pad, flip)
    for spot in spots:
        for bad in (NAN, INF):
            xb = x.clone()
            xb[spot] = bad
            y = fn(*_dev(xb, w, bias), pad, flip)
            torch.cuda.synchronize()
            mask = ~torch.isfinite(_conv_ref(xb, w, bias, pad, flip))
            what = f"{entry} {_id(case)} flip={flip} {bad} at {spot}"
            assert bool(mask.any()) and not bool(mask[torch.arange(B) != spot[0]].any())
            assert bool((mask == mask[:, :1]).all()), "every co alike"
            got = torch.isnan(y) if bad != bad else ~torch.isfinite(y)
            assert torch.equal(got.cpu(), mask), f"{what}: placement"
            _bits_equal_outside(y, clean, mask, what)


# pad 1 and 2 only: there every pixel sits in patch rows (1, 3), (0, 2) or 1 or 2
# alone, each of which reaches all three taps through G^T
NAN_BWDW = [
    ("conv2d_wino_bwdw", (2, 5, 4, 6, 7, 1), [(0, 0, 0, 0), (1, 4, 1, 2), (1, 2, 3, 5)]),
    ("conv2d_wino_bwdw", (7, 15, 6, 6, 63, 1), [(6, 14, 5, 5), (3, 0, 2, 3)]),
    ("conv2d_wino_bwdw", (2, 5, 2, 4, 3, 2), [(0, 0, 0, 0), (1, 4, 1, 3)]),
    ("conv2d_wino_bwdw_fused", (1, 32, 6, 6, 32, 1), [(0, 0, 0, 0), (0, 31, 5, 5), (0, 7, 2, 3)]),
    ("conv2d_wino_bwdw_fused", (2, 64, 6, 6, 64, 1), [(1, 33, 0, 5), (0, 63, 3, 2)]),
    ("conv2d_wino_bwdw_fused", (2, 32, 2, 4, 32, 2), [(1, 0, 0, 0), (0, 31, 1, 3)]),
]


@pytest.mark.parametrize("entry,case,spots", NAN_BWDW,
                         ids=[f"{e}-{_id(c)}" for e, c, _ in NAN_BWDW])
def test_bwdw_nan_stays_in_its_channel(entry, case, spots):
    """a NaN in gy[b0, co0] turns gw[co0] NaN, one in x[b0, c0] turns gw[:, c0]
    NaN (a superset of the direct conv's set at a border: G^T mixes the taps);
    nothing else moves"""
    B, Ci, H, W, Co, pad = case
    OH, OW = _out(H, W, pad)
    gy, x = _bwdw_operands(case, "randn", seed=65)
    gy[gy == 0] = 1.0
    x[x == 0] = 1.0
    fn = getattr(_native(), entry)
    clean = fn(*_dev(gy, x), pad)
    for (b0, c0, i, j) in spots:
        xb = x.clone()
        xb[b0, c0, i, j] = NAN
        gw = fn(*_dev(gy, xb), pad)
        torch.cuda.synchronize()
        ref = torch.isnan(R.conv2d_bwd_weight(gy, xb, 3, 3, 1, pad))
        mask = torch.zeros(Co, Ci, 3, 3, dtype=torch.bool)
        mask[:, c0] = True
        what = f"{entry} {_id(case)} NaN in x at {(b0, c0, i, j)}"
        assert bool(ref.any()) and bool((mask | ~ref).all()), f"{what}: reference set"
        assert torch.equal(torch.isnan(gw).cpu(), mask), f"{what}: placement"
        _bits_equal_outside(gw, clean, mask, what)
        # the same spot scaled into gy's plane and channels
        co0, oi, oj = c0 % Co, i * OH // H, j * OW // W
        gb = gy.clone()
        gb[b0, co0, oi, oj] = NAN
        gw = fn(*_dev(gb, x), pad)
        torch.cuda.synchronize()
        mask = torch.zeros(Co, Ci, 3, 3, dtype=torch.bool)
        mask[co0] = True
        what = f"{entry} {_id(case)} NaN in gy at {(b0, co0, oi, oj)}"
        assert torch.equal(torch.isnan(R.conv2d_bwd_weight(gb, x, 3, 3, 1, pad)), mask)
        assert torch.equal(torch.isnan(gw).cpu(), mask), f"{what}: placement"
        _bits_equal_outside(gw, clean, mask, what)


# ---------------- refusals ----------------

def _bad_weights(w):
    return {"on the CPU": w.cpu(), "double": w.double(), "3-D": w[0]}


def _bad_biases(Co):
    z = torch.zeros
    return {"on the CPU": z(Co), "double": z(Co, device=DEV, dtype=torch.float64),
            "too short": z(Co - 1, device=DEV), "too long": z(Co + 1, device=DEV),
            "strided": z(2 * Co, device=DEV)[::2], "2-D": z(1, Co, device=DEV)}


@pytest.mark.parametrize("flip", [False, True], ids=["fwd", "flip"])
@pytest.mark.parametrize("entry,who,case", [
    ("conv2d_wino", "wino", (2, 5, 4, 6, 7, 1)),
    ("conv2d_wino_fused", "wino_fused", (2, 8, 8, 8, 32, 1))])
def test_conv_entries_refuse_bad_operands(entry, who, case, flip):
    """a weight or bias that is not the fp32 GPU tensor its shape promises, a
    negative pad, and pad 3 under flip are refused before anything is
    allocated or launched.  The kernels read the raw pointers at [0, Co) and
    over the weight's full shape: without these checks each call here would
    address outside a tensor or a host pointer on the GPU, so this test must
    never run against a build without them (it runs only after the checks
    were written and read back)."""
    B, Ci, H, W, Co, pad = case
    fn = getattr(_native(), entry)
    x = torch.zeros(B, Ci, H, W, device=DEV)
    w = torch.zeros((Ci, Co, 3, 3) if flip else (Co, Ci, 3, 3), device=DEV)
    for what, bad in _bad_weights(w).items():
        with pytest.raises(RuntimeError, match=f"{who}: w must"):
            fn(x, bad, None, pad, flip)
    for what, bad in _bad_biases(Co).items():
        with pytest.raises(RuntimeError, match=f"{who}: bias must"):
            fn(x, w, bad, pad, flip)
    with pytest.raises(RuntimeError, match=f"{who}: pad -1"):
        fn(x, w, None, -1, flip)
    if flip:
        with pytest.raises(RuntimeError, match=f"{who}: pad 3 outside"):
            fn(x, w, None, 3, flip)
    with pytest.raises(RuntimeError):
        fn(x.double(), w, None, pad, flip)
    torch.cuda.synchronize()
    y = fn(x, w, torch.ones(Co, device=DEV), pad, flip)       # the good call still runs
    assert bool((y == 1).all())


@pytest.mark.parametrize("entry,who,case", [
    ("conv2d_wino_bwdw", "wino_bwdw", (2, 5, 4, 6, 7, 1)),
    ("conv2d_wino_bwdw_fused", "wino_bwdw_fused", (2, 32, 4, 6, 32, 1))])
def test_bwdw_entries_refuse_bad_operands(entry, who, case):
    """a gy whose batch is not x's, operands that are not fp32 GPU tensors, and
    a pad outside 0..2 are refused before anything is allocated or launched.
    The kernels index gy with x's batch and read both as float: without these
    checks each call here would address outside a tensor, so this test must
    never run against a build without them (it runs only after the checks
    were written and read back)."""
    B, Ci, H, W, Co, pad = case
    fn = getattr(_native(), entry)
    x = torch.zeros(B, Ci, H, W, device=DEV)
    gy = torch.zeros((B, Co) + _out(H, W, pad), device=DEV)
    with pytest.raises(RuntimeError, match=f"{who}: batch of gy 1 is not x's 2"):
        fn(gy[:1], x, pad)
    with pytest.raises(RuntimeError, match=f"{who}: batch of gy 2 is not x's 3"):
        fn(gy, torch.zeros(B + 1, Ci, H, W, device=DEV), pad)
    for bad in (gy.double(), gy.cpu(), gy[0]):
        with pytest.raises(RuntimeError, match=f"{who}: gy must"):
            fn(bad, x, pad)
    for bad in (x.double(), x.cpu(), x[0]):
        with pytest.raises(RuntimeError, match=f"{who}: x must"):
            fn(gy, bad, pad)
    for bad_pad in (-1, 3):
        gyp = torch.zeros((B, Co) + _out(H, W, bad_pad), device=DEV)
        with pytest.raises(RuntimeError, match=f"{who}: pad {bad_pad} outside"):
            fn(gyp, x, bad_pad)
    torch.cuda.synchronize()
    assert not bool(fn(gy, x, pad).any())


def test_pair_entry_refuses_bad_operands():
    """conv2d_bwd_pair read x and w as float on the strength of gy's type alone
    and took a negative pad; both are refused before anything is allocated
    or launched.  Without the checks these calls would address outside a
    tensor: never run this against a build without them."""
    B, Ci, H, W, Co = 2, 32, 8, 8, 64
    fn = _native().conv2d_bwd_pair
    gy = torch.zeros(B, Co, H, W, device=DEV)
    x = torch.zeros(B, Ci, H, W, device=DEV)
    w = torch.zeros(Co, Ci, 3, 3, device=DEV)
    for bad in (x.double(), x.cpu()):
        with pytest.raises(RuntimeError, match="bwd_pair: x must"):
            fn(gy, bad, w, 1, -1)
    for bad in (w.double(), w.cpu()):
        with pytest.raises(RuntimeError, match="bwd_pair: w must"):
            fn(gy, x, bad, 1, -1)
    gyp = torch.zeros(B, Co, H - 4, W - 4, device=DEV)
    with pytest.raises(RuntimeError, match="bwd_pair: pad -1 outside"):
        fn(gyp, x, w, -1, -1)
    with pytest.raises(RuntimeError, match="bwd_pair geometry"):
        fn(gy[:1], x, w, 1, -1)
    torch.cuda.synchronize()
    gx, gw = fn(gy, x, w, 1, -1)
    assert not bool(gx.any()) and not bool(gw.any())
