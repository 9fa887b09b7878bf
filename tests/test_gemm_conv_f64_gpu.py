"""The MFMA tile-GEMM core (tile_gemm.h) through matmul_f32, linear_fwd and the
three direct convolutions plus the conv bias gradient, against float64 at
their edges; and the guard on FastDiv's range.

Reference: tests/f64_reference.py, the plain definition of each op in torch
double on the CPU.  Two kinds of input run at every edge:

exact    integers drawn uniformly from [-4, 4], stored as fp32.  Products are
         at most 16 and every partial sum stays below 2^24, so every
         summation order, split count and atomic arrival order gives the
         same bits: the kernel must EQUAL the float64 reference.  This is
         the indexing test; it fails for any dropped, doubled or misplaced
         term.
randn    the rule of tests/f64_compare.py against torch fp32 on the GPU
         (torch.matmul, F.linear, F.conv2d and its autograd):
         e_kernel <= 4 * e_torch + 4 * eps32 * max|ref|, NaN and inf where the
         reference has them; and, needing no yardstick, for every element
         |kernel - ref| <= (K + 1) * 2^-23 * (|A| @ |B|), the right side in
         double through the op's own gather (a bias adds its |bias| to the
         sum it joins): the bound of an fp32 fma chain of K terms in any
         order, which split-K only reorders.

Shapes are the smallest that reach each path: M, N, K one either side of the
64x64 tile and the 16-wide K step; a short last split (K = 33: 32 + 1, K =
100: 32 + 32 + 32 + 4); the split count shrunk by K-step alignment (K = 4608:
64 becomes 58); 8 and 9 n-tiles (the XCD remap on and off); operands that are
views; every conv specialisation (3x3 s1, 3x3 s2, 1x1, 4x4 s4, run-time
geometry) at pad 0, 1, 2, H != W, B = 1, OH*OW in {1, 9, 25} (plain bwd-weight
addressing) and {16, 64} (the hoisted one), Co and B*OH*OW either side of 64,
Ci*KH*KW either side of 16 and 32.  Each conv case asserts with conv_route
that all three directions take the direct kernels, and its split (the count
matmul_f32_slab_count gives for the direction's M, N, K) decides the output
mode: 1 stores, 2 adds atomically, 3 or more writes slabs;
test_conv_cases_reach_every_output_mode holds the table to all three per
direction.  The 32 MB slab cap of plan_split cannot be reached through
slk_pick_split_k: a split of 3 or more needs fewer than 640 output tiles and
then asks for at most 1280 / tiles + 1 splits of tiles * 16 KB, under 31.4 MB;
no test is contorted for it.

Measured on an MI355X: per family the number of comparisons and the one that
used most of its bound (k/t = e_kernel / e_torch), then the largest share of
the fma-chain ceiling any element used:

family         n  worst case                                e_kernel  e_torch  k/t  bound    k/bound  ceiling
matmul        65  b expanded batch (3x65x63x33)             4.9e-06   3.9e-06  1.3  2.7e-05  0.19     0.25
matmul out=    8  64x64x4608, overwrite (one 4608 chain)    6.6e-04   2.1e-04  3.1  9.8e-04  0.67     0.10
linear        12  63x64x33, no bias                         5.0e-06   3.5e-06  1.4  2.7e-05  0.18     0.09
conv 3x3 s1   44  b1 ci1 7x9 co2 p1 bwd_weight              2.5e-06   4.7e-07  5.3  8.7e-06  0.28     0.19
conv 3x3 s2   32  b2 ci5 7x9 co17 p1 bwd_weight             2.7e-06   7.9e-07  3.4  1.2e-05  0.22     0.19
conv 1x1      36  b3 ci33 5x5 co4 bwd_weight                3.9e-06   7.8e-07  5.0  1.3e-05  0.31     0.24
conv 4x4 s4   32  b1 ci2 16x16 co5 fwd                      3.3e-06   6.2e-07  5.3  1.2e-05  0.27     0.23
conv generic  52  b1 ci3 9x11 co5 7x7 s2 p3 bwd_weight      2.6e-06   4.5e-07  5.9  8.9e-06  0.30     0.11

(The ceiling's largest shares are single products, K = 1: half an ulp of a
product against 2 * 2^-23 of it.)  Every exact comparison held: no indexing
fault was found in the core, the gathers or the stores.  One kernel was
corrected.  The conv bias gradient summed in float, and on conv 1x1 b1 ci3 3x3
co2 p1, whose 25 terms of size 1 sum to 0.06 and 0.31 on its two channels, it
measured e_kernel 7.5e-07 on e_torch 1.2e-07 and a bound of 6.3e-07: summation
order alone, six roundings at the size of the partial sums, but over the rule,
as the softmax backward's float dot was in the small-kernel module.  It now
sums in double and rounds once, as the BatchNorm sums do: 3.7e-09 on the same
case.  (No conv of the benchmarked VGG16 calls it: under a training BatchNorm
the bias gradient is skipped as analytically zero.)

FastDiv: the kernels' index divider is exact only while dividend * divisor <
2^40, and no call site checked the divisor; tests/test_fastdiv.py has the
arithmetic.  The raising tests here check that an out-of-range shape is refused
before anything is launched (they would address far outside the tensor on a
build without the guard, and must never run on one); conv 1x1 on
(16, 1, 512, 512), whose largest dividend * divisor is 2^40 - 2^18, is accepted
and exact.  MaxPool on (1, 3, 1024, 1024) divides by the pooled 512x512 plane
in its forward, which is in range and checked exact; its backward, and the
forward on (1, 2, 2048, 2048), divide by 2^20 and are refused.
"""

import pytest
import torch
import torch.nn.functional as F

import f64_reference as R
from f64_compare import _ceiling, _draw, _gen, cmp, exact

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 12345.0
NAN, INF = float("nan"), float("inf")


def _native():
    from split_learning_amd.ops import native
    return native()


# ---------------- GEMM ----------------

# the slabs matmul_f32 and linear_fwd split K into, at every M, N and batch
# used here (at most 27 tiles, so the split is capped by K alone): K <= 32 is
# not split; 33 = 32 + 1; 100 = 32 + 32 + 32 + 4; 4608 asks for 64 splits of
# 72, which the K-step rounds to 80: 58
SLABS = {33: 2, 100: 4, 4608: 58}


def _assert_slabs(nb, M, N, K):
    got = _native().matmul_f32_slab_count(nb, M, N, K)
    assert got == SLABS.get(K, 1), f"{nb}x{M}x{N}x{K}: {got} slabs"
    assert K > 32 or got == 1


def _mm_dims(a, b, ta, tb):
    M = a.shape[-1] if ta else a.shape[-2]
    K = a.shape[-2] if ta else a.shape[-1]
    N = b.shape[-2] if tb else b.shape[-1]
    return M, N, K


def _check_mm(kind, what, a, b, ta=False, tb=False):
    """a, b: device tensors or views, as matmul_f32 takes them"""
    M, N, K = _mm_dims(a, b, ta, tb)
    _assert_slabs(a.shape[0] if a.dim() == 3 else 1, M, N, K)
    c = _native().matmul_f32(a, b, ta, tb, None, False)
    torch.cuda.synchronize()
    ref = R.matmul(a, b, ta, tb)
    if kind == "exact":
        exact(c, ref, f"matmul {what}")
        return
    at = a.transpose(-1, -2) if ta else a
    bt = b.transpose(-1, -2) if tb else b
    cmp("matmul", what, c, torch.matmul(at, bt), ref)
    _ceiling("matmul", what, c, ref, R.matmul(a.abs(), b.abs(), ta, tb), K)


KINDS = ["exact", "randn"]

# K across the K step and the split thresholds at a tile-straddling (M, N);
# M and N across the tile at an unsplit and a 2-slab K; the corners
MM_SHAPES = (
    [(65, 63, K) for K in (1, 15, 16, 17, 32, 33, 100, 4608)]
    + [(M, 65, K) for M in (1, 63, 64, 129) for K in (17, 33)]
    + [(63, N, K) for N in (1, 64, 65, 129) for K in (17, 33)]
    + [(1, 1, 1), (1, 1, 4608), (64, 64, 4608), (64, 64, 16), (129, 129, 100)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,N,K", MM_SHAPES)
def test_matmul_edges(M, N, K, kind):
    g = _gen(1000 * M + 10 * N + K)
    a, b = _draw(kind, (M, K), g).to(DEV), _draw(kind, (K, N), g).to(DEV)
    _check_mm(kind, f"{M}x{N}x{K}", a, b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True),
                                   (True, True)])
@pytest.mark.parametrize("M,N,K", [(65, 63, 33), (63, 129, 17)])
def test_matmul_trans(M, N, K, ta, tb, kind):
    g = _gen(21)
    a = _draw(kind, (K, M) if ta else (M, K), g).to(DEV)
    b = _draw(kind, (N, K) if tb else (K, N), g).to(DEV)
    _check_mm(kind, f"{M}x{N}x{K} ta={ta} tb={tb}", a, b, ta, tb)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ta,tb", [(False, False), (True, True)])
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("M,N,K", [(65, 63, 33), (63, 65, 17), (64, 1, 100)])
def test_matmul_batched(M, N, K, nb, ta, tb, kind):
    g = _gen(22)
    a = _draw(kind, (nb, K, M) if ta else (nb, M, K), g).to(DEV)
    b = _draw(kind, (nb, N, K) if tb else (nb, K, N), g).to(DEV)
    _check_mm(kind, f"{nb}x{M}x{N}x{K} ta={ta} tb={tb}", a, b, ta, tb)


# operands that are views: (name, a of [.., M, K], b of [.., K, N]) built from
# dense tensors by the view alone, M, N, K = 65, 63, 33
def _views(kind, g):
    M, N, K = 65, 63, 33
    d = lambda *s: _draw(kind, s, g).to(DEV)  # noqa: E731
    yield "a transposed view", d(K, M).t(), d(K, N)
    yield "b transposed view", d(M, K), d(N, K).t()
    yield "a[:, ::2]", d(M, 2 * K)[:, ::2], d(K, N)
    yield "b[:, ::2]", d(M, K), d(K, 2 * N)[:, ::2]
    yield "a[::2], b[::2]", d(2 * M, K)[::2], d(2 * K, N)[::2]
    # [S, H, hd] -> [H, S, hd]: the batch stride is the smallest but one
    yield "a permuted batch", d(M, 3, K).permute(1, 0, 2), d(3, K, N)
    yield "b permuted batch", d(3, M, K), d(K, 3, N).permute(1, 0, 2)
    yield "a expanded row", d(1, K).expand(M, K), d(K, N)
    yield "b expanded column", d(M, K), d(K, 1).expand(K, N)
    yield "b expanded batch", d(3, M, K), d(1, K, N).expand(3, K, N)
    yield "offset views", d(M + 3, K + 5)[3:, 5:], d(K + 2, N + 7)[2:, :N]


@pytest.mark.parametrize("kind", KINDS)
def test_matmul_strided_operands(kind):
    for what, a, b in _views(kind, _gen(23)):
        assert not (a.is_contiguous() and b.is_contiguous()), what
        _check_mm(kind, what, a, b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [512, 576])
@pytest.mark.parametrize("M,K", [(65, 17), (64, 33)])
def test_matmul_xcd_remap(M, K, N, kind):
    """8 n-tiles: block x computes n-tile (x & 7) * (tiles / 8) + (x >> 3);
    9: block x computes n-tile x"""
    g = _gen(24)
    a, b = _draw(kind, (M, K), g).to(DEV), _draw(kind, (K, N), g).to(DEV)
    _check_mm(kind, f"{M}x{N}x{K}", a, b)


def test_matmul_nan_inf():
    g = _gen(25)
    a, b = torch.randn(65, 100, generator=g), torch.randn(100, 63, generator=g)
    a[2, 99] = NAN            # the short last split
    a[64, 3] = INF
    b[3] = b[3].abs() + 1.0   # one sign per product: the row is +inf, not NaN
    b[50, 62] = NAN
    _check_mm("randn", "NaN and inf", a.to(DEV), b.to(DEV))


def _sentinel_out(shape):
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((8 + numel + 8,), SENT, device=DEV)
    gap = torch.ones_like(buf, dtype=torch.bool)
    gap[8:8 + numel] = False
    return buf, gap, buf[8:8 + numel].view(shape)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("nb,M,N,K", [(0, 65, 63, 33), (0, 1, 129, 100),
                                      (3, 63, 65, 17), (0, 64, 64, 4608)])
def test_matmul_out(nb, M, N, K, accumulate, kind):
    """out= is written in place (one launch, no split), overwritten or, with
    accumulate, added to; nothing around it is touched"""
    g = _gen(26)
    batch = (nb,) if nb else ()
    a, b = _draw(kind, batch + (M, K), g).to(DEV), _draw(kind, batch + (K, N), g).to(DEV)
    c0 = _draw(kind, batch + (M, N), g)
    buf, gap, out = _sentinel_out(batch + (M, N))
    out.copy_(c0)
    c = _native().matmul_f32(a, b, False, False, out, accumulate)
    torch.cuda.synchronize()
    assert c.data_ptr() == out.data_ptr()
    assert bool((buf[gap] == SENT).all()), "sentinel overwritten"
    ref = R.matmul(a, b) + (c0.double() if accumulate else 0.0)
    what = f"out= {batch}{M}x{N}x{K} accumulate={accumulate}"
    if kind == "exact":
        exact(out, ref, what)
        return
    t32 = torch.matmul(a, b)
    absref = R.matmul(a.abs(), b.abs())
    if accumulate:
        t32, absref = c0.to(DEV) + t32, absref + c0.double().abs()
    cmp("matmul out=", what, out, t32, ref)
    _ceiling("matmul out=", what, out, ref, absref, K)


def test_matmul_out_must_be_the_dense_product():
    n = _native()
    a, b = torch.zeros(5, 7, device=DEV), torch.zeros(7, 3, device=DEV)
    bad = {"transposed": torch.zeros(3, 5, device=DEV).t(),
           "sliced": torch.zeros(5, 6, device=DEV)[:, ::2],
           "wrong shape": torch.zeros(5, 4, device=DEV),
           "wrong rank": torch.zeros(1, 5, 3, device=DEV),
           "CPU": torch.zeros(5, 3),
           "double": torch.zeros(5, 3, device=DEV, dtype=torch.float64)}
    for what, out in bad.items():
        for accumulate in (False, True):
            with pytest.raises(RuntimeError, match="matmul_f32: out"):
                n.matmul_f32(a, b, False, False, out, accumulate)
    a3, b3 = torch.zeros(2, 5, 7, device=DEV), torch.zeros(2, 7, 3, device=DEV)
    with pytest.raises(RuntimeError, match="matmul_f32: out"):
        n.matmul_f32(a3, b3, False, False, torch.zeros(5, 3, device=DEV), False)
    good = torch.full((2, 5, 3), SENT, device=DEV)
    n.matmul_f32(a3, b3, False, False, good, False)
    assert not bool(good.any())


# bias under no split, 2 slabs and at least 3: it must be added once
LINEAR_SHAPES = [(64, 63, 17), (63, 64, 33), (1, 65, 100), (129, 65, 100),
                 (65, 10, 4608), (1, 1, 33)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_linear_fwd(M, N, K, with_bias, kind):
    g = _gen(27)
    x, w = _draw(kind, (M, K), g).to(DEV), _draw(kind, (N, K), g).to(DEV)
    bias = (10 * _draw(kind, (N,), g)).to(DEV) if with_bias else None
    _assert_slabs(1, M, N, K)
    y = _native().linear_fwd(x, w, bias)
    torch.cuda.synchronize()
    ref = R.linear(x, w, bias)
    what = f"{M}x{N}x{K} bias={with_bias}"
    if kind == "exact":
        exact(y, ref, f"linear {what}")
        return
    cmp("linear", what, y, F.linear(x, w, bias), ref)
    _ceiling("linear", what, y, ref,
             R.linear(x.abs(), w.abs(), None if bias is None else bias.abs()), K)


# ---------------- direct conv ----------------

# (B, Ci, H, W, Co, KH, KW, stride, pad)
CONV_3X3_S1 = [
    (1, 3, 5, 5, 65, 3, 3, 1, 1),     # OH*OW 25, B 1, Co 65, Ci*9 = 27
    (2, 4, 3, 3, 63, 3, 3, 1, 1),     # OH*OW 9, Co 63, Ci*9 = 36
    (1, 5, 4, 4, 64, 3, 3, 1, 1),     # OH*OW 16, Co 64
    (4, 7, 8, 8, 33, 3, 3, 1, 1),     # OH*OW 64, N 256
    (2, 3, 3, 3, 5, 3, 3, 1, 0),      # pad 0, OH*OW 1
    (1, 2, 3, 5, 3, 3, 3, 1, 2),      # pad 2, H != W
    (7, 2, 3, 3, 3, 3, 3, 1, 1),      # B*OH*OW 63
    (1, 1, 7, 9, 2, 3, 3, 1, 1),      # B*OH*OW 63 in one image, Ci 1
    (5, 2, 5, 3, 4, 3, 3, 1, 2),      # B*OH*OW 5 * 7 * 5 = 175
    (1, 2, 4, 4, 65, 3, 3, 1, 3),     # pad 3: more border than image, OH*OW 64
    (2, 8, 3, 5, 3, 3, 3, 1, 1),      # Ci*9 = 72: forward in slabs
]
CONV_3X3_S2 = [
    (2, 5, 7, 9, 17, 3, 3, 2, 1),     # 4x5, Ci*9 = 45
    (1, 2, 9, 9, 65, 3, 3, 2, 1),     # OH*OW 25, Co 65
    (3, 4, 8, 8, 6, 3, 3, 2, 0),      # pad 0, OH*OW 9
    (1, 3, 8, 8, 5, 3, 3, 2, 1),      # OH*OW 16
    (4, 2, 5, 6, 4, 3, 3, 2, 2),      # pad 2, OH*OW 16, N 64
    (1, 1, 3, 3, 1, 3, 3, 2, 0),      # OH*OW 1
    (1, 3, 16, 15, 63, 3, 3, 2, 1),   # OH*OW 64, Co 63
    (5, 8, 8, 8, 3, 3, 3, 2, 1),      # Ci*9 = 72 and B*OH*OW = 80: both in slabs
]
CONV_1X1 = [
    (1, 15, 8, 8, 63, 1, 1, 1, 0),    # Ci 15, N 64, Co 63
    (1, 16, 7, 9, 64, 1, 1, 1, 0),    # Ci 16, N 63, Co 64
    (1, 17, 5, 13, 65, 1, 1, 1, 0),   # Ci 17, N 65, Co 65
    (2, 31, 3, 3, 5, 1, 1, 1, 0),     # Ci 31, OH*OW 9
    (1, 32, 1, 1, 7, 1, 1, 1, 0),     # Ci 32, one pixel
    (3, 33, 5, 5, 4, 1, 1, 1, 0),     # Ci 33: 2 splits
    (1, 100, 4, 4, 3, 1, 1, 1, 0),    # Ci 100: 4 slabs, OH*OW 16
    (1, 3, 3, 3, 2, 1, 1, 1, 1),      # pad 1: a border of bias alone
    (2, 2, 2, 4, 3, 1, 1, 1, 2),      # pad 2, H != W
]
CONV_4X4_S4 = [
    (2, 3, 8, 12, 65, 4, 4, 4, 0),    # 2x3, Ci*16 = 48, Co 65
    (1, 1, 4, 4, 3, 4, 4, 4, 0),      # OH*OW 1, Ci*16 = 16
    (1, 2, 16, 16, 5, 4, 4, 4, 0),    # OH*OW 16, Ci*16 = 32
    (4, 3, 16, 16, 6, 4, 4, 4, 0),    # N 64
    (1, 2, 6, 6, 3, 4, 4, 4, 1),      # pad 1
    (1, 1, 8, 8, 2, 4, 4, 4, 2),      # pad 2, OH*OW 9
    (1, 2, 9, 7, 2, 4, 4, 4, 0),      # rows and columns no window reads
    (5, 5, 16, 16, 3, 4, 4, 4, 0),    # Ci*16 = 80 and B*OH*OW = 80: both in slabs
]
CONV_GENERIC = [
    (2, 3, 5, 7, 4, 5, 5, 1, 2),      # 5x5 s1 p2
    (1, 2, 8, 8, 3, 5, 5, 1, 2),      # 5x5 s1 p2, OH*OW 64
    (1, 3, 9, 11, 5, 7, 7, 2, 3),     # 7x7 s2 p3
    (2, 4, 6, 8, 5, 2, 2, 2, 0),      # 2x2 s2, Ci*4 = 16
    (1, 3, 8, 8, 4, 2, 2, 2, 0),      # 2x2 s2, OH*OW 16
    (2, 3, 7, 8, 5, 3, 3, 3, 1),      # 3x3 s3 p1: bwd-data's % with negative numerators
    (1, 2, 11, 11, 3, 5, 5, 3, 2),    # 5x5 s3 p2, OH*OW 16
    (2, 3, 5, 5, 4, 1, 1, 2, 0),      # 1x1 s2
    (1, 2, 5, 7, 3, 1, 3, 1, 1),      # 1x3
    (2, 3, 7, 5, 4, 3, 1, 1, 0),      # 3x1: KW = 1
    (2, 2, 1, 9, 3, 1, 3, 1, 0),      # H = 1
    (1, 3, 9, 1, 2, 3, 1, 1, 0),      # W = 1
    (3, 2, 6, 6, 2, 2, 2, 1, 1),      # 2x2 s1 p1: odd 7x7 output
]
CONV_CASES = CONV_3X3_S1 + CONV_3X3_S2 + CONV_1X1 + CONV_4X4_S4 + CONV_GENERIC


def _family(case):
    KH, KW, s = case[5], case[6], case[7]
    for name, geo in (("3x3 s1", (3, 3, 1)), ("3x3 s2", (3, 3, 2)),
                      ("1x1", (1, 1, 1)), ("4x4 s4", (4, 4, 4))):
        if (KH, KW, s) == geo:
            return name
    return "generic"


def _case_id(case):
    return "b{}_ci{}_{}x{}_co{}_k{}x{}_s{}_p{}".format(*case)


def _gemm_dims(case):
    """(M, N, K) of the implicit GEMM of each direction"""
    B, Ci, H, W, Co, KH, KW, s, p = case
    OH, OW = R.conv_out_hw(H, W, KH, KW, s, p)
    return {"fwd": (Co, B * OH * OW, Ci * KH * KW),
            "bwd_data": (Ci, B * H * W, Co * KH * KW),
            "bwd_weight": (Co, Ci * KH * KW, B * OH * OW)}


def _mode(case, op):
    """plan_split's output mode: the split is matmul_f32's for one batch"""
    split = _native().matmul_f32_slab_count(1, *_gemm_dims(case)[op])
    return "store" if split == 1 else "atomics" if split == 2 else "slabs"


def _assert_direct(case):
    B, Ci, H, W, Co, KH, KW, s, p = case
    for op in ("fwd", "bwd_data", "bwd_weight"):
        route = _native().conv_route(op, B, Ci, H, W, Co, KH, s, p, KW)
        assert route == "direct", f"{_case_id(case)} {op} runs {route}"


def test_conv_cases_reach_every_output_mode():
    for cases in (CONV_3X3_S1, CONV_3X3_S2, CONV_1X1, CONV_4X4_S4, CONV_GENERIC):
        for op in ("fwd", "bwd_data", "bwd_weight"):
            modes = {_mode(c, op) for c in cases}
            assert modes == {"store", "atomics", "slabs"}, (_family(cases[0]), op, modes)
    for cases in (CONV_3X3_S1, CONV_3X3_S2, CONV_1X1, CONV_4X4_S4, CONV_GENERIC):
        ohow = set()
        for c in cases:
            OH, OW = R.conv_out_hw(c[2], c[3], c[5], c[6], c[7], c[8])
            ohow.add(OH * OW % 16 == 0)
        assert ohow == {True, False}, _family(cases[0])


def _conv_inputs(case, kind, seed):
    B, Ci, H, W, Co, KH, KW, s, p = case
    OH, OW = R.conv_out_hw(H, W, KH, KW, s, p)
    g = _gen(seed)
    return (_draw(kind, (B, Ci, H, W), g), _draw(kind, (Co, Ci, KH, KW), g),
            10 * _draw(kind, (Co,), g), _draw(kind, (B, Co, OH, OW), g))


def _conv_kernels(case, x, w, bias, gy):
    """the four kernels on device copies: y, gx, gw, gb"""
    B, Ci, H, W, Co, KH, KW, s, p = case
    n = _native()
    xd, wd, bd, gyd = (None if t is None else t.to(DEV) for t in (x, w, bias, gy))
    out = (n.conv2d_fwd(xd, wd, bd, s, p), n.conv2d_bwd_data(gyd, wd, s, p, H, W),
           n.conv2d_bwd_weight(gyd, xd, KH, KW, s, p), n.conv2d_bwd_bias(gyd))
    torch.cuda.synchronize()
    return out


def _conv_refs(case, x, w, bias, gy):
    B, Ci, H, W, Co, KH, KW, s, p = case
    return (R.conv2d(x, w, bias, s, p), R.conv2d_bwd_data(gy, w, s, p, H, W),
            R.conv2d_bwd_weight(gy, x, KH, KW, s, p), R.conv2d_bwd_bias(gy))


NAMES = ("fwd", "bwd_data", "bwd_weight", "bwd_bias")


@pytest.mark.parametrize("case", CONV_CASES, ids=_case_id)
def test_conv_exact(case):
    _assert_direct(case)
    x, w, bias, gy = _conv_inputs(case, "exact", 31)
    ours = _conv_kernels(case, x, w, bias, gy)
    for name, k, r in zip(NAMES, ours, _conv_refs(case, x, w, bias, gy)):
        exact(k, r, f"conv {_case_id(case)} {name}")
    y = _conv_kernels(case, x, w, None, gy)[0]
    exact(y, R.conv2d(x, w, None, case[7], case[8]), f"conv {_case_id(case)} fwd, no bias")


@pytest.mark.parametrize("case", CONV_CASES, ids=_case_id)
def test_conv_randn(case):
    _assert_direct(case)
    B, Ci, H, W, Co, KH, KW, s, p = case
    x, w, bias, gy = _conv_inputs(case, "randn", 32)
    ours = _conv_kernels(case, x, w, bias, gy)
    refs = _conv_refs(case, x, w, bias, gy)
    tx, tw, tb = (t.to(DEV).requires_grad_(True) for t in (x, w, bias))
    ty = F.conv2d(tx, tw, tb, stride=s, padding=p)
    ty.backward(gy.to(DEV))
    absrefs = _conv_refs(case, x.abs(), w.abs(), bias.abs(), gy.abs())
    dims = _gemm_dims(case)
    terms = [dims[op][2] for op in NAMES[:3]] + [dims["bwd_weight"][2]]
    family = "conv " + _family(case)
    for name, k, t, r, a, K in zip(NAMES, ours, (ty, tx.grad, tw.grad, tb.grad),
                                   refs, absrefs, terms):
        what = f"{_case_id(case)} {name}"
        cmp(family, what, k, t, r)
        _ceiling(family, what, k, r, a, K)


# ---------------- NaN locality (direct route) ----------------

NAN_CASES = [
    # case, (b0, c0, i, j) of the NaN in x, (b0, co0, i, j) of the NaN in gy
    ((2, 3, 5, 5, 65, 3, 3, 1, 1), (1, 2, 0, 0), (0, 64, 4, 4)),
    ((2, 3, 5, 5, 65, 3, 3, 1, 1), (0, 0, 2, 3), (1, 0, 0, 2)),
    ((2, 5, 7, 9, 17, 3, 3, 2, 1), (1, 4, 6, 8), (0, 16, 3, 0)),
    ((3, 33, 5, 5, 4, 1, 1, 1, 0), (2, 32, 4, 4), (1, 3, 0, 0)),
    ((2, 3, 8, 12, 65, 4, 4, 4, 0), (1, 0, 7, 11), (1, 1, 1, 2)),
    ((2, 3, 7, 8, 5, 3, 3, 3, 1), (1, 1, 0, 0), (0, 4, 2, 2)),
    ((2, 3, 5, 7, 4, 5, 5, 1, 2), (0, 2, 4, 0), (1, 3, 0, 6)),
]


@pytest.mark.parametrize("case,at_x,at_gy", NAN_CASES,
                         ids=[_case_id(c[0]) + f"_{k}" for k, c in enumerate(NAN_CASES)])
def test_conv_nan_stays_in_its_receptive_field(case, at_x, at_gy):
    """a NaN in x reaches exactly the outputs whose window covers it (its
    image, every co) and channel c0's taps of gw that touch it; a NaN in gy
    reaches exactly the inputs that output read.  The clamped address of an
    out-of-window load is (0, 0), so one case has the NaN there."""
    _assert_direct(case)
    B, Ci, H, W, Co, KH, KW, s, p = case
    x, w, bias, gy = _conv_inputs(case, "randn", 33)
    w[w == 0] = 1.0
    xn, gyn = x.clone(), gy.clone()
    xn[at_x] = NAN
    gyn[at_gy] = NAN
    b0, c0, i, j = at_x
    for k, r, name in zip(_conv_kernels(case, xn, w, bias, gy),
                          _conv_refs(case, xn, w, bias, gy), NAMES[:3]):
        if name == "bwd_data":
            assert not bool(torch.isnan(k).any()), "gx does not read x"
            continue
        mask = torch.isnan(r)
        assert bool(mask.any())
        if name == "fwd":
            assert not bool(mask[torch.arange(B) != b0].any())
            assert bool((mask == mask[:, :1]).all()), "every co alike"
        else:
            assert not bool(mask[:, torch.arange(Ci) != c0].any())
        assert torch.equal(torch.isnan(k).cpu(), mask), f"{name}: NaN placement"
    b0, co0 = at_gy[:2]
    gx, gw, gb = _conv_kernels(case, x, w, bias, gyn)[1:]
    rx, rw, rb = _conv_refs(case, x, w, bias, gyn)[1:]
    mask = torch.isnan(rx)
    assert bool(mask.any()) and not bool(mask[torch.arange(B) != b0].any())
    assert torch.equal(torch.isnan(gx).cpu(), mask), "bwd_data: NaN placement"
    mask = torch.isnan(rw)
    assert bool(mask[co0].any()) and not bool(mask[torch.arange(Co) != co0].any())
    assert torch.equal(torch.isnan(gw).cpu(), mask), "bwd_weight: NaN placement"
    assert torch.equal(torch.isnan(gb).cpu(), torch.isnan(rb)), "bwd_bias: NaN placement"


# ---------------- FastDiv's range ----------------

def _conv_1x1_single_channel(B):
    n = _native()
    g = _gen(41)
    x = torch.randint(-4, 5, (B, 1, 512, 512), generator=g).float()
    gy = torch.randint(-4, 5, (B, 1, 512, 512), generator=g).float()
    w = torch.tensor([[[[3.0]]]])
    assert n.conv_route("fwd", B, 1, 512, 512, 1, 1, 1, 0) == "direct"
    return n, x, gy, w


def test_conv_past_fastdiv_range_is_refused():
    """batch 17 of 512x512: the index 17 * 2^18 - 1 times the divisor 2^18 is
    past 2^40 (the first wrong quotient is at 4456447)"""
    n, x, gy, w = _conv_1x1_single_channel(17)
    x, gy, w = x.to(DEV), gy.to(DEV), w.to(DEV)
    with pytest.raises(RuntimeError, match="conv2d_fwd.*FastDiv"):
        n.conv2d_fwd(x, w, None, 1, 0)
    with pytest.raises(RuntimeError, match="conv2d_bwd_data.*FastDiv"):
        n.conv2d_bwd_data(gy, w, 1, 0, 512, 512)
    with pytest.raises(RuntimeError, match="conv2d_bwd_weight.*FastDiv"):
        n.conv2d_bwd_weight(gy, x, 1, 1, 1, 0)
    torch.cuda.synchronize()


def test_conv_at_fastdiv_range_is_exact():
    """batch 16: (16 * 2^18 - 1) * 2^18 = 2^40 - 2^18, the last batch in range.
    (bwd-weight sums 2^22 products; with this seed no partial sum of the
    signed terms comes near 2^24, so it is exact as well.)"""
    n, x, gy, w = _conv_1x1_single_channel(16)
    xd, gyd, wd = x.to(DEV), gy.to(DEV), w.to(DEV)
    y = n.conv2d_fwd(xd, wd, None, 1, 0)
    gx = n.conv2d_bwd_data(gyd, wd, 1, 0, 512, 512)
    gw = n.conv2d_bwd_weight(gyd, xd, 1, 1, 1, 0)
    torch.cuda.synchronize()
    exact(y, 3.0 * x.double(), "fwd")
    exact(gx, 3.0 * gy.double(), "bwd_data")
    exact(gw, (gy.double() * x.double()).sum().reshape(1, 1, 1, 1), "bwd_weight")


def test_batchnorm_and_maxpool_past_fastdiv_range_are_refused():
    """(1, 3, 1024, 1024): indices up to 3 * 2^20 - 1 divided by 2^20 (first
    wrong quotient at 2097151), under the 2^24 elements the ops used to admit"""
    n = _native()
    x = torch.zeros(1, 3, 1024, 1024, device=DEV)
    gamma, beta = torch.ones(3, device=DEV), torch.zeros(3, device=DEV)
    mean, invstd = torch.zeros(3, device=DEV), torch.ones(3, device=DEV)
    for relu, pool in ((False, False), (True, False)):
        with pytest.raises(RuntimeError, match="FastDiv"):
            n.bn2d_train_fwd(x, gamma, beta, None, None, None, 0.1, 1e-5, relu, pool)
    with pytest.raises(RuntimeError, match="FastDiv"):
        n.bn2d_fwd(x, mean, invstd, gamma, beta, False)
    for bwd in (n.bn2d_bwd, n.bn2d_bwd_eval, n.bn2d_train_bwd):
        with pytest.raises(RuntimeError, match="FastDiv"):
            bwd(x, x, gamma, mean, invstd)
    idx = torch.zeros(1, 3, 512, 512, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="maxpool2x2_bwd.*FastDiv"):
        n.maxpool2x2_bwd(x[:, :, :512, :512].contiguous(), idx, 1024, 1024)
    with pytest.raises(RuntimeError, match="maxpool2x2_fwd.*FastDiv"):
        n.maxpool2x2_fwd(torch.zeros(1, 2, 2048, 2048, device=DEV))
    torch.cuda.synchronize()


def test_maxpool_fwd_in_range_at_1024():
    """the forward on (1, 3, 1024, 1024) divides by 512 * 512: in range"""
    x = torch.randint(-99, 100, (1, 3, 1024, 1024), generator=_gen(42)).float()
    y, _ = _native().maxpool2x2_fwd(x.to(DEV))
    torch.cuda.synchronize()
    exact(y, R.maxpool2x2(x), "maxpool 1024")
