"""The bf16-operand MFMA GEMM (csrc/gemm_bf16.hip) behind hf.linear(...,
compute="bf16") and hf.lora_linear(..., compute="bf16").

The operation is defined as: round both operands to bf16 (nearest even),
multiply and sum exactly.  In float64 on the CPU that is
op(a.bfloat16().double()) @ op(b.bfloat16().double()) (+ bias in double).
bf16 x bf16 products are exact in fp32, so the kernel is an fp32 sum of R exact
terms in some order and |kernel - ref| <= (R + 1) * 2^-23 * (|a_bf16| @ |b_bf16|)
element by element: f64_compare._ceiling at terms=R.  A product that skipped
the rounding is far outside that bound, so the comparison also shows that the
bf16 route ran.

Tiles are 128x128, 64x128 and 64x64 with 32 of the reduction per LDS stage;
the host rule takes the largest whose grid reaches 512 blocks (the weight
gradient counts the slabs it may split its reduction over M into, one per
four stages), and splits that reduction once it has 8 stages.
"""

import pytest
import torch

from f64_compare import _ceiling, _draw, _gen, exact
from split_learning_amd.ops import functional as hf

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bf(t):
    return t.detach().cpu().bfloat16().double()


def run_linear(x, w, b, gy, **kw):
    """leaves on the GPU, one forward and backward -> (y, gx, gW, gb)"""
    x, w = (t.to(DEV).requires_grad_() for t in (x, w))
    b = None if b is None else b.to(DEV).requires_grad_()
    y = hf.linear(x, w, b, **kw)
    y.backward(gy.to(DEV))
    return y, x.grad, w.grad, None if b is None else b.grad


# (M, N, K): a single row; odd M below a tile; one row and 8 columns past the
# 64 tile; past 128 both ways; K not a multiple of the stage; odd M whose
# weight gradient splits into two slabs (9 stages) with a ragged last stage;
# the 64x128 forward tile by the rule (544 blocks; its weight gradient takes
# 64x128 in 8 slabs), then the 128x128 one (576 blocks); the rest is 64x64
SHAPES = [(1, 8, 8), (33, 40, 24), (65, 72, 40), (130, 136, 72),
          (64, 128, 264), (257, 72, 520), (2041, 2056, 40), (2945, 2952, 8)]


@pytest.mark.parametrize("shape,bias", [(s, True) for s in SHAPES]
                         + [(SHAPES[0], False), (SHAPES[3], False)])
def test_ceiling(shape, bias):
    (M, N, K), g = shape, _gen(sum(shape))
    x, w, gy = (_draw("randn", s, g) for s in ((M, K), (N, K), (M, N)))
    b = _draw("randn", (N,), g) if bias else None
    y, gx, gw, gb = run_linear(x, w, b, gy, compute="bf16")
    xb, wb, gb16 = bf(x), bf(w), bf(gy)
    what = f"{shape} bias={bias}"
    if bias:
        _ceiling("bf16", f"y {what}", y, xb @ wb.T + b.double(),
                 xb.abs() @ wb.abs().T + b.double().abs(), terms=K + 1)
        _ceiling("bf16", f"gb {what}", gb, gy.double().sum(0),
                 gy.double().abs().sum(0), terms=M)
    else:
        _ceiling("bf16", f"y {what}", y, xb @ wb.T, xb.abs() @ wb.abs().T,
                 terms=K)
    _ceiling("bf16", f"gx {what}", gx, gb16 @ wb, gb16.abs() @ wb.abs(),
             terms=N)
    _ceiling("bf16", f"gW {what}", gw, gb16.T @ xb, gb16.abs().T @ xb.abs(),
             terms=M)


@pytest.mark.parametrize("tile", [None, 0, 1, 2])
@pytest.mark.parametrize("shape", [(130, 136, 264), (257, 72, 40)])
def test_exact(shape, tile):
    """integers from [-4, 4] are bf16 numbers and every sum is an integer
    below 2^24: all three products must be the integer result, through the
    rule's tile (autograd, tile=None) and through each tile by name"""
    (M, N, K), g = shape, _gen(7 + sum(shape))
    x, w, gy = (_draw("exact", s, g) for s in ((M, K), (N, K), (M, N)))
    if tile is None:
        y, gx, gw, _ = run_linear(x, w, None, gy, compute="bf16")
    else:
        ext, (xd, wd, gd) = hf.native(), (t.to(DEV) for t in (x, w, gy))
        y = ext.linear_bf16_fwd(xd, wd, None, tile)
        gx = ext.linear_bf16_bwd_input(gd, wd, tile)
        gw = ext.linear_bf16_bwd_weight(gd, xd, tile)
    x, w, gy = x.double(), w.double(), gy.double()
    exact(y, (x @ w.T).float(), f"y {shape} tile {tile}")
    exact(gx, (gy @ w).float(), f"gx {shape} tile {tile}")
    exact(gw, (gy.T @ x).float(), f"gW {shape} tile {tile}")


def test_rounding_and_specials():
    """W = I at (8, 8, 8), one value per row of x on the diagonal, so
    y = bf16(x) wherever the row is finite: 1+2^-8 is a tie and goes to the
    even 1.0, 1+3*2^-8 is a tie and goes to 1.015625, 1+2^-8+2^-20 goes up,
    0x7f7f7fff (the largest fp32 below the bf16 overflow threshold) stays
    finite.  The +inf row and the NaN row must be NaN in every column (the
    rest of W's row is zero and 0 * inf = 0 * NaN = NaN) except +inf on the
    inf row's diagonal: exactly where the float64 reference has them.  No
    other row is touched."""
    big = torch.tensor(0x7F7F7FFF, dtype=torch.int32).view(torch.float32)
    vals = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20,
            float(big), float("inf"), float("nan"), -3.0, 0.0]
    x = torch.diag(torch.tensor(vals, dtype=torch.float32))
    w = torch.eye(8)
    y = hf.linear(x.to(DEV), w.to(DEV), None, compute="bf16")
    exact(y, (bf(x) @ bf(w).T).float(), "specials against float64")
    fin = [0, 1, 2, 3, 6, 7]
    exact(y[fin], x.bfloat16().float()[fin], "y == bf16(x) on finite rows")
    assert y[0, 0] == 1.0 and y[1, 1] == 1.015625 and y[2, 2] == 1.0078125
    assert torch.isfinite(y[3, 3]) and y[4, 4] == float("inf")


def test_precondition_and_routing():
    g = _gen(3)
    x, w = _draw("randn", (16, 24), g).to(DEV), _draw("randn", (8, 24), g).to(DEV)
    assert hf.linear_bf16_ok(x, w)
    bad = [(x[:, :20].contiguous(), w[:, :20].contiguous()),   # K % 8
           (x, w[:4].contiguous()),                            # N = 4
           (x[:, :8], w[:, :8]),                               # strided weight
           (x.cpu(), w.cpu())]                                 # CPU
    for xx, ww in bad:
        assert not hf.linear_bf16_ok(xx, ww)
        with pytest.raises(ValueError):
            hf.linear(xx, ww, None, compute="bf16")
    # no compute argument: today's routes, above and below the BLAS threshold
    w, b = _draw("randn", (256, 64), g).to(DEV), _draw("randn", (256,), g).to(DEV)
    for m in (16, 1024):
        assert (2.0 * m * 256 * 64 >= hf._LIB_LIN_THRESH) == (m == 1024)
        xs = _draw("randn", (m, 64), g).to(DEV)
        exact(hf.linear(xs, w, b), hf.linear(xs, w, b, compute="fp32"),
              f"default route M={m}")


def test_lora():
    """Base product and g @ W on the bf16 kernels, the adapter in fp32: out
    and x.grad against the double formula with x, W (and g for x.grad)
    rounded in the base term only, at terms = K + r + 2 over the magnitude
    sum of the same formula.  A.grad and B.grad must have the fp32
    call's bits: lora_bwd forms them from g, x, xa and gxa = scaling * g B and
    only adds into gx, whose contents it never reads into gA or gB."""
    (M, N, K), r, sc, g = (130, 72, 40), 8, 2.0, _gen(11)
    x, w, a, b, gy = (_draw("randn", s, g)
                      for s in ((M, K), (N, K), (r, K), (N, r), (M, N)))
    res = {}
    for compute in ("bf16", "fp32"):
        xd, ad, bd = (t.to(DEV).requires_grad_() for t in (x, a, b))
        out = hf.lora_linear(xd, w.to(DEV), None, ad, bd, sc, compute=compute)
        out.backward(gy.to(DEV))
        res[compute] = (out, xd.grad, ad.grad, bd.grad)
    out, gx, ga, gb = res["bf16"]
    x64, a64, b64, g64 = (t.double() for t in (x, a, b, gy))
    _ceiling("bf16", "lora out", out,
             bf(x) @ bf(w).T + sc * (x64 @ a64.T @ b64.T),
             bf(x).abs() @ bf(w).abs().T
             + sc * (x64.abs() @ a64.abs().T @ b64.abs().T), terms=K + r + 2)
    _ceiling("bf16", "lora gx", gx, bf(gy) @ bf(w) + sc * (g64 @ b64 @ a64),
             bf(gy).abs() @ bf(w).abs()
             + sc * (g64.abs() @ b64.abs() @ a64.abs()), terms=K + r + 2)
    exact(ga, res["fp32"][2], "lora A.grad")
    exact(gb, res["fp32"][3], "lora B.grad")
