"""Paired conv backward: bwd-data and bwd-weight of one 3x3 stride-1 layer in
one launch (wino_bwd_pair_kernel) must give the bits of the two standalone
fused Winograd kernels, at the small shapes where the block -> (role, bx, by,
bz) decode and the merged slab reduce can go wrong.

Two comparisons per shape.  conv2d_bwd (the dispatcher Conv2dFn.backward
calls) against conv2d_bwd_data / conv2d_bwd_weight: at shapes the routing
table does not send to both fused kernels the dispatcher falls through, so
that comparison alone would not run the pair kernel there.  conv2d_bwd_pair
(the pair entry itself, both block assignments) against conv2d_wino_fused
(flip) / conv2d_wino_bwdw_fused runs it at every shape.

What each shape exercises is asserted from the split counts the extension
reports.  Two properties the shape list was meant to carry do not hold at its
shapes: at (2, 32, 8, 8, 64) and its swap both roles have 8 blocks (both
splits sit at their caps, which makes the counts equal), and at (6, 64, 8, 8,
64) the tile axis splits into 12 exact 8-tile slices.  (10, 192, 8, 8, 192)
is added for both: 240 vs 252 blocks, and a last tile slice of 16 of 24.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, Ci, H, W, Co), 3x3, stride 1, pad 1
SHAPES = [
    (2, 32, 8, 8, 64),
    (2, 64, 8, 8, 32),
    (4, 64, 16, 16, 128),
    (32, 512, 4, 4, 512),
    (6, 64, 8, 8, 64),
    (32, 64, 32, 32, 64),
    (10, 192, 8, 8, 192),
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _native():
    from split_learning_amd.ops.functional import native
    return native()


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    B, Ci, H, W, Co = shape
    g = torch.Generator(device="cuda").manual_seed(1234 + Ci + 7 * Co + H)
    gy = torch.randn(B, Co, H, W, device="cuda", generator=g)
    x = torch.randn(B, Ci, H, W, device="cuda", generator=g)
    w = torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) * 0.1
    return gy, x, w


@functools.lru_cache(maxsize=None)
def _standalone(shape):
    """gx, gw of the two standalone fused kernels (never modified)."""
    gy, x, w = _inputs(shape)
    n = _native()
    return (n.conv2d_wino_fused(gy, w, None, 1, True),
            n.conv2d_wino_bwdw_fused(gy, x, 1))


def _plan(shape):
    """(data splits, ci per slice, weight splits, tiles per slice, T, data
    blocks, weight blocks) from the extension's own split arithmetic."""
    B, Ci, H, W, Co = shape
    ds, ci_per, ws, t_per = _native().conv2d_bwd_pair_splits(B, Ci, H, W, Co, 1)
    T = B * (H // 2) * (W // 2)
    return ds, ci_per, ws, t_per, T, (T // 32) * (Ci // 32) * ds, \
        (Co // 32) * (Ci // 32) * ws


def test_shapes_exercise_what_they_are_for():
    ds, ci_per, ws, t_per, T, nd, nw = _plan((2, 32, 8, 8, 64))
    assert T == 32 and ds > 1 and ws > 1        # one tile column, both split
    ds2, _, ws2, _, T2, nd2, nw2 = _plan((2, 64, 8, 8, 32))
    assert T2 == 32 and ds2 > 1 and ws2 > 1 and ds2 != ds   # roles swapped
    ds, ci_per, ws, t_per, T, nd, nw = _plan((4, 64, 16, 16, 128))
    assert ds == 128 // 8 and ci_per == 8 and ws > 1        # data at its cap
    ds, ci_per, ws, t_per, T, nd, nw = _plan((32, 512, 4, 4, 512))
    assert ds == 4 and ws == 1                  # one reduce job, gw a view
    ds, ci_per, ws, t_per, T, nd, nw = _plan((6, 64, 8, 8, 64))
    assert T == 96 and ws == 12 and t_per == 8  # three tile columns
    ds, ci_per, ws, t_per, T, nd, nw = _plan((32, 64, 32, 32, 64))
    assert ds == 1 and nd == 512 and nw == 256  # 768 blocks, gx in place
    ds, ci_per, ws, t_per, T, nd, nw = _plan((10, 192, 8, 8, 192))
    assert nd != nw                             # role block counts differ
    assert ws * t_per > T and (T % t_per) % 8 == 0 and T % t_per != 0  # short slice
    assert ds * ci_per == 192 and ci_per > 8    # several K-steps per slice


@pytest.mark.parametrize("interleave", [0, 1], ids=["segregated", "interleaved"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pair_entry_equals_standalone_kernels(shape, interleave):
    gy, x, w = _inputs(shape)
    gx0, gw0 = _standalone(shape)
    gx, gw = _native().conv2d_bwd_pair(gy, x, w, 1, interleave)
    assert gx.shape == x.shape and gw.shape == w.shape
    assert torch.equal(gx, gx0)
    assert torch.equal(gw, gw0)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dispatcher_equals_separate_bindings(shape):
    B, Ci, H, W, Co = shape
    gy, x, w = _inputs(shape)
    n = _native()
    gx, gw = n.conv2d_bwd(gy, x, w, 1, 1, True, True)
    assert torch.equal(gx, n.conv2d_bwd_data(gy, w, 1, 1, H, W))
    assert torch.equal(gw, n.conv2d_bwd_weight(gy, x, 3, 3, 1, 1))


def test_dispatcher_pairs_the_flagship_shapes():
    """The two flagship shapes in the list take both fused routes, so the
    dispatcher comparison above ran the pair kernel for them."""
    n = _native()
    for (B, Ci, H, W, Co) in [(32, 512, 4, 4, 512), (32, 64, 32, 32, 64)]:
        assert n.conv_route("bwd_data", B, Ci, H, W, Co, 3, 1, 1) == "wino_fused"
        assert n.conv_route("bwd_weight", B, Ci, H, W, Co, 3, 1, 1) == "wino_bwdw_fused"


@pytest.mark.parametrize("shape", [(32, 512, 4, 4, 512), (4, 512, 2, 2, 512)],
                         ids=["pairable", "2x2"])
def test_dispatcher_fall_through(shape):
    B, Ci, H, W, Co = shape
    n = _native()
    gy, x, w = _inputs(shape)
    gx_ref = n.conv2d_bwd_data(gy, w, 1, 1, H, W)
    gw_ref = n.conv2d_bwd_weight(gy, x, 3, 3, 1, 1)
    gx, gw = n.conv2d_bwd(gy, x, w, 1, 1, True, False)
    assert gw is None and torch.equal(gx, gx_ref)
    gx, gw = n.conv2d_bwd(gy, x, w, 1, 1, False, True)
    assert gx is None and torch.equal(gw, gw_ref)
    gx, gw = n.conv2d_bwd(gy, x, w, 1, 1, False, False)
    assert gx is None and gw is None
    gx, gw = n.conv2d_bwd(gy, x, w, 1, 1, True, True)
    assert torch.equal(gx, gx_ref) and torch.equal(gw, gw_ref)


@pytest.mark.parametrize("shape", [(32, 512, 4, 4, 512), (32, 64, 32, 32, 64)],
                         ids=["512x4x4", "64x32x32"])
def test_conv2dfn_backward_against_torch(shape):
    """Tolerances are test_kernels_gpu.test_conv2d_bwd's."""
    from split_learning_amd.ops import functional as hf
    gy, x, w = _inputs(shape)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    F.conv2d(xr, wr, None, stride=1, padding=1).backward(gy)
    xn = x.clone().requires_grad_(True)
    wn = w.clone().requires_grad_(True)
    hf.conv2d(xn, wn, None, stride=1, padding=1).backward(gy)
    torch.testing.assert_close(xn.grad, xr.grad, atol=2e-3, rtol=2e-3)
    torch.testing.assert_close(wn.grad, wr.grad, atol=2e-2, rtol=2e-3)


def test_paired_backward_in_a_captured_graph():
    shape = (32, 512, 4, 4, 512)
    n = _native()
    gy0, x0, w0 = _inputs(shape)
    gy, x, w = gy0.clone(), x0.clone(), w0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        n.conv2d_bwd(gy, x, w, 1, 1, True, True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gx, gw = n.conv2d_bwd(gy, x, w, 1, 1, True, True)
    g = torch.Generator(device="cuda").manual_seed(77)
    for _ in range(2):
        for buf in (gy, x, w):
            buf.copy_(torch.randn(buf.shape, device="cuda", generator=g))
        graph.replay()
        torch.cuda.synchronize()
        ex, ew = n.conv2d_bwd(gy, x, w, 1, 1, True, True)
        assert torch.equal(gx, ex) and torch.equal(gw, ew)
