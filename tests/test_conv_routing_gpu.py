"""Pins which kernel each conv shape runs (ops/csrc/conv_route.h).

conv_route() only evaluates the routing table the conv wrappers switch on; it
launches nothing.  The expected names were generated from the routing
predicates as they stood BEFORE they were gathered into conv_route.h, so a
change to any rule shows up here as a named shape instead of as a slower
benchmark.  The table is for the default SLK_WINO level (1).
"""

import os

import pytest

pytestmark = pytest.mark.gpu

OPS = ("fwd", "bwd_data", "bwd_weight")

# ((B, Ci, H, W, Co, K, stride, pad), fwd, bwd_data, bwd_weight)
ROUTES = [
    # the nine VGG16 conv shapes at B = 32 (tools/conv_microbench.py SHAPES)
    ((32, 3, 32, 32, 64, 3, 1, 1), "direct", "direct", "wino_bwdw"),
    ((32, 64, 32, 32, 64, 3, 1, 1), "wino_fused", "wino_fused", "wino_bwdw_fused"),
    ((32, 64, 16, 16, 128, 3, 1, 1), "wino_fused", "wino_fused", "wino_bwdw_fused"),
    ((32, 128, 16, 16, 128, 3, 1, 1), "wino_fused", "wino_fused", "wino_bwdw_fused"),
    ((32, 128, 8, 8, 256, 3, 1, 1), "direct", "wino_fused", "wino_bwdw_fused"),
    ((32, 256, 8, 8, 256, 3, 1, 1), "wino", "wino_fused", "wino_bwdw_fused"),
    ((32, 256, 4, 4, 512, 3, 1, 1), "direct", "wino_fused", "wino_bwdw_fused"),
    ((32, 512, 4, 4, 512, 3, 1, 1), "wino", "wino_fused", "wino_bwdw_fused"),
    ((32, 512, 2, 2, 512, 3, 1, 1), "wino", "wino", "wino_bwdw_fused"),
    # CONV_CASES of tests/test_kernels_gpu.py
    ((4, 3, 32, 32, 64, 3, 1, 1), "direct", "direct", "wino_bwdw"),
    ((4, 64, 32, 32, 64, 3, 1, 1), "wino", "wino_fused", "wino_bwdw_fused"),
    ((4, 64, 16, 16, 128, 3, 1, 1), "direct", "direct", "wino_bwdw_fused"),
    ((4, 256, 4, 4, 512, 3, 1, 1), "direct", "direct", "wino_bwdw_fused"),
    ((4, 512, 2, 2, 512, 3, 1, 1), "wino", "wino", "wino_bwdw_fused"),
    ((4, 64, 16, 16, 128, 1, 1, 0), "direct", "direct", "direct"),
    ((4, 64, 16, 16, 64, 3, 2, 1), "direct", "direct", "direct"),
    ((4, 3, 32, 32, 128, 4, 4, 0), "direct", "direct", "direct"),
    # odd output sizes: no Winograd form is legal
    ((2, 8, 5, 7, 16, 3, 1, 1), "direct", "direct", "direct"),
    # channels not a multiple of 32: unfused bwd-weight territory
    ((8, 24, 8, 8, 24, 3, 1, 1), "direct", "direct", "wino_bwdw"),
]


def test_routes_cover_the_listed_shapes():
    from test_kernels_gpu import CONV_CASES
    shapes = [r[0] for r in ROUTES]
    for case in CONV_CASES:
        assert tuple(case) in shapes, case


@pytest.mark.parametrize("shape,fwd,bwd_data,bwd_weight", ROUTES)
def test_conv_route(shape, fwd, bwd_data, bwd_weight):
    from split_learning_amd.ops import native
    ext = native()
    got = tuple(ext.conv_route(op, *shape) for op in OPS)
    assert got == (fwd, bwd_data, bwd_weight), (
        f"{shape}: routes {dict(zip(OPS, got))} at "
        f"SLK_WINO={os.environ.get('SLK_WINO', '1 (default)')}")


def test_conv_route_rejects_unknown_op():
    from split_learning_amd.ops import native
    with pytest.raises(RuntimeError):
        native().conv_route("bwd", 4, 64, 16, 16, 64, 3, 1, 1)
