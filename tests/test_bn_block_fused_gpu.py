"""Fused BatchNorm block: single-launch training BN for one-chunk layers and
BN -> ReLU -> MaxPool2d(2,2) as one op.

The fused kernels accumulate the same elements in the same order as the
separate-launch kernels and share their per-element expressions, so the first
group of tests demands exact equality (torch.equal) against the composition of
the pre-existing bindings (bn2d_stats_fused, bn2d_fwd, maxpool2x2_fwd,
maxpool2x2_bwd, bn2d_bwd).  Parity with torch uses the tolerances of
tests/test_kernels_gpu.py::test_bn2d_train_fwd_bwd.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MOM, EPS = 0.1, 1e-5


def _native():
    from split_learning_amd.ops import native
    return native()


def _state(C):
    return (torch.linspace(-0.5, 0.5, C, device="cuda"),
            torch.linspace(0.5, 1.5, C, device="cuda"),
            torch.tensor(3, dtype=torch.long, device="cuda"))


def _unfused(x, gamma, beta, gy, relu, pool):
    """stats, apply, pool as separate launches; pool backward scatters the
    pooled gradient to full resolution before the BN backward."""
    n = _native()
    rm, rv, nbt = _state(x.shape[1])
    mean, invstd = n.bn2d_stats_fused(x, rm, rv, nbt, MOM, EPS)
    y_full = n.bn2d_fwd(x, mean, invstd, gamma, beta, relu)
    y, g_full = y_full, gy
    if pool:
        y, idx = n.maxpool2x2_fwd(y_full)
        g_full = n.maxpool2x2_bwd(gy, idx, x.shape[2], x.shape[3])
    gx, gg, gb = n.bn2d_bwd(x, g_full, gamma, mean, invstd,
                            y_full if relu else None)
    return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv,
                num_batches_tracked=nbt, gx=gx, ggamma=gg, gbeta=gb)


def _fused(x, gamma, beta, gy, relu, pool):
    n = _native()
    rm, rv, nbt = _state(x.shape[1])
    out = n.bn2d_train_fwd(x, gamma, beta, rm, rv, nbt, MOM, EPS, relu, pool)
    y, mean, invstd = out[:3]
    idx = out[3] if pool else None
    gx, gg, gb = n.bn2d_train_bwd(x, gy, gamma, mean, invstd,
                                  y if relu else None, idx)
    return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv,
                num_batches_tracked=nbt, gx=gx, ggamma=gg, gbeta=gb)


def _assert_same(a, b):
    for k in a:
        assert a[k].shape == b[k].shape, k
        if not torch.equal(a[k], b[k]):
            d = (a[k].double() - b[k].double()).abs()
            raise AssertionError(
                f"{k}: {int((d > 0).sum())} of {d.numel()} elements differ, "
                f"max |diff| {float(d.max()):.3e}")


def _inputs(shape, pool, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, C, H, W = shape
    x = (torch.randn(shape, generator=g) * 1.5 + 0.3).cuda()
    gamma = (torch.randn(C, generator=g) * 0.5 + 1.0).cuda()
    beta = (torch.randn(C, generator=g) * 0.3).cuda()
    gshape = (B, C, H // 2, W // 2) if pool else shape
    gy = torch.randn(gshape, generator=g).cuda()
    return x, gamma, beta, gy


# [2,3,2,2] fewer elements than threads; [8,32,16,16] one-kernel path, 8 per
# thread; 8191 / 8192 the last one-kernel and the first chunked size;
# [32,5,16,16] two chunks; [4,3,4,6] H != W
EXACT_CASES = [
    ((2, 3, 2, 2), True, False), ((2, 3, 2, 2), True, True),
    ((8, 32, 16, 16), False, False), ((8, 32, 16, 16), True, False),
    ((8, 32, 16, 16), True, True),
    ((1, 2, 1, 8191), True, False), ((1, 2, 1, 8192), True, False),
    ((32, 5, 16, 16), True, False), ((32, 5, 16, 16), True, True),
    ((4, 3, 4, 6), True, False), ((4, 3, 4, 6), True, True),
]


@pytest.mark.parametrize("shape,relu,pool", EXACT_CASES)
def test_fused_equals_unfused_exactly(shape, relu, pool):
    x, gamma, beta, gy = _inputs(shape, pool)
    _assert_same(_fused(x, gamma, beta, gy, relu, pool),
                 _unfused(x, gamma, beta, gy, relu, pool))


@pytest.mark.parametrize("shape", [(4, 3, 4, 4), (32, 3, 16, 16)])
def test_crafted_channels(shape):
    """channel 0: beta strongly negative -> every 2x2 window is zero after
    ReLU, pooled output and every gradient of the channel are 0; channel 1:
    constant input -> zero variance.  Both shapes: one-kernel and chunked."""
    x, gamma, beta, gy = _inputs(shape, True, seed=1)
    beta[0] = -100.0
    x[:, 1] = 2.5
    f = _fused(x, gamma, beta, gy, True, True)
    _assert_same(f, _unfused(x, gamma, beta, gy, True, True))
    assert not f["y"][:, 0].any()
    assert not f["gx"][:, 0].any()
    assert float(f["ggamma"][0]) == 0.0 and float(f["gbeta"][0]) == 0.0
    assert float(f["invstd"][1]) == pytest.approx(EPS ** -0.5, rel=1e-5)
    assert torch.isfinite(f["gx"]).all() and torch.isfinite(f["y"]).all()


def _close(a, b, tol, what):
    torch.testing.assert_close(a, b, atol=tol, rtol=tol,
                               msg=lambda m: f"{what}: {m}")


def _torch_block(x, gamma, beta, rm, rv, pool=True):
    y = F.relu(F.batch_norm(x, rm, rv, gamma, beta, training=True,
                            momentum=MOM, eps=EPS))
    return F.max_pool2d(y, 2, 2) if pool else y


def _leaves(x, gamma, beta):
    return [t.detach().clone().requires_grad_(True) for t in (x, gamma, beta)]


@pytest.mark.parametrize("shape", [(8, 32, 16, 16), (32, 4, 32, 32)])
def test_parity_with_torch(shape):
    from split_learning_amd.ops import functional as hf
    torch.manual_seed(0)
    C = shape[1]
    x = torch.randn(shape, device="cuda")
    gamma = torch.randn(C, device="cuda")
    beta = torch.randn(C, device="cuda")
    x1, g1, b1 = _leaves(x, gamma, beta)
    x2, g2, b2 = _leaves(x, gamma, beta)
    rm1, rv1 = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    rm2, rv2 = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    y = hf.bn_relu_maxpool2x2(x1, g1, b1, rm1, rv1, MOM, EPS)
    yref = _torch_block(x2, g2, b2, rm2, rv2)
    _close(y, yref, 1e-4, "y")
    _close(rm1, rm2, 1e-4, "running_mean")
    _close(rv1, rv2, 1e-4, "running_var")
    gy = torch.randn_like(y)
    y.backward(gy)
    yref.backward(gy)
    _close(x1.grad, x2.grad, 1e-4, "gx")
    _close(g1.grad, g2.grad, 1e-3, "ggamma")
    _close(b1.grad, b2.grad, 1e-3, "gbeta")


# ---------------- routing ----------------

def _triple_cls():
    from split_learning_amd.models.partitioned import SequentialUnits
    from split_learning_amd.ops.modules import (HipBatchNorm2d, HipMaxPool2d,
                                                HipReLU)

    class Triple(SequentialUnits):
        TOTAL_UNITS = 3

        @classmethod
        def unit_factories(cls):
            return {1: lambda: HipBatchNorm2d(3), 2: lambda: HipReLU(),
                    3: lambda: HipMaxPool2d(kernel_size=2, stride=2)}

    return Triple


def _run_against_torch(models, shape):
    """forward+backward through the chained partition(s) vs the torch block;
    returns the grad_fn type names of each partition's output."""
    torch.manual_seed(2)
    x = torch.randn(shape, device="cuda")
    bn = models[0].layer1
    with torch.no_grad():
        bn.weight.copy_(torch.randn(3) * 0.5 + 1.0)
        bn.bias.copy_(torch.randn(3) * 0.3)
    x1 = x.clone().requires_grad_(True)
    x2, g2, b2 = _leaves(x, bn.weight, bn.bias)
    rm2, rv2 = torch.zeros(3, device="cuda"), torch.ones(3, device="cuda")
    names, y = [], x1
    for m in models:
        y = m(y)
        names.append(type(y.grad_fn).__name__)
    yref = _torch_block(x2, g2, b2, rm2, rv2)
    _close(y, yref, 1e-4, "y")
    _close(bn.running_mean, rm2, 1e-4, "running_mean")
    _close(bn.running_var, rv2, 1e-4, "running_var")
    assert int(bn.num_batches_tracked) == 1
    gy = torch.randn_like(y)
    y.backward(gy)
    yref.backward(gy)
    _close(x1.grad, x2.grad, 1e-4, "gx")
    _close(bn.weight.grad, g2.grad, 1e-3, "ggamma")
    _close(bn.bias.grad, b2.grad, 1e-3, "gbeta")
    return names


def test_routing_triple_runs_fused_op():
    m = _triple_cls()(0, 3).cuda().train()
    assert _run_against_torch([m], (4, 3, 6, 8)) == ["BnReluPool2x2FnBackward"]


def test_routing_odd_size_falls_back():
    m = _triple_cls()(0, 3).cuda().train()
    assert _run_against_torch([m], (2, 3, 5, 7)) == ["MaxPool2x2FnBackward"]


def test_routing_eval_mode_falls_back():
    m = _triple_cls()(0, 3).cuda().eval()
    x = torch.randn(2, 3, 4, 4, device="cuda", requires_grad=True)
    y = m(x)
    assert type(y.grad_fn).__name__ == "MaxPool2x2FnBackward"
    ref = F.max_pool2d(F.relu(F.batch_norm(
        x, m.layer1.running_mean, m.layer1.running_var, m.layer1.weight,
        m.layer1.bias, training=False, eps=EPS)), 2, 2)
    _close(y, ref, 1e-4, "eval y")


def test_routing_cut_between_relu_and_pool():
    T = _triple_cls()
    a, b = T(0, 2).cuda().train(), T(2, 3).cuda().train()
    assert _run_against_torch([a, b], (4, 3, 6, 8)) == [
        "BatchNorm2dFnBackward", "MaxPool2x2FnBackward"]


# ---------------- graph capture ----------------

def test_graph_capture_replays_equal_eager():
    from split_learning_amd.ops import functional as hf
    shape, C = (8, 16, 8, 8), 16
    g = torch.Generator(device="cpu").manual_seed(5)
    gamma = (torch.randn(C, generator=g) * 0.5 + 1.0).cuda().requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.3).cuda().requires_grad_(True)
    gy = torch.randn(8, C, 4, 4, generator=g).cuda()
    inputs = [torch.randn(shape, generator=g).cuda() for _ in range(3)]
    static_x = inputs[0].clone()

    def step(xbuf, rm, rv, nbt):
        xin = xbuf.detach().requires_grad_(True)
        y = hf.bn_relu_maxpool2x2(xin, gamma, beta, rm, rv, MOM, EPS, nbt)
        return (y,) + torch.autograd.grad(y, (xin, gamma, beta), gy)

    rm, rv, nbt = _state(C)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(static_x, rm, rv, nbt)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step(static_x, rm, rv, nbt)
    torch.cuda.synchronize()
    # eager twin state starts where the graph's state stands now
    rm_e, rv_e, nbt_e = rm.clone(), rv.clone(), nbt.clone()
    nbt0 = int(nbt)
    for k, xin in enumerate(inputs[1:], start=1):
        static_x.copy_(xin)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(xin, rm_e, rv_e, nbt_e)
        for name, a, b in zip(("y", "gx", "ggamma", "gbeta"), static_out, eager):
            assert torch.equal(a, b), f"replay {k}: {name}"
        assert torch.equal(rm, rm_e) and torch.equal(rv, rv_e), f"replay {k}"
        assert int(nbt) == nbt0 + k == int(nbt_e)
