"""The float64 yardstick of tests/test_small_kernels_f64_gpu.py, checked on the
CPU against torch's own double-precision ops.  Both sides are float64, so
they agree to a few ulps of double; 1e-12 relative to the largest value leaves
room for a different summation order and nothing else."""

import pytest
import torch
import torch.nn.functional as F

import f64_reference as R


def _gen(seed=0):
    return torch.Generator(device="cpu").manual_seed(seed)


def _same(a, b, what, extra=0.0):
    """extra: an absolute allowance for an error of torch's own op"""
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()), 1.0)
    err = float((a - b).abs().max())
    assert err <= 1e-12 * scale + extra, (
        f"{what}: max |diff| {err:.3e}, scale {scale:.3e}")


@pytest.mark.parametrize("momentum,wd", [(0.5, 0.0), (0.0, 0.0), (0.9, 5e-4)])
def test_sgd(momentum, wd):
    g = _gen(1)
    p32 = torch.randn(37, generator=g)
    grads = [torch.randn(37, generator=g) for _ in range(3)]
    tp = p32.double().requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=0.1, momentum=momentum, weight_decay=wd,
                          foreach=False)
    p, buf = p32, torch.zeros(37)
    for k, gr in enumerate(grads):
        tp.grad = gr.double()
        opt.step()
        p, buf = R.sgd_step(p, gr, buf, 0.1, momentum, wd, k == 0)
        _same(p, tp, f"sgd p step {k}")
        if momentum:
            _same(buf, opt.state[tp]["momentum_buffer"], f"sgd buf step {k}")


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw(wd):
    g = _gen(2)
    p32 = torch.randn(37, generator=g)
    grads = [torch.randn(37, generator=g) for _ in range(3)]
    tp = p32.double().requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=1e-3, weight_decay=wd, foreach=False)
    p, m, v = p32, torch.zeros(37), torch.zeros(37)
    for k, gr in enumerate(grads, start=1):
        tp.grad = gr.double()
        opt.step()
        p, m, v = R.adamw_step(p, gr, m, v, k, 1e-3, 0.9, 0.999, 1e-8, wd)
        _same(p, tp, f"adamw p step {k}")
        _same(m, opt.state[tp]["exp_avg"], f"adamw m step {k}")
        _same(v, opt.state[tp]["exp_avg_sq"], f"adamw v step {k}")


def test_softmax_and_cross_entropy():
    g = _gen(3)
    x = torch.randn(9, 13, generator=g) * 20
    x[2, 5] = float("-inf")
    labels = torch.randint(0, 13, (9,), generator=g)
    labels[2] = 4
    xd = x.double().requires_grad_(True)
    y = F.softmax(xd, dim=-1)
    _same(R.softmax(x), y, "softmax")
    gy = torch.randn(9, 13, generator=g)
    y.backward(gy.double())
    _same(R.softmax_bwd(gy, R.softmax(x)), xd.grad, "softmax bwd")

    xd = x.double().requires_grad_(True)
    loss = F.cross_entropy(xd, labels)
    (3 * loss).backward()
    rl, rg = R.cross_entropy(x, labels, upstream=3.0)
    assert torch.isfinite(rl)
    _same(rl, loss, "ce loss")
    _same(rg, xd.grad, "ce grad")


@pytest.mark.parametrize("eps", [1e-12, 1e-5])
def test_layer_norm(eps):
    g = _gen(4)
    x = 1000 + torch.randn(5, 33, generator=g)
    gamma, beta = torch.randn(33, generator=g), torch.randn(33, generator=g)
    gy = torch.randn(5, 33, generator=g)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.layer_norm(xd, (33,), gd, bd, eps=eps)
    y.backward(gy.double())
    ry, mean, invstd = R.layer_norm(x, gamma, beta, eps)
    _same(ry, y, "ln y")
    _same(mean, x.double().mean(dim=-1), "ln mean")
    _same(invstd, (x.double().var(dim=-1, unbiased=False) + eps).rsqrt(), "ln invstd")
    gx, dgamma, dbeta = R.layer_norm_bwd(gy, x, gamma, eps)
    # gx cancels terms of size |gy| * invstd; its own rounding scales with that
    _same(gx / float(invstd.max()), xd.grad / float(invstd.max()), "ln gx")
    _same(dgamma, gd.grad, "ln dgamma")
    _same(dbeta, bd.grad, "ln dbeta")


@pytest.mark.parametrize("offset", [0.3, 1000.0])
def test_batch_norm(offset):
    g = _gen(5)
    x = offset + 1.5 * torch.randn(4, 3, 5, 6, generator=g)
    gamma, beta = torch.randn(3, generator=g), torch.randn(3, generator=g)
    rm0, rv0 = torch.randn(3, generator=g), torch.rand(3, generator=g) + 0.5
    gy = torch.randn(4, 3, 5, 6, generator=g)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = rm0.double(), rv0.double()
    y = F.batch_norm(xd, rm, rv, gd, bd, training=True, momentum=0.1, eps=1e-5)
    y.backward(gy.double())
    ry, mean, invstd, rrm, rrv = R.batch_norm_train(x, gamma, beta, rm0, rv0, 0.1, 1e-5)
    # torch's double op may lose mean^2 * eps64 (relative to a variance of ~2)
    # in its variance; everything that depends on it gets that allowance
    # times the largest value and a factor 16 for how the error spreads
    lost = 16 * offset * offset * 2.0 ** -52

    def same_var(a, b, what):
        _same(a, b, what, extra=lost * max(float(b.detach().abs().max()), 1.0))

    same_var(ry, y, "bn y")
    _same(mean, x.double().mean(dim=(0, 2, 3)), "bn mean")
    same_var(invstd, (x.double().var(dim=(0, 2, 3), unbiased=False) + 1e-5).rsqrt(),
             "bn invstd")
    _same(rrm, rm, "bn running_mean")
    same_var(rrv, rv, "bn running_var")
    gx, gg, gb = R.batch_norm_train_bwd(gy, x, gamma, 1e-5)
    same_var(gx, xd.grad, "bn gx")
    same_var(gg, gd.grad, "bn ggamma")
    _same(gb, bd.grad, "bn gbeta")
    ye = F.batch_norm(x.double(), rm0.double(), rv0.double(), gamma.double(),
                      beta.double(), training=False, eps=1e-5)
    _same(R.batch_norm_eval(x, gamma, beta, rm0, rv0, 1e-5), ye, "bn eval")


def test_activations():
    x = torch.cat([torch.linspace(-12, 12, 97),
                   torch.tensor([0.0, -0.0, 1e-45, 10.0, -10.0, 20.0, -20.0])])
    gy = torch.randn(x.numel(), generator=_gen(6))
    for name, ref, ref_bwd, op in (
            ("relu", R.relu, R.relu_bwd, F.relu),
            ("gelu", R.gelu, R.gelu_bwd, F.gelu),
            ("tanh", R.tanh, R.tanh_bwd, torch.tanh)):
        xd = x.double().requires_grad_(True)
        y = op(xd)
        y.backward(gy.double())
        _same(ref(x), y, name)
        _same(ref_bwd(gy, x), xd.grad, name + " bwd")
    inf = torch.tensor([float("inf"), float("-inf"), float("nan")])
    for ref, op in ((R.relu, F.relu), (R.gelu, F.gelu), (R.tanh, torch.tanh)):
        a, b = ref(inf), op(inf.double())
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])


def test_maxpool():
    g = _gen(7)
    for shape in [(1, 1, 2, 2), (2, 3, 7, 7), (2, 3, 6, 9)]:
        x = torch.randint(-3, 4, shape, generator=g).float()
        assert torch.equal(R.maxpool2x2(x), F.max_pool2d(x.double(), 2, 2))


@pytest.mark.parametrize("padding_idx", [None, 0, 10])
def test_embedding(padding_idx):
    g = _gen(8)
    w = torch.randn(11, 5, generator=g)
    ids = torch.randint(0, 11, (4, 7), generator=g)
    wd = w.double().requires_grad_(True)
    y = F.embedding(ids, wd, padding_idx=padding_idx)
    gy = torch.randn(4, 7, 5, generator=g)
    y.backward(gy.double())
    assert torch.equal(R.embedding(ids, w), y.detach())
    _same(R.embedding_bwd(ids, gy, 11, padding_idx), wd.grad, "embedding gw")
