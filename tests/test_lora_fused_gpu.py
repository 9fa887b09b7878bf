"""Fused LoRA adapter (lora.hip) against the formula in float64 on the CPU:

    out = x W^T + b + s * (dropout(x) A^T) B^T

forward and the gradients autograd takes through LoraLinearFn, by
f64_compare.cmp with the same formula in fp32 torch on the GPU as yardstick.
lora_B is drawn random everywhere: its zero init hides the adapter.
"""

import pytest
import torch

from f64_compare import cmp, cpu64

pytestmark = pytest.mark.gpu

S = 2.0     # alpha / r of the BERT adapters
P = 0.1


def _hf():
    from split_learning_amd.ops import functional as hf
    return hf


def _inputs(M, K, N, r, seed=0):
    """x, W, b, A, B, g"""
    g = torch.Generator().manual_seed(seed + M + K)
    return [torch.randn(s, generator=g)
            for s in ((M, K), (N, K), (N,), (r, K), (N, r), (M, N))]


def _formula(x, W, b, A, B, keep=None):
    xd = x if keep is None else x * keep.to(x) / (1 - P)
    y = x @ W.t() if b is None else x @ W.t() + b
    return y + S * ((xd @ A.t()) @ B.t())


def _fwd_bwd(fn, ts, g, req):
    """[out, grads of the leaves that ask] of fn on fresh leaves"""
    leaves = [None if t is None else t.detach().clone().requires_grad_(rq)
              for t, rq in zip(ts, req)]
    out = fn(*leaves)
    out.backward(g.to(out))
    return out, [out.detach()] + [l.grad for l, rq in zip(leaves, req) if rq]


NAMES = ("gx", "gW", "gb", "gA", "gB")
DEFAULT = (True, False, False, True, True)


def _check(what, ts, g, req=DEFAULT, keep=None):
    """the fused route's out and gradients against float64, cmp's rule"""
    p = 0.0 if keep is None else P
    fn = lambda *a: _hf().lora_linear(*a, S, p, True)  # noqa: E731
    dev = [None if t is None else t.cuda() for t in ts]
    out, ours = _fwd_bwd(fn, dev, g.cuda(), req)
    ref = _fwd_bwd(lambda *a: _formula(*a, keep=keep),
                   [None if t is None else t.double() for t in ts], g.double(),
                   req)[1]
    kd = None if keep is None else keep.cuda()
    yard = _fwd_bwd(lambda *a: _formula(*a, keep=kd), dev, g.cuda(), req)[1]
    names = ["out"] + [n for n, rq in zip(NAMES, req) if rq]
    for name, o, y, r in zip(names, ours, yard, ref, strict=True):
        assert cpu64(r).abs().max() > 0
        cmp("lora", f"{what} {tuple(ts[0].shape)} r={ts[3].shape[0]} {name}",
            o, y, r)
    return out


def _two_slab_m(K, N):
    """smallest M whose weight-gradient grid has two slabs, plus 3: the last
    slab is ragged"""
    slabs = _hf().native().lora_wgrad_slabs
    return next(m for m in range(1, 4096) if slabs(m, K, N) >= 2) + 3


ALL = (True,) * 5
CASES = [(5, 4, 4, 1, "plain", DEFAULT), (18, 32, 72, 8, "plain", DEFAULT),
         (33, 768, 64, 8, "plain", DEFAULT), (None, 72, 32, 16, "plain", DEFAULT),
         (18, 32, 72, 8, "nobias", (True, True, False, True, True)),
         (18, 32, 72, 8, "blas", ALL),     # base products above the threshold
         (18, 32, 72, 8, "no_gx", (False, False, False, True, True))]


@pytest.mark.parametrize("M,K,N,r,variant,req", CASES)
def test_lora_vs_float64(M, K, N, r, variant, req, monkeypatch):
    M = M or _two_slab_m(K, N)
    *ts, g = _inputs(M, K, N, r)
    if variant == "nobias":
        ts[2] = None
    if variant == "blas":
        monkeypatch.setattr(_hf(), "_LIB_LIN_THRESH", 0.0)
    out = _check(variant, ts, g, req)
    assert out.grad_fn.name() == "LoraLinearFnBackward"


def _keep_at(x, counter):
    hf = _hf()
    return hf.native().dropout_fwd_dev(torch.ones_like(x), P,
                                       hf._DROPOUT_STATE["seed"], counter)[1]


@pytest.mark.parametrize("M,K,N,r", [(18, 32, 72, 8), (33, 768, 64, 8)])
def test_lora_dropout(M, K, N, r):
    """dropout()'s keep mask at the same seed and counter is the mask of the
    forward, the row backward and the weight-gradient kernel"""
    hf = _hf()
    *ts, g = _inputs(M, K, N, r, seed=3)
    counter = hf._counter_for(torch.device("cuda", torch.cuda.current_device()))
    counter.add_(1)
    keep = _keep_at(ts[0].cuda(), counter).cpu()
    assert 0.8 < keep.float().mean().item() < 0.97
    counter.sub_(1)     # the call below draws at the same counter value
    out = _check("dropout", ts, g, keep=keep)
    dev = [t.cuda() for t in ts]
    again = hf.lora_linear(*dev, S, P, True)
    assert not torch.equal(out, again), "dropout counter did not advance"
    assert torch.equal(hf.lora_linear(*dev, S, P, False),
                       hf.lora_linear(*dev, S, 0.0, True))


@pytest.mark.parametrize("route", ["fused", "chain", "r17"])
def test_lora_module_route(route, monkeypatch):
    from split_learning_amd.models import lora
    from split_learning_amd.ops.modules import HipLinear
    r = 17 if route == "r17" else 8
    torch.manual_seed(0)
    mod = lora.LoRALinear(HipLinear(32, 72), r, 16, 0.0).cuda()
    with torch.no_grad():
        mod.lora_B.normal_()
    if route == "chain":
        monkeypatch.setattr(lora, "_LORA_CHAIN", True)
    merged = mod.merged_weight().clone()
    x = torch.randn(2, 9, 32).cuda().requires_grad_(True)
    out = mod(x)
    assert (out.grad_fn.name() == "LoraLinearFnBackward") == (route == "fused")
    ts = [t.detach().cpu() for t in (x, mod.base.weight, mod.base.bias,
                                     mod.lora_A * (mod.scaling / S), mod.lora_B)]
    ref = _formula(*(t.double() for t in ts))
    cmp("lora", f"module {route} out", out, _formula(*(t.cuda() for t in ts)), ref)
    assert torch.equal(mod.merged_weight(), merged)


def test_lora_graph_replay():
    """forward + backward captured as one chain: replays draw new masks, and
    each replay's gA belongs to the mask at the offset its forward saved"""
    hf = _hf()
    x, W, b, A, B, g = (t.cuda() for t in _inputs(18, 32, 72, 8, seed=5))
    A.requires_grad_(True)

    def step():
        out = hf.lora_linear(x, W, b, A, B, S, P, True)
        used = out.grad_fn.saved_tensors[5]
        return out, used, torch.autograd.grad(out, A, g)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in static])
    assert not torch.equal(replays[0][0], replays[1][0])
    assert replays[0][1].item() + 1 == replays[1][1].item()

    def g_a(x, g, B, keep):
        return S * (g @ B).t() @ (x * keep.to(x) / (1 - P))

    for i, (out, used, gA) in enumerate(replays):
        keep = _keep_at(x, used)
        cmp("lora", f"replay {i} gA", gA, g_a(x, g, B, keep),
            g_a(cpu64(x), cpu64(g), cpu64(B), keep.cpu()))


def test_lora_checks():
    hf = _hf()
    x, W, _, A, B, _ = (t.cuda() for t in _inputs(5, 8, 4, 2))
    y = torch.zeros(5, 4).cuda()
    bad = {"r=0": (x, W, A[:0], B[:, :0]),
           "K%4": (x[:, :6].contiguous(), W[:, :6].contiguous(),
                   A[:, :6].contiguous(), B),
           "dtype": (x.double(), W, A, B)}
    assert hf.lora_ok(x, W, A, B)
    hf.native().lora_fwd(y, x, A, B, S)
    for what, (xb, Wb, Ab, Bb) in bad.items():
        assert not hf.lora_ok(xb, Wb, Ab, Bb), what
        with pytest.raises(RuntimeError):
            hf.native().lora_fwd(y, xb, Ab, Bb, S)
