"""QKV-grouped LoRA adapter (lora.hip lora_qkv_*, hf.lora_qkv) against the
formula in float64 on the CPU, for j = q, k, v:

    out[:, jN:(j+1)N] = x W_j^T + b_j + s * (dropout_j(x) A_j^T) B_j^T

forward and the gradients autograd takes through LoraQkvFn, by f64_compare.cmp
with the same formula in fp32 torch on the GPU as yardstick.  The three
adapters get different random values (lora_B too), so a swapped third fails.
"""

import copy

import pytest
import torch

from f64_compare import cmp, cpu64

pytestmark = pytest.mark.gpu

S = 2.0     # alpha / r of the BERT adapters
P = 0.1
# leaves: x, W q k v, b q k v, A q k v, B q k v
NAMES = ["gx"] + [f"g{n}_{j}" for n in "WbAB" for j in "qkv"]
ADAPTERS = [False] * 7 + [True] * 6
DEFAULT = [True] + ADAPTERS[1:]


def _hf():
    from split_learning_amd.ops import functional as hf
    return hf


def _inputs(M, K, N, r, seed=0):
    """the 13 leaves and g [M,3N]"""
    g = torch.Generator().manual_seed(seed + M + K)
    shapes = [(M, K)] + [(N, K)] * 3 + [(N,)] * 3 + [(r, K)] * 3 + [(N, r)] * 3
    return [torch.randn(s, generator=g) for s in shapes + [(M, 3 * N)]]


def _formula(x, *ts, keeps=None):
    outs = []
    for j in range(3):
        W, b, A, B = ts[j], ts[3 + j], ts[6 + j], ts[9 + j]
        xd = x if keeps is None else x * keeps[j].to(x) / (1 - P)
        y = x @ W.t() if b is None else x @ W.t() + b
        outs.append(y + S * ((xd @ A.t()) @ B.t()))
    return torch.cat(outs, -1)


def _qkv(x, *ts, p=0.0, training=True):
    return _hf().lora_qkv(x, ts[0:3], ts[3:6], ts[6:9], ts[9:12], S, p, training)


def _fwd_bwd(fn, ts, g, req):
    """[out, grads of the leaves that ask] of fn on fresh leaves"""
    leaves = [None if t is None else t.detach().clone().requires_grad_(rq)
              for t, rq in zip(ts, req)]
    out = fn(*leaves)
    out.backward(g.to(out))
    return out, [out.detach()] + [l.grad for l, rq in zip(leaves, req) if rq]


def _check(what, ts, g, req=DEFAULT, keeps=None):
    """the grouped route's out and gradients against float64, cmp's rule"""
    dev = [None if t is None else t.cuda() for t in ts]
    out, ours = _fwd_bwd(lambda *a: _qkv(*a, p=0.0 if keeps is None else P),
                         dev, g.cuda(), req)
    ref = _fwd_bwd(lambda *a: _formula(*a, keeps=keeps),
                   [None if t is None else t.double() for t in ts], g.double(),
                   req)[1]
    kd = None if keeps is None else [k.cuda() for k in keeps]
    yard = _fwd_bwd(lambda *a: _formula(*a, keeps=kd), dev, g.cuda(), req)[1]
    names = ["out"] + [n for n, rq in zip(NAMES, req) if rq]
    for name, o, y, r in zip(names, ours, yard, ref, strict=True):
        assert cpu64(r).abs().max() > 0
        cmp("lora_qkv", f"{what} {tuple(ts[0].shape)} r={ts[7].shape[0]} {name}",
            o, y, r)
    return out


def _two_slab_m(K, N):
    """smallest M whose weight-gradient grid has two slabs, plus 3: the last
    slab is ragged"""
    slabs = _hf().native().lora_qkv_wgrad_slabs
    return next(m for m in range(1, 4096) if slabs(m, K, N) >= 2) + 3


CASES = [(5, 4, 4, 1, "plain", DEFAULT), (18, 32, 72, 8, "plain", DEFAULT),
         (33, 768, 64, 8, "plain", DEFAULT), (None, 72, 32, 16, "plain", DEFAULT),
         (18, 32, 72, 8, "nobias", DEFAULT),
         (18, 32, 72, 8, "blas", [True] * 13),   # base products above the threshold
         (18, 32, 72, 8, "no_gx", ADAPTERS)]


@pytest.mark.parametrize("M,K,N,r,variant,req", CASES)
def test_lora_qkv_vs_float64(M, K, N, r, variant, req, monkeypatch):
    M = M or _two_slab_m(K, N)
    *ts, g = _inputs(M, K, N, r)
    if variant == "nobias":
        ts[4:7] = [None] * 3
    if variant == "blas":
        monkeypatch.setattr(_hf(), "_LIB_LIN_THRESH", 0.0)
    out = _check(variant, ts, g, req)
    assert out.grad_fn.name() == "LoraQkvFnBackward"


@pytest.mark.parametrize("M,K,N,r", [(18, 32, 72, 8), (33, 768, 64, 8)])
def test_lora_qkv_dropout(M, K, N, r):
    """the bits of three lora_linear calls in q, k, v order, the counter 3
    further, and dropout()'s keep masks at those three counter values in the
    forward, the row backward and the weight-gradient kernel"""
    hf = _hf()
    *ts, g = _inputs(M, K, N, r, seed=3)
    dev = [t.cuda() for t in ts]
    counter = hf._counter_for(dev[0].device)
    start = counter.item()
    singles = torch.cat([hf.lora_linear(dev[0], *dev[1 + j::3], S, P, True)
                         for j in range(3)], -1)
    assert counter.item() == start + 3
    keeps = []
    for j in range(3):
        counter.fill_(start + 1 + j)
        keeps.append(hf.native().dropout_fwd_dev(
            torch.ones_like(dev[0]), P, hf._DROPOUT_STATE["seed"], counter)[1].cpu())
        assert 0.8 < keeps[j].float().mean().item() < 0.97
    assert not torch.equal(keeps[0], keeps[1])
    counter.fill_(start)    # the call below starts where the three singles did
    out = _check("dropout", ts, g, keeps=keeps)
    assert counter.item() == start + 3
    assert torch.equal(out, singles)
    assert not torch.equal(out, _qkv(*dev, p=P)), "dropout counter did not advance"
    assert torch.equal(_qkv(*dev, p=P, training=False), _qkv(*dev))


def _graph_names(fn, seen=None):
    seen = set() if seen is None else seen
    if fn is not None and fn not in seen:
        seen.add(fn)
        for nxt, _ in fn.next_functions:
            _graph_names(nxt, seen)
    return {f.name() for f in seen}


@pytest.mark.parametrize("seq", [130, 20])   # packed tiled attention; the chain
def test_lora_qkv_module_route(seq, monkeypatch):
    from split_learning_amd.models import lora
    from split_learning_amd.models.bert import BertSdpaSelfAttention
    torch.manual_seed(0)
    mod = lora.apply_lora(BertSdpaSelfAttention(64, 2, 0.0), r=8, alpha=16,
                          dropout=0.0).train()
    adapters = [p for n, p in mod.named_parameters() if "lora_" in n]
    assert len(adapters) == 6
    with torch.no_grad():
        for p in adapters:
            p.normal_(std=0.3)
    x, g = torch.randn(2, seq, 64), torch.randn(2, seq, 64)

    def run(m, dtype, device):
        m = copy.deepcopy(m).to(device=device, dtype=dtype)
        out = m(x.to(device=device, dtype=dtype))
        grads = torch.autograd.grad(out, [p for n, p in m.named_parameters()
                                          if "lora_" in n], g.to(out))
        return out, [out.detach(), *grads]

    monkeypatch.setattr(lora, "_LORA_SINGLE", False)
    out, ours = run(mod, torch.float32, "cuda")
    assert "LoraQkvFnBackward" in _graph_names(out.grad_fn)
    ref = run(mod, torch.float64, "cpu")[1]
    yard = run(mod, torch.float32, "cpu")[1]     # plain torch in fp32
    for i, (o, y, r) in enumerate(zip(ours, yard, ref, strict=True)):
        cmp("lora_qkv", f"module S={seq} {'out' if i == 0 else f'grad {i}'}",
            o, y, r)
    monkeypatch.setattr(lora, "_LORA_SINGLE", True)
    single = run(mod, torch.float32, "cuda")[0]
    assert "LoraQkvFnBackward" not in _graph_names(single.grad_fn)
    assert torch.equal(single, out)
