"""Causal mode of the tiled attention kernels against plain float64 on the
CPU (matmul, +triu(-inf), softmax, matmul); helpers, B = 2, H = 3 and the
fp32 yardstick of test_attn_tiled_gpu.py; the walk bounds by exact equality."""
import math

import pytest
import torch

from f64_compare import cmp, exact
from split_learning_amd.ops import functional as hf
from split_learning_amd.ops import modules
from test_attn_tiled_gpu import B, H, _bias, _fwd_bwd, _inputs, _is_tiled

pytestmark = pytest.mark.gpu


def _attn(q, k, v, scale, bias, keep, p):
    BH, S, _ = q.shape
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if bias is not None:
        s = (s.view(B, H, S, S) + bias.to(s)[:, None, None, :]).view(BH, S, S)
    pr = torch.softmax(s + torch.full((S, S), -math.inf).triu(1).to(s), dim=-1)
    return torch.matmul(pr if keep is None else pr * keep.to(pr) / (1 - p), v)


def _core(scale, bias=None, p=0.0):
    return lambda a, b, c: modules.attention_core(
        a, b, c, dropout_p=p, training=True, scale=scale, heads=H,
        key_bias=None if bias is None else bias.cuda(), is_causal=True)


@pytest.mark.parametrize("S,hd,neg,p", [
    (S, hd, neg, 0.0) for S, hd in [(7, 32), (65, 32), (128, 64), (130, 64)]
    for neg in (None, -10000.0)] + [(65, 32, -10000.0, 0.1), (128, 64, -10000.0, 0.1)])
def test_attn_causal_vs_float64(S, hd, neg, p, monkeypatch):
    monkeypatch.setattr(modules, "_FATTN_TILED", False)   # causal needs no switch
    q, k, v, go, scale = _inputs(S, hd, seed=3)
    dev = [t.cuda() for t in (q, k, v, go)]
    bias, keep = None if neg is None else _bias(S, neg), None
    if p > 0.0:     # the one-launch kernel's keep mask at this seed and counter
        counter = hf._counter_for(dev[0].device)
        counter.add_(1)
        keep = hf.native().attn_fwd(*dev[:3], scale, p, hf._DROPOUT_STATE["seed"],
                                    counter, bias.cuda(), H)[2].cpu()
        counter.sub_(1)     # the call below draws at the same counter value
    out, ours = _fwd_bwd(_core(scale, bias, p), *dev)
    assert _is_tiled(out)
    ref = lambda a, b, c: _attn(a, b, c, scale, bias, keep, p)
    want = _fwd_bwd(ref, *(t.double() for t in (q, k, v, go)))[1]
    for name, o, y, r in zip("oqkv", ours, _fwd_bwd(ref, *dev)[1], want):
        cmp("attn_causal", f"bias={neg} p={p} S={S} hd={hd} {name}", o, y, r)


@pytest.mark.parametrize("j", [64, 70])
def test_attn_causal_nothing_from_the_future(j):
    q, k, v, go = (t.cuda() for t in _inputs(130, 64)[:4])
    go[:, j:], scale = 0, 0.125
    k2, v2 = k.clone(), v.clone()
    k2[:, j:], v2[:, j:] = 40.0 * k[:, j:] + 3.0, -70.0 * v[:, j:]
    ours = _fwd_bwd(_core(scale), q, k, v, go)[1]
    exact(_fwd_bwd(_core(scale), q, k2, v2, go)[1][0][:, :j], ours[0][:, :j], "out")
    for name, g in zip(("gk", "gv"), ours[2:]):
        exact(g[:, j:], torch.zeros_like(g[:, j:]), name)


@pytest.mark.parametrize("heads,hd,p", [(2, 64, 0.0), (4, 32, 0.1)])
def test_attn_causal_heads_equals_tiled(heads, hd, p):
    S, E, scale = 130, heads * hd, 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(heads)
    leaf = torch.randn(B, S, 3 * E, generator=g).cuda().requires_grad_(True)
    go = torch.randn(B, S, E, generator=g).cuda()
    def heads_first(t):     # [B,S,E] -> [BH,S,hd]
        return t.reshape(B, S, heads, hd).permute(0, 2, 1, 3).reshape(-1, S, hd)
    out = hf.attention_heads(*leaf.split(E, dim=-1), heads, scale, dropout_p=p,
                             training=True, is_causal=True)
    out.backward(go)
    hf._counter_for(leaf.device).sub_(int(p > 0.0))     # same counter value below
    copies = [heads_first(t).detach().contiguous().requires_grad_(True)
              for t in leaf.split(E, dim=-1)]
    ref = hf.attention_tiled(*copies, scale, dropout_p=p, training=True,
                             heads=heads, is_causal=True)
    ref.backward(heads_first(go))
    exact(heads_first(out), ref, "out")
    for name, ours, c in zip("qkv", leaf.grad.split(E, dim=-1), copies):
        exact(heads_first(ours), c.grad, f"g{name}")


def _mha(mod, x, kpm, stock):
    fwd = torch.nn.MultiheadAttention.forward if stock else type(mod).forward
    mask = torch.ones(x.shape[1], x.shape[1], dtype=torch.bool, device=x.device)
    return fwd(mod, x, x, x, key_padding_mask=kpm.to(x.device), is_causal=True,
               attn_mask=mask.triu(1), need_weights=False)[0]


def test_attn_causal_module():
    """reference: the stock forward of a float64 copy; yardstick: in fp32"""
    torch.manual_seed(11)
    S, E = 20, 64
    mod = modules.HipMultiheadAttention(E, 2, batch_first=True).cuda()
    ref = torch.nn.MultiheadAttention(E, 2, batch_first=True).double()
    ref.load_state_dict(mod.state_dict())
    x, go = torch.randn(3, S, E), torch.randn(3, S, E)
    kpm = torch.arange(S)[None, :] >= torch.tensor([S, 15, 11])[:, None]
    res = []
    for m, xx, stock in (mod, x.cuda(), 0), (mod, x.cuda(), 1), (ref, x.double(), 1):
        m.zero_grad()
        out = _mha(m, xx, kpm, stock)
        out.backward(go.to(out))
        res.append([out, m.in_proj_weight.grad.clone()])
    assert res[0][0].grad_fn.next_functions[0][0].name() == "AttnHeadsFnBackward"
    for name, o, y, r in zip(("out", "in_proj_weight"), *res):
        cmp("attn_causal", f"mha S={S} {name}", o, y, r)
    kpm[1, 0] = True    # sample 1's query row 0 sees no key; out_proj is row-wise
    out = _mha(mod, x.cuda(), kpm, False).detach().cpu()
    assert out[1, 0].isnan().all() and int((~out.isfinite()).sum()) == E
