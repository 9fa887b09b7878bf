"""hf.attention_heads (attention_tiled.hip on the projections' [B,S,E] layout)
against plain float64 on the CPU over the permuted heads, against the
contiguous kernels bit for bit, and through the MHA and BERT modules.  B = 2,
H = 3, valid lengths [S, S//2 + 1]; f64_compare.cmp, yardstick: torch fp32."""

import math

import pytest
import torch
import torch.nn as nn

from f64_compare import cmp, exact
from split_learning_amd.models.bert import BertSdpaSelfAttention
from split_learning_amd.ops import functional as hf
from split_learning_amd.ops import modules

pytestmark = pytest.mark.gpu

B, H = 2, 3
NODE = "AttnHeadsFnBackward"


def _valid(S, pad, keep=0.0):
    """[B, S]: sample 0 sees every key, sample 1 the first S//2 + 1"""
    t = torch.full((B, S), keep)
    t[1, S // 2 + 1:] = pad
    return t


def _leaves(layout, raw, E):
    """raw [3, B, S, E+4] -> (leaves, (q, k, v)) in raw's dtype and device"""
    if layout == "packed":
        leaf = torch.cat([r[..., :E] for r in raw], -1).requires_grad_(True)
        return [leaf], leaf.split(E, dim=-1)
    cols = E if layout == "separate" else E + 4
    leaves = [r[..., :cols].clone().requires_grad_(True) for r in raw]
    return leaves, [t[:, :, :E] for t in leaves]


def _attn(q, k, v, scale, bias):
    """matmul, softmax, matmul over the permuted heads, q's dtype and device"""
    _, S, E = q.shape
    q, k, v = (t.reshape(B, S, H, E // H).permute(0, 2, 1, 3) for t in (q, k, v))
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.to(s)[:, None, None, :]
    return torch.matmul(torch.softmax(s, -1), v).permute(0, 2, 1, 3).reshape(B, S, E)


def _run(fn, layout, raw, E, go):
    leaves, qkv = _leaves(layout, raw, E)
    out = fn(*qkv)
    out.backward(go.to(out))
    return out, [out.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("S,hd", [(7, 32), (65, 32), (130, 64)])
@pytest.mark.parametrize("layout", ["packed", "separate", "padded"])
@pytest.mark.parametrize("neg", [None, -10000.0])
def test_attn_heads_vs_float64(S, hd, layout, neg):
    E = H * hd
    g = torch.Generator().manual_seed(S)
    raw = torch.randn(3, B, S, E + 4, generator=g)
    go = torch.randn(B, S, E, generator=g)
    scale = float(torch.tensor(1.0 / math.sqrt(hd), dtype=torch.float32))
    bias = None if neg is None else _valid(S, neg)
    bd = None if neg is None else bias.cuda()
    dev = (layout, raw.cuda(), E, go.cuda())
    out, ours = _run(lambda q, k, v: hf.attention_heads(
        q, k, v, H, scale, key_bias=bd), *dev)
    assert out.grad_fn.name() == NODE and out.is_contiguous()
    yard = _run(lambda q, k, v: _attn(q, k, v, scale, bd), *dev)[1]
    ref = _run(lambda q, k, v: _attn(q, k, v, scale, bias), layout,
               raw.double(), E, go.double())[1]
    for i, (o, y, r) in enumerate(zip(ours, yard, ref)):
        cmp("attn_heads", f"{layout} bias={neg} S={S} hd={hd} [{i}]", o, y, r)


@pytest.mark.parametrize("S,hd", [(65, 32), (128, 64)])
def test_attn_heads_equals_tiled(S, hd):
    """same seed, same counter value: the packed layout's out and gradients
    are the contiguous kernels' on permuted copies, bit for bit"""
    E, p, scale = H * hd, 0.1, 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(3 + S)
    leaf = torch.randn(B, S, 3 * E, generator=g).cuda().requires_grad_(True)
    go = torch.randn(B, S, E, generator=g).cuda()
    bias = _valid(S, -10000.0).cuda()
    def heads_first(t):     # [B,S,E] -> [BH,S,hd]
        return t.reshape(B, S, H, hd).permute(0, 2, 1, 3).reshape(B * H, S, hd)

    counter = hf._counter_for(leaf.device)
    start = counter.item()
    out = hf.attention_heads(*leaf.split(E, dim=-1), H, scale, dropout_p=p,
                             training=True, key_bias=bias)
    out.backward(go)
    assert counter.item() == start + 1
    counter.sub_(1)     # the contiguous call draws at the same counter value
    copies = [heads_first(t).detach().contiguous().requires_grad_(True)
              for t in leaf.split(E, dim=-1)]
    ref = hf.attention_tiled(*copies, scale, dropout_p=p, training=True,
                             key_bias=bias, heads=H)
    ref.backward(heads_first(go))
    assert counter.item() == start + 1
    exact(heads_first(out), ref, f"out S={S}")
    for name, ours, c in zip("qkv", leaf.grad.split(E, dim=-1), copies):
        exact(heads_first(ours), c.grad, f"g{name} S={S}")


def _module_grads(mod, call, x, go, params):
    x = x.detach().clone().requires_grad_(True)
    mod.zero_grad()
    out = call(mod, x)
    out.backward(go.to(out))
    return out, [out.detach(), x.grad] + [mod.get_parameter(n).grad.clone()
                                          for n in params]


@pytest.mark.parametrize("kind,S,switch", [    # S = 130: the default route
    ("mha", 65, True), ("mha_masked", 65, True), ("bert", 130, False),
    ("bert", 65, True)])
def test_attn_heads_modules(kind, S, switch, monkeypatch):
    """the module on the new route (the node that ran is AttnHeadsFn's)
    against a float64 CPU module; yardstick: itself with the route off"""
    torch.manual_seed(11)
    if kind == "bert":
        E, params = 128, ["query.weight", "key.weight", "value.weight"]
        mod = BertSdpaSelfAttention(E, 2, 0.0).cuda()
        ref = BertSdpaSelfAttention(E, 2, 0.0).double()
        mask = _valid(S, 0.0, keep=1.0)
        def call(m, t):
            return m(t, mask.to(t.device))
        node = lambda out: out.grad_fn.name()
    else:
        E, params = 64, ["in_proj_weight", "out_proj.weight"]
        mod = modules.HipMultiheadAttention(E, 2, batch_first=True).cuda()
        ref = nn.MultiheadAttention(E, 2, batch_first=True).double()
        kpm = _valid(S, 1.0).bool() if kind == "mha_masked" else None
        def call(m, t):
            return m(t, t, t, need_weights=False, key_padding_mask=None
                     if kpm is None else kpm.to(t.device))[0]
        node = lambda out: out.grad_fn.next_functions[0][0].name()  # -> out_proj
    ref.load_state_dict(mod.state_dict())
    x, go = torch.randn(B, S, E), torch.randn(B, S, E)
    monkeypatch.setattr(modules, "_FATTN_TILED", switch)
    out, ours = _module_grads(mod, call, x.cuda(), go.cuda(), params)
    assert node(out) == NODE
    monkeypatch.setattr(modules, "_FATTN_TILED", False)
    if switch:      # S = 65 with the switch off: today's route
        assert node(call(mod, x.cuda())) != NODE
    monkeypatch.setattr(modules, "_TILED_MIN_S", 1 << 30)   # off at every S
    out, yard = _module_grads(mod, call, x.cuda(), go.cuda(), params)
    assert node(out) != NODE
    want = _module_grads(ref, call, x.double(), go.double(), params)[1]
    for name, o, y, r in zip(["out", "gx"] + params, ours, yard, want):
        cmp("attn_heads", f"{kind} S={S} {name}", o, y, r)


def test_attn_heads_checks():
    S, E, fwd = 7, H * 32, hf.native().attn_heads_fwd
    q = torch.randn(B, S, E).cuda()
    every_other = torch.randn(B, S, 2 * E).cuda()[:, :, ::2]
    odd_rows = torch.randn(B, S, E + 1).cuda()[:, :, :E]
    q16 = q[:, :, :H * 16]
    bad = [(every_other, q, q, H, 0.5), (q, odd_rows, q, H, 0.5),
           (q16, q16, q16, H, 0.5), (q, q, q, 5, 0.5), (q, q[:, :5], q, H, 0.5),
           (q, q, q, H, 0.5, 0.0, 0, None, torch.zeros(B, S - 1).cuda())]
    for args in bad:
        with pytest.raises(RuntimeError):
            fwd(*args)
    for args in bad[:-1]:       # the bias is not the operands' precondition
        assert not hf.attn_heads_ok(*args[:4])
    assert hf.attn_heads_ok(q, q, q, H) and len(fwd(q, q, q, H, 0.5)) == 3
