"""bf16-operand tiled attention (attention_tiled_bf16.hip) against a plain
float64 CPU reference.

B = 2, H = 3, per-sample valid lengths [S, S//2 + 1] as in
test_attn_tiled_gpu.py.  The reference is the float64 chain matmul, + bias
(, triu -inf), softmax, o keep / (1 - p), matmul and its autograd on the
bf16-rounded q, k, v and upstream gradient, with no intermediate rounding.

Error units, u = 2^-8 (bf16's half-spacing), from the reference's own P, P_d
(dropped and scaled), dS, and D_i = sum_d |gOb_id| (P_d |vb|)_id: one operand
rounding of relative size u where the kernels round,
  out: u P_d |vb|                     (the P operand)
  gv:  u P_d^T |gOb|                  (the P_d operand)
  gq:  u scale (|dS| |kb| + D o (P |kb|))      (the dS operand; the forward's
  gk:  u scale (|dS|^T |qb| + (P o D)^T |qb|)   output error entering delta)
Everything fp32 in the kernels is estimated under 3 % of a unit here, so the
assertion is |kernel - ref| <= (1 + 1/16) unit element by element; the fp32
kernels on unrounded operands miss this reference by a unit or more, so it
also shows the bf16 route ran.  Where a unit is 0 (masked keys' gk and gv)
the kernel must be exactly 0.
"""

import math

import pytest
import torch

from f64_compare import _draw, _gen, cpu64, exact

pytestmark = pytest.mark.gpu

B, H = 2, 3
U = 2.0 ** -8
NAMES = ("out", "gq", "gk", "gv")


def _hf():
    from split_learning_amd.ops import functional as hf
    return hf


def _inputs(S, hd, seed=0):
    g = _gen(seed + S)
    q, k, v, go = (_draw("randn", (B * H, S, hd), g) for _ in range(4))
    return q, k, v, go, float(torch.tensor(1.0 / math.sqrt(hd)))


def _bias(S, neg, valid1=None):
    """[B, S]: sample 0 sees every key, sample 1 keys valid1 (default the
    first S//2 + 1)"""
    bias = torch.zeros(B, S)
    lo, hi = valid1 or (0, S // 2 + 1)
    bias[1, :lo] = neg
    bias[1, hi:] = neg
    return bias


def _ref(q, k, v, go, scale, bias=None, causal=False, keep=None, p=0.0):
    """float64 [out, gq, gk, gv] on the rounded operands, and their units"""
    qb, kb, vb, gb = (t.bfloat16().double() for t in (q, k, v, go))
    leaves = [t.requires_grad_(True) for t in (qb, kb, vb)]
    BH, S, _ = q.shape
    s = qb @ kb.transpose(-1, -2) * scale
    if bias is not None:
        s = (s.view(B, H, S, S) + bias.double()[:, None, None, :]).view(BH, S, S)
    if causal:
        s = s + torch.full((S, S), float("-inf"), dtype=s.dtype).triu(1)
    P = torch.softmax(s, dim=-1)
    drop = 1.0 if keep is None else keep.double() / (1 - p)
    Pd = P * drop
    out = Pd @ vb
    out.backward(gb)
    with torch.no_grad():
        dS = P * ((gb @ vb.transpose(-1, -2)) * drop
                  - (gb * out).sum(-1, keepdim=True))
        D = (gb.abs() * (Pd @ vb.abs())).sum(-1, keepdim=True)
        aq, ak = qb.abs(), kb.abs()
        units = [U * (Pd @ vb.abs()),
                 U * scale * (dS.abs() @ ak + D * (P @ ak)),
                 U * scale * (dS.abs().transpose(-1, -2) @ aq
                              + (P * D).transpose(-1, -2) @ aq),
                 U * (Pd.transpose(-1, -2) @ gb.abs())]
    return [out.detach(), qb.grad, kb.grad, vb.grad], units


def _heads(t):      # [BH,S,hd] -> [B,S,E]
    return t.view(B, H, *t.shape[1:]).permute(0, 2, 1, 3).reshape(B, t.shape[1], -1)


def _unheads(t, hd):    # [B,S,E] -> [BH,S,hd]
    return t.view(B, -1, H, hd).permute(0, 2, 1, 3).reshape(B * H, -1, hd)


def _run(layout, q, k, v, go, scale, bias=None, causal=False, p=0.0):
    """the bf16 route's output tensor and its [out, gq, gk, gv] as [BH,S,hd]"""
    from split_learning_amd.ops import modules
    bd = None if bias is None else bias.cuda()
    if layout == "contiguous":
        leaves = [t.cuda().requires_grad_(True) for t in (q, k, v)]
        out = modules.attention_core(*leaves, dropout_p=p, training=True,
                                     scale=scale, key_bias=bd, heads=H,
                                     is_causal=causal, compute="bf16")
        assert out.grad_fn.name() == "AttnTiledBf16FnBackward"
        out.backward(go.cuda())
        return out, [out.detach()] + [t.grad for t in leaves]
    hd = q.shape[-1]
    x = torch.cat([_heads(t) for t in (q, k, v)], -1).cuda().requires_grad_(True)
    out = _hf().attention_heads(*x.split(H * hd, -1), H, scale, dropout_p=p,
                                training=True, key_bias=bd, packed=x,
                                is_causal=causal, compute="bf16")
    assert out.grad_fn.name() == "AttnHeadsBf16FnBackward"
    out.backward(_heads(go).cuda())
    assert x.grad.shape == x.shape      # the one packed gradient
    return out, [_unheads(t, hd) for t in
                 (out.detach(), *x.grad.split(H * hd, -1))]


def _within(what, ours, refs, units):
    for name, o, r, unit in zip(NAMES, ours, refs, units):
        o = cpu64(o)
        assert torch.equal(torch.isnan(o), torch.isnan(r)), f"{what} {name}: NaN"
        err = (o - r).abs()
        pos = unit > 0
        worst = float((err[pos] / unit[pos]).max()) if bool(pos.any()) else 0.0
        print(f"attn_bf16 {what} {name}: worst {worst:.3f} units")
        bad = err > (1 + 1 / 16) * unit     # unit 0: the kernel must be exact
        assert not bool(bad.any()), \
            f"{what} {name}: {int(bad.sum())} over the cap, worst {worst:.3f}"


def _check(what, layout, S, hd, bias=None, causal=False, keep=None, p=0.0,
           seed=0):
    q, k, v, go, scale = _inputs(S, hd, seed)
    out, ours = _run(layout, q, k, v, go, scale, bias, causal, p)
    refs, units = _ref(q, k, v, go, scale, bias, causal, keep, p)
    _within(f"{what} {layout} S={S} hd={hd}", ours, refs, units)
    return out


@pytest.mark.parametrize("S,hd", [(1, 32), (7, 32), (65, 32), (128, 64), (130, 64)])
@pytest.mark.parametrize("layout", ["contiguous", "packed"])
@pytest.mark.parametrize("neg", [None, -10000.0])
def test_attn_bf16_vs_float64(S, hd, layout, neg):
    _check(f"bias={neg}", layout, S, hd, None if neg is None else _bias(S, neg))


@pytest.mark.parametrize("hd", [32, 64])
def test_attn_bf16_one_key_is_exact(hd):
    """S = 1: P = 1 and lse = s, so out is vb and gv is gOb, bit for bit"""
    q, k, v, go, scale = _inputs(1, hd)
    _, ours = _run("contiguous", q, k, v, go, scale)
    exact(ours[0], v.bfloat16().float(), "out")
    exact(ours[3], go.bfloat16().float(), "gv")


def test_attn_bf16_inf_mask():
    """sample 1 sees keys 70..74 only: its first key tile is all -inf; no NaN"""
    _check("-inf", "contiguous", 130, 64, _bias(130, float("-inf"), (70, 75)))


def test_attn_bf16_no_valid_key_is_nan():
    q, k, v, _, scale = _inputs(130, 64)
    bias = _bias(130, float("-inf"), (0, 0))
    out = _hf().attention_tiled(q.cuda(), k.cuda(), v.cuda(), scale,
                                key_bias=bias.cuda(), heads=H,
                                compute="bf16").view(B, H, 130, 64)
    assert out[1].isnan().all() and out[0].isfinite().all()


@pytest.mark.parametrize("S,hd", [(65, 32), (130, 64)])
@pytest.mark.parametrize("neg", [None, -10000.0])
def test_attn_bf16_causal(S, hd, neg):
    for layout in ("contiguous", "packed"):
        _check(f"causal bias={neg}", layout, S, hd,
               None if neg is None else _bias(S, neg), causal=True)


@pytest.mark.parametrize("S,hd", [(65, 32), (128, 64)])
def test_attn_bf16_dropout(S, hd):
    """the keep mask of the one-launch kernel at the same seed and counter is
    these kernels' mask, forward and both backward kernels"""
    hf = _hf()
    p = 0.1
    q, k, v, go, scale = _inputs(S, hd, seed=3)
    bias = _bias(S, -10000.0)
    counter = hf._counter_for(torch.device("cuda", torch.cuda.current_device()))
    counter.add_(1)
    keep = hf.native().attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale, p,
                                hf._DROPOUT_STATE["seed"], counter,
                                bias.cuda(), H)[2].cpu()
    assert 0.8 < keep.float().mean().item() < 0.97
    counter.sub_(1)     # the call below draws at the same counter value
    out = _check("dropout", "contiguous", S, hd, bias, keep=keep, p=p, seed=3)
    again, _ = _run("contiguous", q, k, v, go, scale, bias, p=p)
    assert not torch.equal(out, again), "dropout counter did not advance"


def test_attn_bf16_routing_and_state():
    hf = _hf()
    q, k, v, _, scale = (t.cuda() if torch.is_tensor(t) else t
                         for t in _inputs(130, 64))
    for bad in (q[..., :16], q.cpu(), q.double()):
        with pytest.raises(ValueError):
            hf.attention_tiled(bad, bad, bad, scale, compute="bf16")
        with pytest.raises(ValueError):
            hf.attention_heads(_heads(bad), _heads(bad), _heads(bad), H, scale,
                               compute="bf16")
    today = hf.attention_tiled(q, k, v, scale)
    for compute in (None, "fp32"):
        assert torch.equal(hf.attention_tiled(q, k, v, scale, compute=compute),
                           today)
    assert not torch.equal(hf.attention_tiled(q, k, v, scale, compute="bf16"),
                           today)
    out = hf.attention_tiled(q.requires_grad_(True), k, v, scale, compute="bf16")
    assert all(t is None or t.numel() < B * H * 130 * 130
               for t in out.grad_fn.saved_tensors)


def test_attn_bf16_multihead_attention():
    """HipMultiheadAttention.compute = "bf16" at S = 65 (below the tiled
    route's threshold) with a boolean key_padding_mask: the final output
    against float64 attention on the module's own in-projection, pushed
    through the float64 out-projection; unit = out unit . |W_out|^T"""
    from split_learning_amd.ops import modules
    S, E = 65, 96
    torch.manual_seed(0)
    mha = modules.HipMultiheadAttention(E, H, batch_first=True).cuda().eval()
    mha.compute = "bf16"
    x = _draw("randn", (B, S, E), _gen(5)).cuda()
    pad = torch.zeros(B, S, dtype=torch.bool)
    pad[1, S // 2 + 1:] = True
    out, _ = mha(x, x, x, key_padding_mask=pad.cuda())
    seen, todo = set(), [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is not None and fn not in seen:
            seen.add(fn)
            todo += [f for f, _ in fn.next_functions]
    assert "AttnHeadsBf16FnBackward" in {f.name() for f in seen}
    qkv = _hf().linear(x, mha.in_proj_weight, mha.in_proj_bias).detach().cpu()
    q, k, v = (_unheads(t, E // H) for t in qkv.split(E, -1))
    refs, units = _ref(q, k, v, torch.zeros_like(q), 1.0 / math.sqrt(E // H),
                       _bias(S, float("-inf")))
    W, b = cpu64(mha.out_proj.weight), cpu64(mha.out_proj.bias)
    ref = _heads(refs[0]) @ W.t() + b
    unit = _heads(units[0]) @ W.abs().t()
    _within("mha S=65", [out], [ref], [unit])
