"""Tiled MFMA attention (attention_tiled.hip) against a plain float64 CPU
reference: forward and gradients, -10000 and -inf key masks, dropout with the
one-launch kernel's keep mask, routing and saved state, hipGraph replay.

B = 2, H = 3, per-sample valid lengths [S, S//2 + 1] as in
test_attn_mask_gpu.py.  Tensors compare by f64_compare.cmp with torch's fp32
chain (matmul, softmax, matmul and its autograd) on the GPU as the yardstick.
"""

import math

import pytest
import torch

from f64_compare import cmp, cpu64

pytestmark = pytest.mark.gpu

B, H = 2, 3


def _hf():
    from split_learning_amd.ops import functional as hf
    return hf


def _inputs(S, hd, seed=0):
    g = torch.Generator().manual_seed(seed + S)
    q, k, v, go = (torch.randn(B * H, S, hd, generator=g) for _ in range(4))
    scale = float(torch.tensor(1.0 / math.sqrt(hd), dtype=torch.float32))
    return q, k, v, go, scale


def _bias(S, neg, valid1=None):
    """[B, S]: sample 0 sees every key, sample 1 keys valid1 (default the
    first S//2 + 1)"""
    bias = torch.zeros(B, S)
    lo, hi = valid1 or (0, S // 2 + 1)
    bias[1, :lo] = neg
    bias[1, hi:] = neg
    return bias


def _attn(q, k, v, scale, bias, keep=None, p=0.0):
    """matmul, softmax, matmul in the dtype and on the device of q"""
    BH, S, _ = q.shape
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if bias is not None:
        s = (s.view(B, H, S, S) + bias.to(s)[:, None, None, :]).view(BH, S, S)
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep.to(pr) / (1 - p)
    return torch.matmul(pr, v)


def _fwd_bwd(fn, q, k, v, go):
    """[out, gq, gk, gv] of fn on fresh leaves"""
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    out = fn(*leaves)
    out.backward(go.to(out))
    return out, [out.detach()] + [t.grad for t in leaves]


def _tiled(scale, bias, p=0.0):
    from split_learning_amd.ops import modules
    return lambda a, b, c: modules.attention_core(
        a, b, c, dropout_p=p, training=True, scale=scale,
        key_bias=None if bias is None else bias.cuda(), heads=H)


def _is_tiled(out):
    return out.grad_fn is not None and out.grad_fn.name() == "AttnTiledFnBackward"


def _check(what, S, hd, bias, monkeypatch, keep=None, p=0.0, seed=0):
    """the tiled route's out, gq, gk, gv against float64, cmp's rule"""
    from split_learning_amd.ops import modules
    # S >= _TILED_MIN_S goes over the default route, the switch untouched
    monkeypatch.setattr(modules, "_FATTN_TILED", S < modules._TILED_MIN_S)
    q, k, v, go, scale = _inputs(S, hd, seed)
    dev = [t.cuda() for t in (q, k, v, go)]
    out, ours = _fwd_bwd(_tiled(scale, bias, p), *dev)
    assert _is_tiled(out)
    ref = _fwd_bwd(lambda a, b, c: _attn(a, b, c, scale, bias, keep, p),
                   *(t.double() for t in (q, k, v, go)))[1]
    kd = None if keep is None else keep.cuda()
    bd = None if bias is None else bias.cuda()
    yard = _fwd_bwd(lambda a, b, c: _attn(a, b, c, scale, bd, kd, p), *dev)[1]
    for name, o, y, r in zip(("out", "gq", "gk", "gv"), ours, yard, ref):
        cmp("attn_tiled", f"{what} S={S} hd={hd} {name}", o, y, r)
    return out


SHAPES = [(7, 32), (65, 32), (128, 64), (130, 64)]


@pytest.mark.parametrize("S,hd", SHAPES)
@pytest.mark.parametrize("neg", [None, -10000.0])
def test_attn_tiled_vs_float64(S, hd, neg, monkeypatch):
    _check(f"bias={neg}", S, hd, None if neg is None else _bias(S, neg),
           monkeypatch)


def test_attn_tiled_inf_mask(monkeypatch):
    """sample 1 sees keys 70..74 only: its first key tile is all -inf and must
    not poison the running max; no NaN anywhere (cmp checks placement)"""
    _check("-inf", 130, 64, _bias(130, float("-inf"), (70, 75)), monkeypatch)


def test_attn_tiled_no_valid_key_is_nan():
    hf = _hf()
    q, k, v, _, scale = _inputs(130, 64)
    bias = _bias(130, float("-inf"), (0, 0))
    out = hf.attention_tiled(q.cuda(), k.cuda(), v.cuda(), scale,
                             key_bias=bias.cuda(), heads=H).view(B, H, 130, 64)
    assert out[1].isnan().all() and out[0].isfinite().all()


@pytest.mark.parametrize("S,hd", [(65, 32), (128, 64)])
def test_attn_tiled_dropout(S, hd, monkeypatch):
    """the keep mask of the one-launch kernel at the same seed and counter is
    the tiled kernels' mask, forward and both backward kernels"""
    hf = _hf()
    p = 0.1
    q, k, v, _, scale = _inputs(S, hd, seed=3)
    bias = _bias(S, -10000.0)
    counter = hf._counter_for(torch.device("cuda", torch.cuda.current_device()))
    counter.add_(1)
    keep = hf.native().attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale, p,
                                hf._DROPOUT_STATE["seed"], counter,
                                bias.cuda(), H)[2].cpu()
    assert 0.8 < keep.float().mean().item() < 0.97
    counter.sub_(1)     # the call below draws at the same counter value
    out = _check("dropout", S, hd, bias, monkeypatch, keep=keep, p=p, seed=3)
    again = _tiled(scale, bias, p)(q.cuda(), k.cuda(), v.cuda())
    assert not torch.equal(out, again), "dropout counter did not advance"


def test_attn_tiled_route_and_state():
    from split_learning_amd.ops import modules

    def core(S, hd):
        q, k, v, _, _ = _inputs(S, hd)
        return modules.attention_core(q.cuda().requires_grad_(True), k.cuda(),
                                      v.cuda(), key_bias=_bias(S, -10000.0).cuda(),
                                      heads=H)

    S = modules._TILED_MIN_S
    out = core(S, 64)
    assert _is_tiled(out)
    for t in out.grad_fn.saved_tensors:
        assert t is None or t.numel() < B * H * S * S, tuple(t.shape)
    assert not _is_tiled(core(S - 1, 64))
    assert not _is_tiled(core(130, 16))
    q, k, v, _, _ = _inputs(S, 64)
    assert _is_tiled(modules.attention_core(q.cuda().requires_grad_(True),
                                            k.cuda(), v.cuda()))


def test_attn_tiled_checks():
    hf = _hf()
    q = torch.randn(B * H, 7, 32).cuda()
    fwd = hf.native().attn_tiled_fwd
    bad = [(q.double(), q, q, 0.5), (q.cpu(), q, q, 0.5), (q, q[:, :5], q, 0.5),
           (q[:, :, :16], q[:, :, :16], q[:, :, :16], 0.5), (q, q, q, 0.5, 1.0),
           (q, q, q, 0.5, 0.0, 0, None, torch.zeros(B, 6).cuda(), H),
           (q, q, q, 0.5, 0.0, 0, None, torch.zeros(B, 7).cuda(), 4)]
    for args in bad:
        with pytest.raises(RuntimeError):
            fwd(*args)


def test_attn_tiled_graph_replay(monkeypatch):
    """forward + backward captured as one chain: replays draw new masks, and
    each replay's gq is the eager backward at the offset that replay's forward
    saved, run when the live counter has moved on"""
    from split_learning_amd.ops import modules
    hf = _hf()
    monkeypatch.setattr(modules, "_FATTN_TILED", True)
    S, hd, p = 65, 32, 0.1
    q, k, v, go, scale = (t.cuda() if torch.is_tensor(t) else t
                          for t in _inputs(S, hd, seed=5))
    bias = _bias(S, -10000.0).cuda()
    q.requires_grad_(True)

    def step():
        out = modules.attention_core(q, k, v, dropout_p=p, training=True,
                                     scale=scale, key_bias=bias, heads=H)
        lse, used = out.grad_fn.saved_tensors[4:6]
        return out, lse, used, torch.autograd.grad(out, q, go)[0]

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
    assert replays[0][2].item() + 1 == replays[1][2].item()
    for out, lse, used, gq in replays:
        eager = hf.native().attn_tiled_bwd(
            go, q.detach(), k, v, out, lse, scale, p, hf._DROPOUT_STATE["seed"],
            used, bias, H)[0]
        assert torch.equal(eager, gq)
        assert cpu64(gq).abs().max() > 0
