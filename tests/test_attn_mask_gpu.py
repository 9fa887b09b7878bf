"""Attention padding masks on the GPU: the masked-softmax kernels
(attn_softmax_fwd / attn_softmax_bwd), the key bias in the one-launch kernel,
attention_core / HipMultiheadAttention routing, hipGraph replay and BERT.

Shapes are (B, H, S, hd).  Per-sample valid lengths are [S, S//2 + 1], so the
two samples differ and a wrong bh / heads shows; H = 3 keeps the head count off
a power of two.  The bias is -10000 at padded keys unless stated.
"""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NEG = -10000.0

# Max abs error of the softmax_fwd kernel (loss.hip, unchanged by masks)
# against a float64 softmax of the same UNMASKED fp32 scores, measured on one
# MI355X with the scores of _scores() below, per S:
PARENT_SOFTMAX_ERR = {7: 4.7249e-08, 65: 7.5712e-09, 128: 4.3503e-09,
                      130: 4.7289e-09, 257: 2.9698e-09}


def _hf():
    from split_learning_amd.ops import functional as hf
    return hf


def _lengths(S):
    return [S, S // 2 + 1]


def _bias(B, S, neg=NEG):
    assert B == 2
    bias = torch.zeros(B, S)
    for b, n in enumerate(_lengths(S)):
        bias[b, n:] = neg
    return bias.cuda()


def _scores(B, H, S):
    g = torch.Generator().manual_seed(100 + S)
    return torch.randn(B * H, S, S, generator=g).cuda()


def _qkv(B, H, S, hd, seed=0):
    g = torch.Generator().manual_seed(seed + S)
    return [torch.randn(B * H, S, hd, generator=g).cuda() for _ in range(3)]


def _ref_probs64(scores, scale, bias, H):
    BH, S, _ = scores.shape
    x = scores.double() * float(torch.tensor(scale, dtype=torch.float32))
    if bias is not None:
        x = (x.view(BH // H, H, S, S) + bias.double()[:, None, None, :]).view(BH, S, S)
    return torch.softmax(x, dim=-1)


def _ref_attention(q, k, v, scale, bias, H, keep=None, p=0.0):
    """torch autograd graph of masked attention (same keep-mask if given)"""
    BH, S, _ = q.shape
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    s = (s.view(BH // H, H, S, S) + bias[:, None, None, :]).view(BH, S, S)
    pr = F.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep.float() / (1 - p)
    return torch.matmul(pr, v)


def _close(a, b, what, tol=1e-3):
    torch.testing.assert_close(a, b, atol=tol, rtol=tol,
                               msg=lambda m: f"{what}: {m}")


SM_SHAPES = [(2, 3, 7), (2, 3, 65), (2, 3, 128), (2, 3, 130), (2, 2, 257)]


# ---------------- 6. masked softmax forward ----------------

@pytest.mark.parametrize("B,H,S", SM_SHAPES)
def test_attn_softmax_fwd_vs_float64(B, H, S):
    """attn_softmax_fwd against softmax(scores*scale + bias) in float64 from
    the same fp32 scores.  Masked columns are exactly 0.0 (exp underflows
    below -104; |score*scale| stays under 3 here), rows sum to 1 within 1e-5,
    and valid columns are within 2x the max abs error that the softmax_fwd
    kernel shows on the same unmasked scores (PARENT_SOFTMAX_ERR).

    Measured on MI355X, max abs error vs float64 (S: softmax_fwd unmasked /
    attn_softmax_fwd masked): 7: 4.72e-8 / 2.36e-8, 65: 7.57e-9 / 7.17e-9,
    128: 4.35e-9 / 3.48e-9, 130: 4.73e-9 / 3.64e-9, 257: 2.97e-9 / 1.80e-9.
    A padded row spreads its mass over half the keys, so its probabilities
    and their fp32 ulp are twice the unmasked row's: with softmax_fwd's fp32
    sequence the kernel measured 1.59e-8 at S=65, over the 1.51e-8 bound,
    which is why it computes in fp64 and rounds once."""
    hf = _hf()
    scale = 0.5
    scores, bias = _scores(B, H, S), _bias(B, S)
    probs, dropped, mask = hf.native().attn_softmax_fwd(scores, bias, H, scale)
    assert dropped.data_ptr() == probs.data_ptr() and mask.numel() == 0
    ref = _ref_probs64(scores, scale, bias, H)
    parent = hf.native().softmax_fwd((scores * scale).reshape(-1, S))
    parent_err = (parent.double().view_as(ref)
                  - _ref_probs64(scores, scale, None, H)).abs().max().item()
    err = (probs.double() - ref).abs().max().item()
    print(f"S={S}: parent softmax_fwd max abs err {parent_err:.3e}, "
          f"attn_softmax_fwd max abs err {err:.3e}")
    pv = probs.view(B, H, S, S)
    for b, n in enumerate(_lengths(S)):
        assert (pv[b, :, :, n:] == 0.0).all(), "masked column not exactly 0"
        assert (pv[b, :, :, :n] > 0.0).all()
    assert (probs.sum(-1) - 1.0).abs().max().item() < 1e-5
    assert err <= 2.0 * PARENT_SOFTMAX_ERR[S], (err, PARENT_SOFTMAX_ERR[S])


def test_attn_softmax_fwd_no_bias_and_inf_bias():
    """key_bias=None is the zero bias; a -inf bias (what MHA feeds) gives
    exact zeros too, and a row whose keys are all -inf is NaN, as in torch."""
    hf = _hf()
    B, H, S, scale = 2, 3, 65, 0.5
    scores = _scores(B, H, S)
    zero = hf.native().attn_softmax_fwd(scores, torch.zeros(B, S).cuda(), H, scale)[0]
    assert torch.equal(hf.native().attn_softmax_fwd(scores, None, H, scale)[0], zero)
    inf_bias = _bias(B, S, float("-inf"))
    probs = hf.native().attn_softmax_fwd(scores, inf_bias, H, scale)[0]
    ref = _ref_probs64(scores, scale, inf_bias, H)
    assert (probs.double() - ref).abs().max().item() <= 2.0 * PARENT_SOFTMAX_ERR[S]
    assert (probs.view(B, H, S, S)[1, :, :, S // 2 + 1:] == 0.0).all()
    inf_bias[0, :] = float("-inf")
    probs = hf.native().attn_softmax_fwd(scores, inf_bias, H, scale)[0]
    assert probs.view(B, H, S, S)[0].isnan().all()
    assert not probs.view(B, H, S, S)[1].isnan().any()


def test_attn_softmax_checks():
    hf = _hf()
    scores = _scores(2, 3, 7)
    with pytest.raises(RuntimeError):
        hf.native().attn_softmax_fwd(scores, _bias(2, 7), 4, 0.5)   # 6 % 4
    with pytest.raises(RuntimeError):
        hf.native().attn_softmax_fwd(scores, _bias(2, 7), 2, 0.5)   # [2,7] != [3,7]
    with pytest.raises(RuntimeError):
        hf.native().attn_softmax_fwd(scores, _bias(2, 7)[:, :6], 3, 0.5)
    with pytest.raises(RuntimeError):
        hf.native().attn_fwd(scores, scores, scores, 0.5, 0.0, 0, None,
                             _bias(2, 7), 2)


# ---------------- 7. zero bias == the unmasked softmax ----------------

@pytest.mark.parametrize("B,H,S", SM_SHAPES)
def test_attn_softmax_fwd_zero_bias_is_softmax_fwd(B, H, S):
    """Zero bias against softmax_fwd(scores*scale).  Not bit-identical: the
    masked kernel computes in fp64 and rounds once (see
    test_attn_softmax_fwd_vs_float64; with softmax_fwd's fp32 sequence it was
    bit-identical at every shape here, but missed that test's bound on padded
    rows).  So the two agree within the tolerance of that test, 2x
    softmax_fwd's own max abs error."""
    hf = _hf()
    scale = 0.5
    scores = _scores(B, H, S)
    probs = hf.native().attn_softmax_fwd(scores, torch.zeros(B, S).cuda(), H, scale)[0]
    parent = hf.native().softmax_fwd((scores * scale).reshape(-1, S)).view_as(probs)
    print(f"S={S}: bit-identical to softmax_fwd: {torch.equal(probs, parent)}, "
          f"max abs diff {(probs - parent).abs().max().item():.3e}")
    assert (probs - parent).abs().max().item() <= 2.0 * PARENT_SOFTMAX_ERR[S]


# ---------------- softmax backward kernel ----------------

@pytest.mark.parametrize("B,H,S", SM_SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attn_softmax_bwd_vs_torch(B, H, S, p):
    hf = _hf()
    scale = 0.5
    scores, bias = _scores(B, H, S), _bias(B, S)
    counter = hf._counter_for(scores.device)
    counter.add_(1)
    probs, dropped, mask = hf.native().attn_softmax_fwd(
        scores, bias, H, scale, p, hf._DROPOUT_STATE["seed"], counter)
    g = torch.randn(B * H, S, S, generator=torch.Generator().manual_seed(S)).cuda()
    gs = hf.native().attn_softmax_bwd(g, probs, mask if p > 0 else None, scale, p)
    sr = scores.double().requires_grad_(True)
    pr = _ref_probs64(sr, scale, bias, H)
    if p > 0:
        pr = pr * mask.double() / (1 - p)
        _close(dropped, pr.float(), "dropped probs", 1e-5)
    pr.backward(g.double())
    _close(gs, sr.grad.float(), f"attn_softmax_bwd S={S} p={p}", 1e-5)


# ---------------- 8. attention_core with a bias, fwd + grads ----------------

def _grads_vs_ref(run, q, k, v, scale, bias, H, what):
    qo, ko, vo = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = run(qo, ko, vo)
    ref = _ref_attention(qr, kr, vr, scale, bias, H)
    _close(out, ref, f"{what} fwd")
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).cuda()
    out.backward(g)
    ref.backward(g)
    for name, a, b in (("gq", qo, qr), ("gk", ko, kr), ("gv", vo, vr)):
        assert a.grad is not None, f"{what}: {name} is None"
        _close(a.grad, b.grad, f"{what} {name}")


@pytest.mark.parametrize("B,H,S,hd", [(2, 3, 7, 16), (2, 3, 65, 32),
                                      (2, 4, 128, 64), (2, 3, 130, 16)])
def test_attention_core_key_bias_chain(B, H, S, hd, monkeypatch):
    from split_learning_amd.ops import modules
    monkeypatch.setattr(modules, "_FATTN_FORCE", False)
    q, k, v = _qkv(B, H, S, hd)
    bias = _bias(B, S)
    _grads_vs_ref(lambda a, b, c: modules.attention_core(
        a, b, c, dropout_p=0.0, training=True, key_bias=bias, heads=H),
        q, k, v, 1.0 / math.sqrt(hd), bias, H, f"chain S={S} hd={hd}")


@pytest.mark.parametrize("B,H,S,hd", [(2, 3, 7, 64), (2, 3, 65, 32),
                                      (2, 4, 128, 64)])
def test_attention_core_key_bias_one_launch(B, H, S, hd, monkeypatch):
    from split_learning_amd.ops import modules
    monkeypatch.setattr(modules, "_FATTN_FORCE", True)
    q, k, v = _qkv(B, H, S, hd)
    bias = _bias(B, S)
    _grads_vs_ref(lambda a, b, c: modules.attention_core(
        a, b, c, dropout_p=0.0, training=True, key_bias=bias, heads=H),
        q, k, v, 1.0 / math.sqrt(hd), bias, H, f"one-launch S={S} hd={hd}")
    # the kernel itself: padded keys get exactly zero probability
    probs = _hf().native().attn_fwd(q, k, v, 1.0 / math.sqrt(hd), 0.0, 0, None,
                                    bias, H)[1]
    assert (probs.view(B, H, S, S)[1, :, :, S // 2 + 1:] == 0.0).all()


# ---------------- 9. dropout ----------------

@pytest.mark.parametrize("route", ["chain", "one_launch"])
def test_attention_key_bias_dropout(route, monkeypatch):
    """Keep rate within 5 sigma of 1-p, dropped probs exactly 0 where the
    keep-mask is 0 or the key is padded, forward and grads against a torch
    graph rebuilt from the SAME keep-mask (counter rewound, as
    test_attn_fused_dropout_mask_and_grads does)."""
    from split_learning_amd.ops import modules
    hf = _hf()
    monkeypatch.setattr(modules, "_FATTN_FORCE", route == "one_launch")
    B, H, S, hd, p = 2, 4, 128, 64, 0.1
    scale = 1.0 / math.sqrt(hd)
    q, k, v = _qkv(B, H, S, hd, seed=9)
    bias = _bias(B, S)
    seed = hf._DROPOUT_STATE["seed"]
    counter = hf._counter_for(q.device)
    counter.add_(1)
    if route == "chain":
        scores = hf.matmul_f32(q, k, trans_b=True)
        probs, dropped, mask = hf.native().attn_softmax_fwd(
            scores, bias, H, scale, p, seed, counter)
        assert dropped.data_ptr() != probs.data_ptr()
        assert (dropped[mask == 0] == 0.0).all()
        assert (dropped.view(B, H, S, S)[1, :, :, S // 2 + 1:] == 0.0).all()
        kept = mask.bool()
        _close(dropped[kept], probs[kept] / (1 - p), "inverted scaling", 1e-6)
    else:
        _, probs, mask = hf.native().attn_fwd(q, k, v, scale, p, seed, counter,
                                              bias, H)
    assert mask.dtype == torch.uint8 and mask.shape == probs.shape
    assert (probs.view(B, H, S, S)[1, :, :, S // 2 + 1:] == 0.0).all()
    n = mask.numel()
    sigma = math.sqrt(p * (1 - p) / n)
    keep = mask.float().mean().item()
    print(f"{route}: keep rate {keep:.5f}, 5 sigma = {5 * sigma:.5f}")
    assert abs(keep - (1 - p)) < 5 * sigma

    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ref = _ref_attention(qr, kr, vr, scale, bias, H, keep=mask, p=p)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(4)).cuda()
    ref.backward(g)
    counter.sub_(1)     # the autograd call below draws the same mask
    qo, ko, vo = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = modules.attention_core(qo, ko, vo, dropout_p=p, training=True,
                                 key_bias=bias, heads=H)
    _close(out, ref, f"{route} dropout fwd")
    out.backward(g)
    _close(qo.grad, qr.grad, f"{route} dropout gq")
    _close(ko.grad, kr.grad, f"{route} dropout gk")
    _close(vo.grad, vr.grad, f"{route} dropout gv")


# ---------------- 10. unmasked routes did not move ----------------

@pytest.mark.parametrize("BH,S,hd", [(24, 32, 16), (12, 128, 64)])
def test_unmasked_attention_core_is_the_literal_chain(BH, S, hd, monkeypatch):
    from split_learning_amd.ops import modules
    hf = _hf()
    monkeypatch.setattr(modules, "_FATTN_FORCE", False)
    g = torch.Generator().manual_seed(BH)
    q, k, v = (torch.randn(BH, S, hd, generator=g).cuda() for _ in range(3))
    s = 1.0 / math.sqrt(hd)
    literal = hf.matmul_f32(hf.softmax_lastdim(hf.matmul_f32(q, k, trans_b=True) * s), v)
    assert torch.equal(modules.attention_core(q, k, v), literal)
    assert torch.equal(modules.attention_core(q, k, v, key_bias=None, heads=4), literal)


# ---------------- 11. HipMultiheadAttention key_padding_mask ----------------

def _mha_pair():
    from split_learning_amd.ops.modules import HipMultiheadAttention
    torch.manual_seed(1)
    ref = torch.nn.MultiheadAttention(64, 4, dropout=0.0, batch_first=True).cuda().train()
    ours = HipMultiheadAttention(64, 4, dropout=0.0, batch_first=True).cuda().train()
    ours.load_state_dict(ref.state_dict())
    return ours, ref


@pytest.mark.parametrize("route", ["mfma", "lib", "one_launch"])
@pytest.mark.parametrize("float_mask", [False, True])
def test_mha_key_padding_mask(route, float_mask, monkeypatch):
    """All three native branches honour key_padding_mask (bool -> -inf, or an
    additive float mask): outputs at valid query positions and the in_proj
    gradient match the stock module."""
    from split_learning_amd.ops import modules
    hf = _hf()
    monkeypatch.setattr(modules, "_FATTN_FORCE", route == "one_launch")
    monkeypatch.setattr(hf, "use_lib_mm", lambda *a: route == "lib")
    ours, ref = _mha_pair()
    B, S = 3, 20
    lengths = [20, 11, 1]
    kpm = torch.ones(B, S, dtype=torch.bool)
    for b, n in enumerate(lengths):
        kpm[b, :n] = False
    kpm = kpm.cuda()
    valid = ~kpm
    mask_arg = (torch.zeros(B, S).cuda().masked_fill(kpm, float("-inf"))
                if float_mask else kpm)
    x = torch.randn(B, S, 64, generator=torch.Generator().manual_seed(2)).cuda()
    x.requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    y, w = ours(x, x, x, key_padding_mask=mask_arg, need_weights=False)
    yr, _ = ref(xr, xr, xr, key_padding_mask=mask_arg, need_weights=False)
    assert w is None
    _close(y[valid], yr[valid], f"mha {route} fwd")
    # without the mask the valid positions of the padded samples differ
    y0, _ = ours(x, x, x, need_weights=False)
    assert not torch.allclose(y0[1][valid[1]], yr[1][valid[1]], atol=1e-3)
    y[valid].sum().backward()
    yr[valid].sum().backward()
    _close(ours.in_proj_weight.grad, ref.in_proj_weight.grad,
           f"mha {route} in_proj grad")
    _close(x.grad, xr.grad, f"mha {route} input grad")


def test_mha_attn_mask_and_need_weights_use_the_stock_forward():
    ours, _ = _mha_pair()
    B, S = 3, 20
    x = torch.randn(B, S, 64, generator=torch.Generator().manual_seed(2)).cuda()
    am = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1).cuda()
    stock = torch.nn.MultiheadAttention.forward
    with torch.no_grad():
        y, w = ours(x, x, x, attn_mask=am, need_weights=False)
        ys, ws = stock(ours, x, x, x, attn_mask=am, need_weights=False)
        assert torch.equal(y, ys) and w is None and ws is None
        # causal: the first query sees only key 0, so later keys cannot matter
        x2 = x.clone()
        x2[:, 1:] += 1.0
        y2, _ = ours(x2, x2, x2, attn_mask=am, need_weights=False)
        _close(y2[:, 0], y[:, 0], "attn_mask honoured", 1e-5)
        y, w = ours(x, x, x, need_weights=True)
        ys, ws = stock(ours, x, x, x, need_weights=True)
        assert torch.equal(y, ys) and torch.equal(w, ws)


# ---------------- 12. hipGraph ----------------

def test_attention_core_key_bias_graph_replay():
    """One chain, no parallel branches: a static key_bias buffer is re-read on
    replay, and the in-kernel dropout offset keeps advancing."""
    from split_learning_amd.ops import modules
    B, H, S, hd = 2, 3, 65, 32
    q, k, v = _qkv(B, H, S, hd, seed=12)
    bias_a = _bias(B, S)
    bias_b = torch.flip(bias_a, dims=[0]).contiguous()
    static_bias = bias_a.clone()

    def capture(p):
        fn = lambda: modules.attention_core(q, k, v, dropout_p=p, training=True,
                                            key_bias=static_bias, heads=H)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn()
        torch.cuda.synchronize()
        return graph, out

    with torch.no_grad():
        graph, out = capture(0.0)
        static_bias.copy_(bias_b)
        graph.replay()
        torch.cuda.synchronize()
        eager = modules.attention_core(q, k, v, key_bias=bias_b, heads=H)
        _close(out, eager, "graph replay with a new bias")
        assert not torch.allclose(
            eager, modules.attention_core(q, k, v, key_bias=bias_a, heads=H),
            atol=1e-3)

        graph, out = capture(0.1)
        graph.replay()
        torch.cuda.synchronize()
        first = out.clone()
        graph.replay()
        torch.cuda.synchronize()
        assert not torch.equal(first, out), "dropout offset did not advance"


# ---------------- 13. BERT ----------------

TINY = dict(hidden_size=32, num_attention_heads=4, intermediate_size=64,
            vocab_size=50, max_position_embeddings=16)


def test_bert_emotion_mask_gpu():
    from split_learning_amd.models.bert import BERT_EMOTION
    torch.manual_seed(0)
    model = BERT_EMOTION(start_layer=0, end_layer=4, **TINY).eval()
    B, S, lengths = 3, 12, [12, 7, 1]
    ids = torch.randint(1, TINY["vocab_size"], (B, S),
                        generator=torch.Generator().manual_seed(0))
    m = torch.zeros(B, S)
    for b, n in enumerate(lengths):
        m[b, :n] = 1.0
    with torch.no_grad():
        cpu = model(ids, attention_mask=m)
        cpu_unmasked = model(ids)
        model.cuda()
        gpu = model(ids.cuda(), attention_mask=m.cuda())
    _close(gpu.cpu(), cpu, "BERT_EMOTION masked, GPU vs CPU")
    assert not torch.allclose(cpu, cpu_unmasked, atol=1e-3)

    model.train()
    model.mask_pad_token_id = 0
    out = model((ids * m.long()).cuda())
    out.square().mean().backward()
    seen = 0
    for name, prm in model.named_parameters():
        if name.startswith(("layer2.", "layer4.")) and prm.requires_grad:
            assert prm.grad is not None, f"{name}: no gradient"
            assert torch.isfinite(prm.grad).all(), f"{name}: non-finite gradient"
            seen += 1
    assert seen == 20   # 2 blocks x (q, k, v, dense: weight+bias; LayerNorm: 2)
