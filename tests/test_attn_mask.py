"""Attention padding masks on the CPU route: BERT attention_mask through
BERT_EMOTION / BERT_AGNEWS against a plain-torch re-implementation of the
reference formula (scores/sqrt(hd) + (1 - mask) * -10000, softmax, @V) run with
the same weights, padding independence, the pad-id-derived mask, and the
loader's pad_token_id.  Both sides are CPU fp32, so the tolerance is 1e-5.
"""

import math

import pytest
import torch
import torch.nn.functional as F

from split_learning_amd.models.bert import (BERT_AGNEWS, BERT_EMOTION,
                                            BertSdpaSelfAttention)
from split_learning_amd.ops.modules import attention_core

TINY = dict(hidden_size=32, num_attention_heads=4, intermediate_size=64,
            vocab_size=50, max_position_embeddings=16)
B, S = 3, 12
LENGTHS = [12, 7, 1]
TOL = dict(atol=1e-5, rtol=1e-5)


def _mask():
    m = torch.zeros(B, S)
    for b, n in enumerate(LENGTHS):
        m[b, :n] = 1.0
    return m


def _ids(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, TINY["vocab_size"], (B, S), generator=g)


def _emotion():
    torch.manual_seed(0)
    return BERT_EMOTION(start_layer=0, end_layer=4, **TINY).eval()


def _agnews():
    torch.manual_seed(0)
    return BERT_AGNEWS(start_layer=0, end_layer=3, **TINY).eval()


# ---- plain-torch reference (stock ops only, the model's own weights) --------

def _lin(m, x):
    return F.linear(x, m.weight, m.bias)


def _ln(m, x):
    return F.layer_norm(x, m.normalized_shape, m.weight, m.bias, m.eps)


def _ref_embeddings(emb, ids):
    pos = torch.arange(ids.size(1)).unsqueeze(0).expand_as(ids)
    e = (F.embedding(ids, emb.word_embeddings.weight)
         + F.embedding(pos, emb.position_embeddings.weight)
         + F.embedding(torch.zeros_like(ids), emb.token_type_embeddings.weight))
    return _ln(emb.LayerNorm, e)


def _ref_self_attention(att, x, mask):
    b, s, e = x.shape
    h, hd = att.num_attention_heads, att.attention_head_size

    def heads(t):
        return t.view(b, s, h, hd).permute(0, 2, 1, 3)

    q, k, v = heads(_lin(att.query, x)), heads(_lin(att.key, x)), heads(_lin(att.value, x))
    scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    if mask is not None:
        scores = scores + ((1.0 - mask.float()) * -10000.0)[:, None, None, :]
    probs = torch.softmax(scores, dim=-1)
    return torch.matmul(probs, v).permute(0, 2, 1, 3).reshape(b, s, e)


def _ref_out(mod, h, residual):
    return _ln(mod.LayerNorm, _lin(mod.dense, h) + residual)


def _ref_emotion(model, ids, mask):
    x = _ref_embeddings(model.layer1, ids)
    x = _ref_out(model.layer2[1], _ref_self_attention(model.layer2[0], x, mask), x)
    x = _ref_out(model.layer3[1], F.gelu(_lin(model.layer3[0].dense, x)), x)
    x = _ref_out(model.layer4[1], _ref_self_attention(model.layer4[0], x, mask), x)
    return x


def _ref_agnews(model, ids, mask):
    x = _ref_embeddings(model.layer1, ids)
    for layer in (model.layer2, model.layer3):
        a = _ref_out(layer.attention.output,
                     _ref_self_attention(layer.attention.self, x, mask), x)
        x = _ref_out(layer.output, F.gelu(_lin(layer.intermediate.dense, a)), a)
    return x


def _valid(t):
    """rows of [B, S, E] at valid (non-pad) positions"""
    return torch.cat([t[b, :n] for b, n in enumerate(LENGTHS)])


def _repadded(ids):
    """the same valid tokens, other ids at the padded positions"""
    other = ids.clone()
    for b, n in enumerate(LENGTHS):
        other[b, n:] = (ids[b, n:] + 17) % (TINY["vocab_size"] - 1) + 1
    assert not torch.equal(other, ids)
    return other


# ---- tests ------------------------------------------------------------------

def _check_matches_reference(model, ref_fn, call):
    ids, m = _ids(), _mask()
    with torch.no_grad():
        out = call(model, ids, m)
        torch.testing.assert_close(out, ref_fn(model, ids, m), **TOL)
        # the all-ones mask is the unmasked model; a zero in the mask moves it
        torch.testing.assert_close(call(model, ids, torch.ones(B, S)),
                                   ref_fn(model, ids, None), **TOL)
        assert not torch.allclose(out, call(model, ids, None), atol=1e-4)
        # any dtype: bool and int masks give the float mask's result
        assert torch.equal(out, call(model, ids, m.bool()))
        assert torch.equal(out, call(model, ids, m.long()))


def _check_padding_independence(model, call):
    ids, m = _ids(), _mask()
    with torch.no_grad():
        a = call(model, ids, m)
        b = call(model, _repadded(ids), m)
    torch.testing.assert_close(_valid(a), _valid(b), **TOL)


def _call_emotion(model, ids, m):
    return model(ids, attention_mask=m)


def _call_agnews(model, ids, m):
    return model(input_ids=ids, attention_mask=m)


def test_emotion_mask_matches_reference_formula():
    _check_matches_reference(_emotion(), _ref_emotion, _call_emotion)


def test_emotion_padding_independence():
    _check_padding_independence(_emotion(), _call_emotion)


def test_agnews_mask_matches_reference_formula():
    _check_matches_reference(_agnews(), _ref_agnews, _call_agnews)


def test_agnews_padding_independence():
    _check_padding_independence(_agnews(), _call_agnews)


def test_masked_key_probabilities_are_exactly_zero():
    """exp(-10000 - max) underflows in fp32: padded keys get probability 0,
    so V rows at padded keys cannot reach the output at all."""
    torch.manual_seed(1)
    h, hd = 4, 8
    q, k, v = (torch.randn(B * h, S, hd) for _ in range(3))
    bias = (1.0 - _mask()) * -10000.0
    out = attention_core(q, k, v, key_bias=bias, heads=h)
    v2 = v.clone().view(B, h, S, hd)
    for b, n in enumerate(LENGTHS):
        v2[b, :, n:] = 1e6
    assert torch.equal(out, attention_core(q, k, v2.view(B * h, S, hd),
                                           key_bias=bias, heads=h))
    with pytest.raises(ValueError):
        attention_core(q, k, v, key_bias=bias[:2], heads=h)


def _parent_self_attention_forward(self, hidden_states, attention_mask=None):
    """BertSdpaSelfAttention.forward as it was before masks: straight through
    attention_core(q, k, v)."""
    b, s, e = hidden_states.shape
    h, hd = self.num_attention_heads, self.attention_head_size

    def heads(t):
        return t.view(b, s, h, hd).permute(0, 2, 1, 3).reshape(b * h, s, hd).contiguous()

    ctx = attention_core(heads(self.query(hidden_states)),
                         heads(self.key(hidden_states)),
                         heads(self.value(hidden_states)),
                         dropout_p=self.dropout.p, training=self.training)
    return ctx.reshape(b, h, s, hd).permute(0, 2, 1, 3).reshape(b, s, e)


@pytest.mark.parametrize("make,call", [(_emotion, _call_emotion),
                                       (_agnews, _call_agnews)])
def test_pad_id_derived_mask_and_unmasked_identity(make, call, monkeypatch):
    model = make()
    assert model.mask_pad_token_id is None
    ids, m = _ids(), _mask()
    ids = ids * m.long()                      # trailing zeros = pad id 0
    with torch.no_grad():
        explicit = call(model, ids, m)
        unmasked = call(model, ids, None)
        model.mask_pad_token_id = 0
        assert torch.equal(call(model, ids, None), explicit)
        # an explicit mask wins over the derived one
        assert torch.equal(call(model, ids, torch.ones(B, S)), unmasked)
        model.mask_pad_token_id = None
        assert torch.equal(call(model, ids, None), unmasked)
        monkeypatch.setattr(BertSdpaSelfAttention, "forward",
                            _parent_self_attention_forward)
        assert torch.equal(call(model, ids, None), unmasked)


def test_later_partition_stays_unmasked_without_a_mask():
    """A partition without layer 1 never sees ids: the pad id does nothing
    there, an explicit mask still does."""
    torch.manual_seed(0)
    model = BERT_EMOTION(start_layer=1, end_layer=4, **TINY).eval()
    x = torch.randn(B, S, TINY["hidden_size"])
    with torch.no_grad():
        plain = model(x)
        model.mask_pad_token_id = 0
        assert torch.equal(model(x), plain)
        assert not torch.allclose(model(x, attention_mask=_mask()), plain, atol=1e-4)


def test_lora_composes_with_mask():
    from split_learning_amd.models.lora import apply_lora
    model = _emotion()
    apply_lora(model, r=2, alpha=4, dropout=0.0,
               target_modules=("query", "key", "value", "dense"))
    model.eval()
    ids, m = _ids(), _mask()
    with torch.no_grad():
        a = model(ids, attention_mask=m)
        b = model(_repadded(ids), attention_mask=m)
    torch.testing.assert_close(_valid(a), _valid(b), **TOL)


def test_synthetic_loader_has_no_pad_id():
    from split_learning_amd.data import data_loader
    loader = data_loader("AGNEWS", batch_size=4, distribution=[2, 2, 2, 2])
    assert loader.pad_token_id is None
    from split_learning_amd.data.real import pad_token_id
    assert pad_token_id("AGNEWS") == 0
    assert pad_token_id("CIFAR10") is None
