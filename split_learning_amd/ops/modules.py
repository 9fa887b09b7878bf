"""HIP-backed drop-in layer modules.

Each class subclasses the corresponding torch.nn module so parameter/buffer names
(and therefore state_dict keys and .pth files) are identical to the reference
models (reference src/model/VGG16_CIFAR10.py etc.).  Dispatch rule:

* input on GPU  -> hand-written CDNA4 kernels via ops.functional (REQUIRED —
  raises if the native extension is missing; no silent eager fallback);
* input on CPU  -> the stock torch forward (used by the CPU test suite and by
  server-side validation on CPU-only hosts).
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as hf


import os

# debug bisection toggles: SLK_DBG_TORCH=conv,bn,linear,pool,dropout,relu
# routes the named op families to stock torch GPU kernels (used to isolate the
# graph-replay divergence; no effect unless the env var is set)
_DBG_TORCH = frozenset((os.environ.get("SLK_DBG_TORCH") or "").split(","))


def _use_native(kind: str, x: torch.Tensor) -> bool:
    return x.is_cuda and kind not in _DBG_TORCH


def _on_gpu(x: torch.Tensor) -> bool:
    return x.is_cuda


class HipConv2d(nn.Conv2d):
    def forward(self, x, bias_grad_zero: bool = False):
        if _use_native("conv", x):
            return hf.conv2d(x, self.weight, self.bias,
                             stride=self.stride[0], padding=self.padding[0],
                             bias_grad_zero=bias_grad_zero)
        return super().forward(x)


class HipLinear(nn.Linear):
    def forward(self, x):
        if _use_native("linear", x):
            return hf.linear(x, self.weight, self.bias)
        return super().forward(x)


class HipBatchNorm2d(nn.BatchNorm2d):
    def forward(self, x, fuse_relu: bool = False, fuse_pool: bool = False):
        """fuse_pool (callers check can_fuse_bn_relu_pool first) also folds the
        following ReLU + MaxPool2d(2,2) into the op."""
        if _use_native("bn", x):
            # num_batches_tracked++ happens inside the stats finalize kernel
            nbt = (self.num_batches_tracked
                   if self.training and self.track_running_stats else None)
            if fuse_pool:
                return hf.bn_relu_maxpool2x2(x, self.weight, self.bias,
                                             self.running_mean, self.running_var,
                                             self.momentum, self.eps,
                                             num_batches_tracked=nbt)
            return hf.batch_norm2d(x, self.weight, self.bias, self.running_mean,
                                   self.running_var, self.training, self.momentum,
                                   self.eps, fuse_relu=fuse_relu,
                                   num_batches_tracked=nbt)
        y = super().forward(x)
        if fuse_pool:
            return F.max_pool2d(torch.relu(y), 2, 2)
        return torch.relu(y) if fuse_relu else y


def can_fuse_bn_relu_pool(bn, pool, x: torch.Tensor) -> bool:
    """True when bn -> HipReLU -> pool on x may run as the single fused op:
    training-mode BN on the GPU, a plain MaxPool2d(2,2), even H and W, none of
    the three families routed to torch by SLK_DBG_TORCH, SLK_BN_FUSED not 0."""
    return (hf.BN_FUSED and x.is_cuda and x.dim() == 4 and bn.training
            and x.dtype == torch.float32
            and isinstance(pool, HipMaxPool2d)
            and pool.kernel_size == 2 and pool.stride == 2
            and pool.padding == 0 and pool.dilation == 1
            and not pool.ceil_mode and not pool.return_indices
            and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and x.numel() > 0
            and _DBG_TORCH.isdisjoint(("bn", "relu", "pool")))


class HipReLU(nn.ReLU):
    def forward(self, x):
        if _use_native("relu", x):
            return hf.relu(x)
        return super().forward(x)


class HipGELU(nn.GELU):
    def forward(self, x):
        if _on_gpu(x):
            return hf.gelu(x)
        return super().forward(x)


class HipTanh(nn.Tanh):
    def forward(self, x):
        if _on_gpu(x):
            return hf.tanh(x)
        return super().forward(x)


class HipMaxPool2d(nn.MaxPool2d):
    def forward(self, x):
        if _use_native("pool", x) and self.kernel_size == 2 and self.stride == 2:
            return hf.maxpool2x2(x)
        return super().forward(x)


class HipDropout(nn.Dropout):
    def forward(self, x):
        if _use_native("dropout", x):
            return hf.dropout(x, self.p, self.training)
        return super().forward(x)


class HipLayerNorm(nn.LayerNorm):
    def forward(self, x):
        if _on_gpu(x) and len(self.normalized_shape) == 1:
            return hf.layer_norm(x, self.weight, self.bias, self.eps)
        return super().forward(x)


class HipEmbedding(nn.Embedding):
    def forward(self, ids):
        if ids.is_cuda:
            return hf.embedding(ids, self.weight, self.padding_idx)
        return super().forward(ids)


class HipMultiheadAttention(nn.MultiheadAttention):
    """Self-attention-only MHA (q=k=v, batch_first) backed by HIP GEMM+softmax.

    Parameter layout (in_proj_weight [3E,E], in_proj_bias, out_proj.*) matches
    nn.MultiheadAttention so KWT/ViT state dicts interoperate
    (reference src/model/KWT_SPEECHCOMMANDS.py:9, other/.../ViT_CIFAR10.py:7).
    """

    def forward(self, query, key, value, **kwargs):  # type: ignore[override]
        # The native path computes plain or key-padded self-attention and
        # returns no weights.  What it cannot honour goes to the stock
        # forward: an attn_mask, is_causal, or weights explicitly asked for
        # (need_weights left at its default keeps the native path, as before).
        if (not _use_native("attn", query) or (query is not key)
                or (key is not value) or not self.batch_first
                or query.dim() != 3
                or kwargs.get("attn_mask") is not None
                or kwargs.get("is_causal", False)
                or kwargs.get("need_weights", False)):
            return super().forward(query, key, value, **kwargs)
        x = query  # [B, S, E]
        B, S, E = x.shape
        H = self.num_heads
        hd = E // H
        key_bias = _key_padding_bias(kwargs.get("key_padding_mask"), B, S)
        qkv = hf.linear(x, self.in_proj_weight, self.in_proj_bias)  # [B,S,3E]
        q, k, v = qkv.split(E, dim=-1)
        scale = 1.0 / math.sqrt(hd)
        if S <= 128 and hd <= 64 and (hd & (hd - 1)) == 0 \
                and "fattn" not in _DBG_TORCH \
                and _fused_attn_worth_it(B * H, S, self.dropout, self.training):
            q = q.reshape(B, S, H, hd).permute(0, 2, 1, 3).reshape(B * H, S, hd)
            k = k.reshape(B, S, H, hd).permute(0, 2, 1, 3).reshape(B * H, S, hd)
            v = v.reshape(B, S, H, hd).permute(0, 2, 1, 3).reshape(B * H, S, hd)
            # fused SDPA kernel, in-kernel attention dropout (round 2)
            ctxv = hf.attention(q, k, v, scale, dropout_p=self.dropout,
                                training=self.training, key_bias=key_bias,
                                heads=H)
            ctxv = ctxv.reshape(B, H, S, hd).permute(0, 2, 1, 3).reshape(B, S, E)
        elif hf.use_lib_mm(B * H, S, S, hd):
            # library route (rocBLAS batched GEMM): keep [B,H,S,hd] strided
            # VIEWS end-to-end — no contiguous copies; softmax/dropout stay
            # on the fused HIP kernels
            q = q.reshape(B, S, H, hd).transpose(1, 2)
            k = k.reshape(B, S, H, hd).transpose(1, 2)
            v = v.reshape(B, S, H, hd).transpose(1, 2)
            if key_bias is not None:
                # masked: scale + bias + softmax + dropout in one launch on
                # [BH,S,S] views of the library GEMM's scores
                scores = torch.matmul(q, k.transpose(-1, -2))
                probs = hf.attn_probs(scores.reshape(B * H, S, S), key_bias,
                                      H, scale, self.dropout, self.training
                                      ).reshape(B, H, S, S)
            else:
                scores = torch.matmul(q, k.transpose(-1, -2)) * scale
                probs = hf.softmax_lastdim(scores)
                if self.dropout > 0.0:
                    probs = hf.dropout(probs, self.dropout, self.training)
            ctxv = torch.matmul(probs, v)  # [B, H, S, hd]
            ctxv = ctxv.transpose(1, 2).reshape(B, S, E)
        else:
            # native MFMA route: [B*H, S, hd] contiguous batches
            q = q.reshape(B, S, H, hd).permute(0, 2, 1, 3).reshape(B * H, S, hd)
            k = k.reshape(B, S, H, hd).permute(0, 2, 1, 3).reshape(B * H, S, hd)
            v = v.reshape(B, S, H, hd).permute(0, 2, 1, 3).reshape(B * H, S, hd)
            if key_bias is not None:
                probs = hf.attn_probs(hf.matmul_f32(q, k, trans_b=True),
                                      key_bias, H, scale, self.dropout,
                                      self.training)
            else:
                scores = hf.matmul_f32(q, k, trans_b=True) * scale
                probs = hf.softmax_lastdim(scores)
                if self.dropout > 0.0:
                    probs = hf.dropout(probs, self.dropout, self.training)
            ctxv = hf.matmul_f32(probs, v)  # [B*H, S, hd]
            ctxv = ctxv.reshape(B, H, S, hd).permute(0, 2, 1, 3).reshape(B, S, E)
        out = hf.linear(ctxv, self.out_proj.weight, self.out_proj.bias)
        return out, None


def _key_padding_bias(key_padding_mask, B, S):
    """nn.MultiheadAttention's key_padding_mask as an additive [B, S] bias:
    bool (True = ignore this key) becomes -inf, a float mask is already
    additive.  Device ops only."""
    if key_padding_mask is None:
        return None
    if tuple(key_padding_mask.shape) != (B, S):
        raise ValueError(f"key_padding_mask must be [{B}, {S}], got "
                         f"{tuple(key_padding_mask.shape)}")
    if key_padding_mask.dtype == torch.bool:
        return torch.zeros(B, S, dtype=torch.float32,
                           device=key_padding_mask.device).masked_fill_(
                               key_padding_mask, float("-inf"))
    if not key_padding_mask.is_floating_point():
        raise TypeError("key_padding_mask must be bool or floating point")
    return key_padding_mask.to(torch.float32)


_FATTN_FORCE = os.environ.get("SLK_FATTN", "0") == "1"


def _fused_attn_worth_it(bh, s_len, dropout_p, training) -> bool:
    """Round-2 A/B (profiles/SUMMARY.md): the one-launch fused SDPA kernel
    LOSES to the routed MFMA-GEMM + fused-softmax(+dropout) chain at every
    model shape, dropout or not — its grid is BH workgroups (<= 384 on the
    zoo) with scalar-FMA row sweeps, so the chip runs underfilled:
    BERT 308 vs 63 us, KWT 200 vs 56, ViT 78 vs 55.  The GEMM chain is also
    all hand-written kernels, so routing there keeps the native path.  The
    fused kernel stays available (SLK_FATTN=1 + kernel tests) pending the
    roadmap rewrite (block-per-(bh, row-tile) with MFMA scores/PV)."""
    return _FATTN_FORCE


def attention_core(q, k, v, dropout_p: float = 0.0, training: bool = False,
                   scale: Optional[float] = None, key_bias=None,
                   heads: int = 1):
    """scaled-dot-product attention on [B*H, S, hd] tensors via HIP kernels.

    key_bias ([B, S] additive float, B = q.shape[0] // heads) is added to the
    scaled scores of every head and query row of its sample before the
    softmax: a padding mask.  Without it every route is the unmasked one."""
    hd = q.shape[-1]
    s = scale if scale is not None else 1.0 / math.sqrt(hd)
    if key_bias is not None:
        return _attention_core_biased(q, k, v, dropout_p, training, s,
                                      key_bias, heads)
    if (_use_native("attn", q) and "fattn" not in _DBG_TORCH and q.dim() == 3
            and q.shape[1] <= 128 and hd <= 64 and (hd & (hd - 1)) == 0
            and _fused_attn_worth_it(q.shape[0], q.shape[1], dropout_p,
                                     training)):
        # fused SDPA kernel, attention dropout included in-kernel
        return hf.attention(q, k, v, s, dropout_p=dropout_p, training=training)
    if _use_native("attn", q):
        scores = hf.matmul_f32(q, k, trans_b=True) * s
        probs = hf.softmax_lastdim(scores)
        if dropout_p > 0.0:
            probs = hf.dropout(probs, dropout_p, training)
        return hf.matmul_f32(probs, v)
    scores = torch.matmul(q, k.transpose(-1, -2)) * s
    probs = F.softmax(scores, dim=-1)
    if dropout_p > 0.0:
        probs = F.dropout(probs, dropout_p, training)
    return torch.matmul(probs, v)


def _attention_core_biased(q, k, v, dropout_p, training, s, key_bias, heads):
    """attention_core with an additive key bias; same three routes."""
    hd = q.shape[-1]
    if q.dim() != 3 or q.shape[0] % heads != 0 or \
            tuple(key_bias.shape) != (q.shape[0] // heads, q.shape[1]):
        raise ValueError(
            f"key_bias must be [B*H / heads, S] for q {tuple(q.shape)} and "
            f"heads={heads}, got {tuple(key_bias.shape)}")
    if (_use_native("attn", q) and "fattn" not in _DBG_TORCH
            and q.shape[1] <= 128 and hd <= 64 and (hd & (hd - 1)) == 0
            and _fused_attn_worth_it(q.shape[0], q.shape[1], dropout_p,
                                     training)):
        return hf.attention(q, k, v, s, dropout_p=dropout_p, training=training,
                            key_bias=key_bias, heads=heads)
    if _use_native("attn", q):
        # GEMM -> ONE scale+bias+softmax+dropout launch -> GEMM
        scores = hf.matmul_f32(q, k, trans_b=True)
        probs = hf.attn_probs(scores, key_bias, heads, s, dropout_p, training)
        return hf.matmul_f32(probs, v)
    BH, S, _ = q.shape
    scores = torch.matmul(q, k.transpose(-1, -2)) * s
    scores = (scores.view(BH // heads, heads, S, S)
              + key_bias.to(scores.dtype)[:, None, None, :]).view(BH, S, S)
    probs = F.softmax(scores, dim=-1)
    if dropout_p > 0.0:
        probs = F.dropout(probs, dropout_p, training)
    return torch.matmul(probs, v)
