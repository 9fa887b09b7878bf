"""Autograd wrappers around the hand-written CDNA4 HIP kernels.

Every Function here is GPU-only (callers dispatch CPU tensors to plain torch in
split_learning_amd/ops/modules.py).  Numerics are exact fp32: the GEMM-shaped ops
run on the f32-input MFMA path (v_mfma_f32_16x16x4_f32 — bitwise an fmaf chain),
matching the reference's fp32 PyTorch math (reference trains pure fp32:
src/train/VGG16.py has no dtype casts).

Kernel-side entry points live in split_learning_amd/ops/csrc/ and are exported by
the in-tree _sl_kernels extension (see ops/__init__.py loading policy).
"""

from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as _F
from torch.autograd import Function

from . import native

# Large plain GEMMs route to the platform BLAS (rocBLAS/hipBLASLt via
# torch.matmul / F.linear): measured per-model on MI355X (profiles/SUMMARY.md
# "library-GEMM routing"), our 64x64-tile MFMA kernel wins for the small/skinny
# shapes of the conv nets (VGG16 linear: 11.8k vs 10.9k samples/s) while the
# library wins ~2x for transformer shapes (ViT 3.2k vs 1.6k, KWT 1.2k vs
# 0.57k).  Thresholds are in FLOPs of the whole call, set by a GPU sweep
# (MM 1e6..5e7 x LIN 1e7..2e8); env-overridable for sweeps.  Fused / gather /
# split-K ops (conv, BN, optimizers, attention softmax) always stay on the
# hand-written kernels.
_LIB_MM_THRESH = float(os.environ.get("SLK_LIB_MM_THRESH", "1e7"))
_LIB_LIN_THRESH = float(os.environ.get("SLK_LIB_LIN_THRESH", "2e7"))


def use_lib_mm(batch, m, n, k) -> bool:
    """True when a batched matmul of this size routes to the platform BLAS."""
    return 2.0 * batch * m * n * k >= _LIB_MM_THRESH


# ---------------------------------------------------------------------------
# GEMM / Linear
# ---------------------------------------------------------------------------

def _matmul_raw(a, b, trans_a=False, trans_b=False, out=None, accumulate=False):
    """Non-differentiable strided MFMA GEMM (internal / backward use)."""
    return native().matmul_f32(a, b, trans_a, trans_b, out, accumulate)


class MatmulFn(Function):
    """Autograd for C = op(A) @ op(B): without this, the raw pybind op returns
    a detached tensor and gradient flow through the attention score/context
    matmuls silently stops (in_proj and the q/k/v projections would never
    train on GPU while the CPU fallback path trains — caught by
    tests/test_kernels_gpu.py::test_attention_core_grads)."""

    @staticmethod
    def forward(ctx, a, b, trans_a, trans_b):
        a = a.contiguous()
        b = b.contiguous()
        ctx.save_for_backward(a, b)
        ctx.trans = (trans_a, trans_b)
        return native().matmul_f32(a, b, trans_a, trans_b, None, False)

    @staticmethod
    def backward(ctx, gy):
        a, b = ctx.saved_tensors
        ta, tb = ctx.trans
        gy = gy.contiguous()
        ga = gb = None
        if ctx.needs_input_grad[0]:
            ga = (_matmul_raw(gy, b, trans_a=False, trans_b=not tb) if not ta
                  else _matmul_raw(b, gy, trans_a=tb, trans_b=True))
        if ctx.needs_input_grad[1]:
            gb = (_matmul_raw(a, gy, trans_a=not ta, trans_b=False) if not tb
                  else _matmul_raw(gy, a, trans_a=True, trans_b=ta))
        return ga, gb, None, None


def matmul_f32(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = False,
               out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """C = op(A) @ op(B) for 2-D or batched 3-D fp32 tensors (strided MFMA GEMM).

    Differentiable unless `out`/`accumulate` are used (those forms are
    internal building blocks and bypass autograd)."""
    if out is not None or accumulate:
        return native().matmul_f32(a, b, trans_a, trans_b, out, accumulate)
    m = a.shape[-1] if trans_a else a.shape[-2]
    k = a.shape[-2] if trans_a else a.shape[-1]
    n = b.shape[-2] if trans_b else b.shape[-1]
    batch = a.shape[0] if a.dim() == 3 else 1
    if 2.0 * batch * m * n * k >= _LIB_MM_THRESH:
        av = a.transpose(-1, -2) if trans_a else a
        bv = b.transpose(-1, -2) if trans_b else b
        return torch.matmul(av, bv)
    return MatmulFn.apply(a, b, trans_a, trans_b)


class LinearFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        # x: [*, K] -> flatten rows; weight: [N, K]; y = x @ w^T + b
        xs = x.reshape(-1, x.shape[-1])
        y = native().linear_fwd(xs.contiguous(), weight, bias)
        ctx.save_for_backward(xs, weight)
        ctx.has_bias = bias is not None
        ctx.x_shape = x.shape
        return y.reshape(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, gy):
        xs, weight = ctx.saved_tensors
        gys = gy.reshape(-1, gy.shape[-1]).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _matmul_raw(gys, weight)              # [M,N]x[N,K] -> [M,K]
            gx = gx.reshape(ctx.x_shape)
        if ctx.needs_input_grad[1]:
            gw = _matmul_raw(gys, xs, trans_a=True)    # [N,M]x[M,K] -> [N,K]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = native().colsum_f32(gys)
        return gx, gw, gb


def linear(x, weight, bias=None):
    rows = x.numel() // x.shape[-1]
    if 2.0 * rows * weight.shape[0] * weight.shape[1] >= _LIB_LIN_THRESH:
        return _F.linear(x, weight, bias)
    return LinearFn.apply(x, weight, bias)


# ---------------------------------------------------------------------------
# Convolution (implicit-GEMM, NCHW)
# ---------------------------------------------------------------------------

class Conv2dFn(Function):
    """Implicit-GEMM conv on the MFMA tile framework, gathering directly
    from the unpadded tensors (the bounds math measured free — conv2d.hip
    round-2 notes).  3x3 stride-1 shapes may run a Winograd kernel instead:
    native().conv_route(op, ...) names the kernel a shape takes."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, bias_grad_zero):
        x = x.contiguous()
        y = native().conv2d_fwd(x, weight, bias, stride, padding)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        ctx.padding = padding
        ctx.has_bias = bias is not None
        ctx.bias_grad_zero = bias_grad_zero
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gb = None
        gx, gw = native().conv2d_bwd(gy, x, weight, ctx.stride, ctx.padding,
                                     ctx.needs_input_grad[0],
                                     ctx.needs_input_grad[1])
        if ctx.has_bias and ctx.needs_input_grad[2]:
            if ctx.bias_grad_zero:
                # conv feeding a TRAINING-mode BatchNorm: the bias gradient is
                # analytically zero (sum over the batch of the BN-backward
                # output is gamma*invstd*(sum_gy - sum_gy - sum_gy_xhat*
                # sum(xhat)/n) and sum(xhat) == 0 by construction).  Return
                # None rather than materializing zeros: AccumulateGrad then
                # skips the parameter entirely (no fill launch, no buffer),
                # and the fused optimizers already skip None-grad params —
                # with zero grad the momentum/Adam state stays zero, so the
                # update is bit-identical to accumulating explicit zeros.
                gb = None
            else:
                gb = native().conv2d_bwd_bias(gy)
        return gx, gw, gb, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, bias_grad_zero=False):
    return Conv2dFn.apply(x, weight, bias, int(stride), int(padding),
                          bool(bias_grad_zero))


# ---------------------------------------------------------------------------
# BatchNorm2d (training + eval), optional fused ReLU
# ---------------------------------------------------------------------------

# SLK_BN_FUSED=0 restores the separate-launch BN block (stats, apply and pool
# as their own ops) for same-build A/B and bisection.  Default: training BN
# layers with chunks == 1 run as one launch per direction, and a
# BN -> ReLU -> MaxPool2d(2,2) triple runs as one op (BnReluPool2x2Fn).
BN_FUSED = os.environ.get("SLK_BN_FUSED", "1") != "0"


class BatchNorm2dFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps,
                fuse_relu, num_batches_tracked):
        x = x.contiguous()
        ctx.one_launch = training and BN_FUSED
        if ctx.one_launch:
            # batch stats + torch-exact running-stat update (unbiased var) +
            # num_batches_tracked++ + apply: one launch when a block per
            # channel covers the layer, chunked stats + apply otherwise
            y, mean, invstd = native().bn2d_train_fwd(
                x, gamma, beta, running_mean, running_var, num_batches_tracked,
                momentum, eps, fuse_relu, False)
        else:
            if training:
                mean, invstd = native().bn2d_stats_fused(
                    x, running_mean, running_var, num_batches_tracked,
                    momentum, eps)
            else:
                mean = running_mean
                invstd = (running_var + eps).rsqrt()
            y = native().bn2d_fwd(x, mean, invstd, gamma, beta, fuse_relu)
        ctx.save_for_backward(x, gamma, mean, invstd, y)
        ctx.training = training
        ctx.fuse_relu = fuse_relu
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, mean, invstd, y = ctx.saved_tensors
        gy = gy.contiguous()
        # fused ReLU backward: the mask rides inside the BN backward kernels
        # (no standalone relu_bwd launch, no extra full tensor pass)
        relu_y = y if ctx.fuse_relu else None
        if ctx.one_launch:
            gx, ggamma, gbeta = native().bn2d_train_bwd(x, gy, gamma, mean,
                                                        invstd, relu_y, None)
        elif ctx.training:
            gx, ggamma, gbeta = native().bn2d_bwd(x, gy, gamma, mean, invstd,
                                                  relu_y)
        else:
            # eval-mode backward: per-channel affine with fixed stats
            gx, ggamma, gbeta = native().bn2d_bwd_eval(x, gy, gamma, mean,
                                                       invstd, relu_y)
        return gx, ggamma, gbeta, None, None, None, None, None, None, None


def batch_norm2d(x, gamma, beta, running_mean, running_var, training, momentum=0.1,
                 eps=1e-5, fuse_relu=False, num_batches_tracked=None):
    return BatchNorm2dFn.apply(x, gamma, beta, running_mean, running_var, training,
                               momentum, eps, fuse_relu, num_batches_tracked)


class BnReluPool2x2Fn(Function):
    """Training-mode BatchNorm2d -> ReLU -> MaxPool2d(2,2) as one op (even H
    and W).  Forward writes only the pooled output and its 1-byte argmax;
    backward derives each full-resolution gradient element from the pooled
    gradient, the pooled output and the argmax inside the BN backward
    kernels.  Values are those of the three separate ops, bit for bit."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps,
                num_batches_tracked):
        x = x.contiguous()
        y, mean, invstd, idx = native().bn2d_train_fwd(
            x, gamma, beta, running_mean, running_var, num_batches_tracked,
            momentum, eps, True, True)
        ctx.save_for_backward(x, gamma, mean, invstd, y, idx)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, mean, invstd, y, idx = ctx.saved_tensors
        gx, ggamma, gbeta = native().bn2d_train_bwd(x, gy.contiguous(), gamma,
                                                    mean, invstd, y, idx)
        return gx, ggamma, gbeta, None, None, None, None, None


def bn_relu_maxpool2x2(x, gamma, beta, running_mean, running_var, momentum=0.1,
                       eps=1e-5, num_batches_tracked=None):
    return BnReluPool2x2Fn.apply(x, gamma, beta, running_mean, running_var,
                                 momentum, eps, num_batches_tracked)


# ---------------------------------------------------------------------------
# ReLU / GELU / Tanh
# ---------------------------------------------------------------------------

class ReluFn(Function):
    @staticmethod
    def forward(ctx, x):
        y = native().relu_fwd(x.contiguous())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return native().relu_bwd(gy.contiguous(), y)


def relu(x):
    return ReluFn.apply(x)


class GeluFn(Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = native().gelu_fwd(x)  # exact erf GELU (matches nn.GELU default)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return native().gelu_bwd(gy.contiguous(), x)


def gelu(x):
    return GeluFn.apply(x)


class TanhFn(Function):
    @staticmethod
    def forward(ctx, x):
        y = native().tanh_fwd(x.contiguous())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return native().tanh_bwd(gy.contiguous(), y)


def tanh(x):
    return TanhFn.apply(x)


# ---------------------------------------------------------------------------
# MaxPool2d 2x2 stride 2 (the only pooling the model zoo uses)
# ---------------------------------------------------------------------------

class MaxPool2x2Fn(Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y, idx = native().maxpool2x2_fwd(x)
        ctx.save_for_backward(idx)
        ctx.in_hw = (x.shape[2], x.shape[3])
        return y

    @staticmethod
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        return native().maxpool2x2_bwd(gy.contiguous(), idx, ctx.in_hw[0], ctx.in_hw[1])


def maxpool2x2(x):
    return MaxPool2x2Fn.apply(x)


# ---------------------------------------------------------------------------
# Dropout (philox-style counter hash; mask stashed for backward)
# ---------------------------------------------------------------------------

class DropoutFn(Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset_t):
        x = x.contiguous()
        y, mask = native().dropout_fwd_dev(x, float(p), int(seed), offset_t)
        ctx.save_for_backward(mask)
        ctx.p = float(p)
        return y

    @staticmethod
    def backward(ctx, gy):
        (mask,) = ctx.saved_tensors
        return native().dropout_bwd(gy.contiguous(), mask, ctx.p), None, None, None


# The philox-style offset lives in DEVICE memory and is bumped by a captured
# add, so dropout masks keep advancing under hipGraph replay of the step.
_DROPOUT_STATE = {"seed": 0x5EEDC0DE, "counters": {}}


def seed_dropout(seed: int) -> None:
    _DROPOUT_STATE["seed"] = int(seed) & 0xFFFFFFFFFFFFFFFF
    for c in _DROPOUT_STATE["counters"].values():
        c.zero_()


def _counter_for(device) -> torch.Tensor:
    c = _DROPOUT_STATE["counters"].get(device)
    if c is None:
        c = torch.zeros(1, dtype=torch.int64, device=device)
        _DROPOUT_STATE["counters"][device] = c
    return c


def dropout(x, p, training=True):
    if not training or p == 0.0:
        return x
    counter = _counter_for(x.device)
    counter.add_(1)
    return DropoutFn.apply(x, p, _DROPOUT_STATE["seed"], counter)


# ---------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------

class LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        xs = x.reshape(-1, x.shape[-1]).contiguous()
        y, mean, invstd = native().layernorm_fwd(xs, gamma, beta, float(eps))
        ctx.save_for_backward(xs, gamma, mean, invstd)
        ctx.x_shape = x.shape
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, gy):
        xs, gamma, mean, invstd = ctx.saved_tensors
        gys = gy.reshape(-1, gy.shape[-1]).contiguous()
        gx, ggamma, gbeta = native().layernorm_bwd(gys, xs, gamma, mean, invstd)
        return gx.reshape(ctx.x_shape), ggamma, gbeta, None


def layer_norm(x, gamma, beta, eps=1e-5):
    return LayerNormFn.apply(x, gamma, beta, eps)


class DropResLnFn(Function):
    """Fused transformer epilogue y = LayerNorm(dropout(x) + residual) in one
    kernel (norm.hip drop_res_ln_fwd; SURVEY §2.4 bias-residual-LN row — the
    bias rides in the producing GEMM).  Backward composes the existing
    layernorm_bwd + dropout_bwd kernels: the residual branch takes the LN
    input-grad directly, the dense branch takes it through the mask."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, p, seed, offset_t):
        xs = x.reshape(-1, x.shape[-1]).contiguous()
        rs = res.reshape(-1, res.shape[-1]).contiguous()
        y, h, mean, invstd, mask = native().drop_res_ln_fwd(
            xs, rs, gamma, beta, float(eps), float(p), seed, offset_t)
        ctx.save_for_backward(h, gamma, mean, invstd, mask)
        ctx.p = float(p)
        ctx.x_shape = x.shape
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, gy):
        h, gamma, mean, invstd, mask = ctx.saved_tensors
        gys = gy.reshape(-1, gy.shape[-1]).contiguous()
        gh, ggamma, gbeta = native().layernorm_bwd(gys, h, gamma, mean, invstd)
        gres = gh.reshape(ctx.x_shape)
        if ctx.p > 0.0:
            gx = native().dropout_bwd(gh, mask, ctx.p).reshape(ctx.x_shape)
        else:
            gx = gres
        return gx, gres, ggamma, gbeta, None, None, None, None


def dropout_residual_layer_norm(x, res, gamma, beta, eps=1e-12, p=0.0,
                                training=False):
    pp = float(p) if training else 0.0
    if pp > 0.0:
        counter = _counter_for(x.device)
        counter.add_(1)
        seed, offset_t = _DROPOUT_STATE["seed"], counter
    else:
        seed, offset_t = 0, None
    return DropResLnFn.apply(x, res, gamma, beta, eps, pp, seed, offset_t)


# ---------------------------------------------------------------------------
# Fused attention (small-S SDPA: S<=128, hd in {32,64} — the model zoo's regime)
# ---------------------------------------------------------------------------

class AttnFn(Function):
    """dropout(softmax(Q@K^T * scale)) @ V in ONE forward kernel
    (attention.hip): K/V live in LDS, no scores round-trip through HBM, no
    separate scale/softmax/dropout launches.  Backward reuses the GEMM +
    softmax-bwd + dropout-bwd kernels on the saved CLEAN probability matrix
    and the kernel-produced mask (identical math to the unfused path)."""

    @staticmethod
    def forward(ctx, q, k, v, scale, p, seed, offset_t, key_bias=None,
                heads=1):
        out, probs, mask = native().attn_fwd(q, k, v, scale, p, seed, offset_t,
                                             key_bias, heads)
        ctx.save_for_backward(q, k, v, probs, mask)
        ctx.scale = scale
        ctx.p = float(p)
        return out

    @staticmethod
    def backward(ctx, gy):
        q, k, v, probs, mask = ctx.saved_tensors
        gy = gy.contiguous()
        # pd = dropout(P); dV = pd^T @ gO ; dP = dropout_bwd(gO @ V^T) ;
        # dS = softmax_bwd(dP, P) * scale
        if ctx.p > 0.0:
            mflat = mask.reshape(-1, mask.shape[-1])
            pd = native().dropout_bwd(
                probs.reshape(-1, probs.shape[-1]).contiguous(), mflat,
                ctx.p).reshape(probs.shape)
        else:
            pd = probs
        gv = _matmul_raw(pd, gy, trans_a=True)
        gp = _matmul_raw(gy, v, trans_b=True)
        if ctx.p > 0.0:
            gp = native().dropout_bwd(
                gp.reshape(-1, gp.shape[-1]).contiguous(),
                mask.reshape(-1, mask.shape[-1]), ctx.p).reshape(gp.shape)
        bhs = probs.shape[0] * probs.shape[1]
        gs = native().softmax_bwd(gp.reshape(bhs, -1).contiguous(),
                                  probs.reshape(bhs, -1)).reshape(probs.shape)
        gs = gs * ctx.scale
        gq = _matmul_raw(gs, k)
        gk = _matmul_raw(gs, q, trans_a=True)
        return gq, gk, gv, None, None, None, None, None, None


def attn_fused_ok(q) -> bool:
    """fused path precondition: [BH, S<=128, hd<=64 pow2] fp32 CUDA."""
    if not (q.is_cuda and q.dim() == 3 and q.dtype == torch.float32):
        return False
    s, hd = q.shape[1], q.shape[2]
    return s <= 128 and hd <= 64 and (hd & (hd - 1)) == 0


def _key_bias_arg(key_bias):
    """additive [B, S] key bias as the kernels take it: fp32, contiguous, no
    gradient (a padding mask is constant)."""
    if key_bias is None:
        return None
    return key_bias.detach().to(torch.float32).contiguous()


def attention(q, k, v, scale, dropout_p=0.0, training=False, key_bias=None,
              heads=1):
    """Fused SDPA with optional in-kernel attention dropout;
    inputs [BH, S, hd] contiguous.  key_bias [BH/heads, S] is added to the
    scaled scores of every head and query row of its sample."""
    p = float(dropout_p) if training else 0.0
    if p > 0.0:
        counter = _counter_for(q.device)
        counter.add_(1)
        seed, offset_t = _DROPOUT_STATE["seed"], counter
    else:
        seed, offset_t = 0, None
    return AttnFn.apply(q.contiguous(), k.contiguous(), v.contiguous(), scale,
                        p, seed, offset_t, _key_bias_arg(key_bias), int(heads))


class AttnProbsFn(Function):
    """dropout(softmax(scores * scale + key_bias)) in ONE kernel per direction
    (attention.hip attn_softmax_fwd / attn_softmax_bwd): the masked GEMM
    chain's only launch between its two GEMMs.  Saves the CLEAN probs and the
    kernel-produced keep-mask; the bias is constant and gets no gradient."""

    @staticmethod
    def forward(ctx, scores, key_bias, heads, scale, p, seed, offset_t):
        probs, dropped, mask = native().attn_softmax_fwd(
            scores, key_bias, heads, scale, p, seed, offset_t)
        ctx.save_for_backward(probs, mask)
        ctx.scale = scale
        ctx.p = float(p)
        return dropped

    @staticmethod
    def backward(ctx, g):
        probs, mask = ctx.saved_tensors
        gs = native().attn_softmax_bwd(g.contiguous(), probs,
                                       mask if ctx.p > 0.0 else None,
                                       ctx.scale, ctx.p)
        return gs, None, None, None, None, None, None


def attn_probs(scores, key_bias, heads, scale, dropout_p=0.0, training=False):
    """Attention probabilities from raw [BH, S, S] scores with an additive
    [BH/heads, S] key bias (or None) and in-kernel dropout."""
    p = float(dropout_p) if training else 0.0
    if p > 0.0:
        counter = _counter_for(scores.device)
        counter.add_(1)
        seed, offset_t = _DROPOUT_STATE["seed"], counter
    else:
        seed, offset_t = 0, None
    return AttnProbsFn.apply(scores.contiguous(), _key_bias_arg(key_bias),
                             int(heads), float(scale), p, seed, offset_t)


# ---------------------------------------------------------------------------
# Softmax (last dim) — used by attention
# ---------------------------------------------------------------------------

class SoftmaxFn(Function):
    @staticmethod
    def forward(ctx, x):
        xs = x.reshape(-1, x.shape[-1]).contiguous()
        y = native().softmax_fwd(xs)
        ctx.save_for_backward(y)
        ctx.x_shape = x.shape
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gys = gy.reshape(-1, gy.shape[-1]).contiguous()
        return native().softmax_bwd(gys, y).reshape(ctx.x_shape)


def softmax_lastdim(x):
    return SoftmaxFn.apply(x)


# ---------------------------------------------------------------------------
# Cross-entropy (fused log-softmax + NLL + NaN detect, mean reduction)
# ---------------------------------------------------------------------------

class CrossEntropyFn(Function):
    @staticmethod
    def forward(ctx, logits, labels):
        logits = logits.contiguous()
        loss, probs = native().ce_fwd(logits, labels)
        ctx.save_for_backward(probs, labels)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        probs, labels = ctx.saved_tensors
        return native().ce_bwd(probs, labels, gloss), None


def cross_entropy(logits, labels):
    return CrossEntropyFn.apply(logits, labels)


# ---------------------------------------------------------------------------
# Embedding
# ---------------------------------------------------------------------------

class EmbeddingFn(Function):
    @staticmethod
    def forward(ctx, ids, weight, padding_idx):
        ids = ids.contiguous()
        y = native().embedding_fwd(ids, weight)
        ctx.save_for_backward(ids)
        ctx.num_embeddings = weight.shape[0]
        ctx.dim = weight.shape[1]
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        return y

    @staticmethod
    def backward(ctx, gy):
        (ids,) = ctx.saved_tensors
        gw = native().embedding_bwd(ids, gy.contiguous(), ctx.num_embeddings,
                                    ctx.padding_idx)
        return None, gw, None


def embedding(ids, weight, padding_idx=None):
    return EmbeddingFn.apply(ids, weight, padding_idx)


# ---------------------------------------------------------------------------
# Fused optimizers (multi-tensor)
# ---------------------------------------------------------------------------

def sgd_step(params, grads, momentum_bufs, lr, momentum, weight_decay=0.0,
             first_step=False, zero_grad_after=False):
    """Fused multi-tensor SGD+momentum matching torch.optim.SGD semantics
    (buf = m*buf + g; p -= lr*buf; first step: buf = g).  zero_grad_after
    clears grads in the same kernel (replaces zero_grad fills)."""
    native().sgd_step(list(params), list(grads), list(momentum_bufs),
                      float(lr), float(momentum), float(weight_decay),
                      bool(first_step), bool(zero_grad_after))


def adamw_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1, beta2, eps,
               weight_decay, zero_grad_after=False):
    """Fused multi-tensor AdamW matching torch.optim.AdamW."""
    native().adamw_step(list(params), list(grads), list(exp_avgs), list(exp_avg_sqs),
                        int(step), float(lr), float(beta1), float(beta2), float(eps),
                        float(weight_decay), bool(zero_grad_after))
