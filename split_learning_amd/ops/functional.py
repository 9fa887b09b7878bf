"""Autograd wrappers around the hand-written CDNA4 HIP kernels.

Every Function here is GPU-only (callers dispatch CPU tensors to plain torch in
split_learning_amd/ops/modules.py).  By default numerics are exact fp32: the
GEMM-shaped ops run on the f32-input MFMA path (v_mfma_f32_16x16x4_f32 — bitwise
an fmaf chain), matching the reference's fp32 PyTorch math (reference trains
pure fp32: src/train/VGG16.py has no dtype casts).

The one opt-in exception is the bf16-operand GEMM of linear() and lora_linear()
(compute="bf16", or SLK_GEMM=bf16 for the calls that otherwise leave HIP for
the platform BLAS): tensors, master weights, accumulation, bias, outputs and
gradients stay fp32, and only the multiplier's operands are rounded to bf16
(nearest even) on their way into LDS (csrc/gemm_bf16.hip).  Each product is
then the fp32 sum of exact products of the rounded operands; what that does to
a model's accuracy beyond the recorded BERT loss is not measured.

The tiled attention kernels have the same opt-in (attention_tiled() and
attention_heads() compute="bf16", or SLK_ATTN=bf16 for the calls that take the
tiled route anyway; csrc/attention_tiled_bf16.hip): q, k, v, the upstream
gradient, the probabilities and dS are rounded to bf16 as MFMA operands; the
scores' sum, the softmax, lse, delta and every accumulator stay fp32.

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


class Bf16LinearFn(Function):
    """LinearFn on the bf16-operand MFMA GEMM (gemm_bf16.hip): NT forward, NN
    for gx, TN (split into slabs, summed in order) for gW.  gb is colsum_f32
    below _LIB_LIN_THRESH, as in LinearFn, and gys.sum(0) from there on, as on
    LoraLinearFn's BLAS-sized route: colsum_f32 is one thread per column
    walking all M rows, and at M = 3168 it alone took the KWT step from 5.6 to
    32 ms (profiles/SUMMARY.md "bf16 MFMA GEMM").  Everything it reads, saves
    and returns is fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        xs = x.reshape(-1, x.shape[-1]).contiguous()
        y = native().linear_bf16_fwd(xs, weight, bias)
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
            gx = native().linear_bf16_bwd_input(gys, weight).reshape(ctx.x_shape)
        if ctx.needs_input_grad[1]:
            gw = native().linear_bf16_bwd_weight(gys, xs)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            flops = 2.0 * gys.shape[0] * weight.shape[0] * weight.shape[1]
            gb = (gys.sum(0) if flops >= _LIB_LIN_THRESH
                  else native().colsum_f32(gys))
        return gx, gw, gb


# SLK_GEMM=bf16 makes "bf16" the default `compute` of linear() and
# lora_linear(): the calls that otherwise go to the platform BLAS take the
# bf16-operand kernels instead (profiles/SUMMARY.md "bf16 MFMA GEMM").
_GEMM_DEFAULT = "bf16" if os.environ.get("SLK_GEMM", "") == "bf16" else "fp32"


def _bf16_fail(x, weight) -> Optional[str]:
    """the condition of linear_bf16_ok that x, weight miss, or None"""
    if not (torch.is_tensor(x) and torch.is_tensor(weight)
            and x.is_cuda and weight.is_cuda):
        return "x and weight must be CUDA tensors"
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        return "x and weight must be float32"
    if weight.dim() != 2 or not weight.is_contiguous():
        return "weight must be a dense [N, K] matrix"
    n, k = weight.shape
    if x.dim() < 1 or x.shape[-1] != k:
        return f"x must be [..., K={k}]"
    if k % 8 or n % 8 or k == 0 or n == 0:
        return f"K={k} and N={n} must be positive multiples of 8"
    if x.numel() == 0:
        return "x must have at least one row"
    if x.data_ptr() % 16 or weight.data_ptr() % 16:
        return "data pointers must be 16-byte aligned"
    return None


def linear_bf16_ok(x, weight) -> bool:
    """bf16 GEMM precondition: fp32 CUDA tensors, weight dense [N, K],
    x [..., K] with at least one row, K % 8 == 0, N % 8 == 0, 16-byte-aligned
    data pointers.  The row count M is free."""
    return _bf16_fail(x, weight) is None


def _takes_bf16(x, weight, compute) -> bool:
    """does this Linear-shaped product run on the bf16 kernels?  An explicit
    compute="bf16" must (ValueError if it cannot); the SLK_GEMM=bf16 default
    takes only the calls that would otherwise go to the platform BLAS."""
    if compute not in (None, "fp32", "bf16"):
        raise ValueError(f"compute must be None, 'fp32' or 'bf16', got {compute!r}")
    if compute == "bf16":
        why = _bf16_fail(x, weight)
        if why is not None:
            raise ValueError(f"compute='bf16': {why}")
        return True
    if compute == "fp32" or _GEMM_DEFAULT != "bf16":
        return False
    rows = x.numel() // max(x.shape[-1], 1)
    return (2.0 * rows * weight.shape[0] * weight.shape[1] >= _LIB_LIN_THRESH
            and linear_bf16_ok(x, weight))


def linear(x, weight, bias=None, compute=None):
    """compute: "fp32" (the fp32 routes), "bf16" (bf16 multiplier operands,
    any size linear_bf16_ok admits), None (the module default: "fp32", or
    under SLK_GEMM=bf16 the bf16 kernels for the platform-BLAS-sized calls)."""
    if _takes_bf16(x, weight, compute):
        return Bf16LinearFn.apply(x, weight, bias)
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
# LoRA linear (lora.hip): base GEMM + fused adapter
# ---------------------------------------------------------------------------

class LoraLinearFn(Function):
    """out = x W^T + b + scaling * (dropout(x) A^T) B^T.  The base product and
    g @ W keep the route linear() gives them (platform BLAS above
    _LIB_LIN_THRESH, the MFMA GEMM below, the bf16-operand GEMM where
    `bf16` says so); everything else stays fp32 and is one launch
    forward (lora_fwd, in place on the base output) and three backward
    (lora_bwd: rows, weight gradients, slab sum).  Saves x, W, A, B, xa [M,r]
    and the one-element offset the forward read: no xd, mask or delta."""

    @staticmethod
    def forward(ctx, x, weight, bias, lora_A, lora_B, scaling, p, seed, offset_t,
                bf16=False):
        xs = x.reshape(-1, x.shape[-1]).contiguous()
        lib = 2.0 * xs.shape[0] * weight.shape[0] * weight.shape[1] >= _LIB_LIN_THRESH
        if bf16:
            y = native().linear_bf16_fwd(xs, weight, bias)
        elif lib:
            y = _F.linear(xs, weight, bias)
        else:
            y = native().linear_fwd(xs, weight, bias)
        lora_A, lora_B = lora_A.contiguous(), lora_B.contiguous()
        xa, used = native().lora_fwd(y, xs, lora_A, lora_B, scaling, p, seed,
                                     offset_t)
        ctx.save_for_backward(xs, weight, lora_A, lora_B, xa, used)
        ctx.args = (scaling, p, seed, lib, bias is not None, x.shape, bf16)
        return y.reshape(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, gy):
        xs, weight, lora_A, lora_B, xa, used = ctx.saved_tensors
        scaling, p, seed, lib, has_bias, x_shape, bf16 = ctx.args
        gys = gy.reshape(-1, gy.shape[-1]).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if bf16:
                gx = native().linear_bf16_bwd_input(gys, weight)
            else:
                gx = torch.matmul(gys, weight) if lib else _matmul_raw(gys, weight)
        gA, gB = native().lora_bwd(gys, xs, lora_A, lora_B, xa, gx, scaling, p,
                                   seed, used)
        if ctx.needs_input_grad[1]:
            if bf16:
                gw = native().linear_bf16_bwd_weight(gys, xs)
            else:
                gw = (torch.matmul(gys.t(), xs) if lib
                      else _matmul_raw(gys, xs, trans_a=True))
        if has_bias and ctx.needs_input_grad[2]:
            gb = gys.sum(0) if lib else native().colsum_f32(gys)
        if gx is not None:
            gx = gx.reshape(x_shape)
        return gx, gw, gb, gA, gB, None, None, None, None, None


def lora_ok(x, weight, lora_A, lora_B) -> bool:
    """fused adapter precondition: fp32 CUDA tensors, x [..., K], W [N,K],
    A [r,K], B [N,r], 1 <= r <= 16, K % 4 == 0, N % 4 == 0."""
    ts = (x, weight, lora_A, lora_B)
    if not all(t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    if x.dim() < 1 or weight.dim() != 2 or lora_A.dim() != 2 or lora_B.dim() != 2:
        return False
    n, k = weight.shape
    r = lora_A.shape[0]
    return (1 <= r <= 16 and k % 4 == 0 and n % 4 == 0 and x.shape[-1] == k
            and lora_A.shape[1] == k and tuple(lora_B.shape) == (n, r)
            and x.data_ptr() % 16 == 0)


def lora_linear(x, weight, bias, lora_A, lora_B, scaling, dropout_p=0.0,
                training=False, compute=None):
    """Linear with a LoRA adapter on the fused kernels; dropout(x) draws from
    dropout()'s stream: same counter, same keep decisions.  compute: as in
    linear(), for the base product and its gradients; the adapter is fp32."""
    bf16 = _takes_bf16(x, weight, compute)
    p = float(dropout_p) if training else 0.0
    if p > 0.0:
        counter = _counter_for(x.device)
        counter.add_(1)
        seed, offset_t = _DROPOUT_STATE["seed"], counter
    else:
        seed, offset_t = 0, None
    return LoraLinearFn.apply(x, weight, bias, lora_A, lora_B, float(scaling),
                              p, seed, offset_t, bf16)


class LoraQkvFn(Function):
    """Three LoraLinearFn on one x (the query, key and value projections of a
    self-attention block) with the adapters grouped: one launch forward
    (lora_qkv_fwd), three backward (lora_qkv_bwd).  Returns the packed
    [..., 3N] tensor whose column thirds are q, k, v, which is the layout
    attention_heads(packed=) reads and whose gradient it returns whole.

    The three base products keep linear()'s route and its dense stores
    (neither route's GEMM targets a column third without a copy: the MFMA
    store is dense row-major, and the BLAS route through a strided out= was
    not measured); the forward kernel reads them and writes the thirds, so an
    element is still read once and written once.  g_j W_j accumulate into one
    gx buffer, each route in its own accumulate form, and read the thirds of
    the packed gradient in place.  Saves x, the W_j, A_j, B_j, xa [3,M,r] and
    the one-element offset of q's mask: no xd, mask or delta."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, bq, bk, bv, aq, ak, av, b_q, b_k, b_v,
                scaling, p, seed, offset_t):
        xs = x.reshape(-1, x.shape[-1]).contiguous()
        ws, bs = (wq, wk, wv), (bq, bk, bv)
        n, k = wq.shape
        lib = 2.0 * xs.shape[0] * n * k >= _LIB_LIN_THRESH
        base = [_F.linear(xs, w, b) if lib else native().linear_fwd(xs, w, b)
                for w, b in zip(ws, bs)]
        las = [t.contiguous() for t in (aq, ak, av)]
        lbs = [t.contiguous() for t in (b_q, b_k, b_v)]
        out = xs.new_empty(xs.shape[0], 3 * n)
        xa, used = native().lora_qkv_fwd(out, base, xs, las, lbs, scaling, p,
                                         seed, offset_t)
        ctx.save_for_backward(xs, *ws, *las, *lbs, xa, used)
        ctx.args = (scaling, p, seed, lib, [b is not None for b in bs], x.shape)
        return out.reshape(*x.shape[:-1], 3 * n)

    @staticmethod
    def backward(ctx, gy):
        xs, *rest = ctx.saved_tensors
        ws, las, lbs, (xa, used) = rest[0:3], rest[3:6], rest[6:9], rest[9:]
        scaling, p, seed, lib, has_bias, x_shape = ctx.args
        n = ws[0].shape[0]
        g = gy.reshape(-1, 3 * n)
        if g.stride(1) != 1 or g.stride(0) % 4 or g.data_ptr() % 16:
            g = g.contiguous()
        gs = g.split(n, dim=1)          # strided thirds: both GEMM routes and
        gx = None                       # the kernels read them in place
        if ctx.needs_input_grad[0]:
            if lib:
                gx = torch.matmul(gs[0], ws[0])
                for j in (1, 2):
                    gx.addmm_(gs[j], ws[j])
            else:
                gx = _matmul_raw(gs[0], ws[0])
                for j in (1, 2):
                    _matmul_raw(gs[j], ws[j], out=gx, accumulate=True)
        gA, gB = native().lora_qkv_bwd(g, xs, las, lbs, xa, gx, scaling, p,
                                       seed, used)
        gw, gb = [None] * 3, [None] * 3
        for j in range(3):
            if ctx.needs_input_grad[1 + j]:
                gw[j] = (torch.matmul(gs[j].t(), xs) if lib
                         else _matmul_raw(gs[j], xs, trans_a=True))
            if has_bias[j] and ctx.needs_input_grad[4 + j]:
                # colsum_f32 reads a dense matrix: it copies its third
                gb[j] = gs[j].sum(0) if lib else native().colsum_f32(gs[j])
        if gx is not None:
            gx = gx.reshape(x_shape)
        return (gx, *gw, *gb, *gA.unbind(0), *gB.unbind(0), None, None, None,
                None)


def lora_qkv_ok(x, weights, lora_As, lora_Bs) -> bool:
    """grouped adapter precondition: three (W, A, B) that each pass lora_ok
    on x and have one shape (so one N, K and r)."""
    if not len(weights) == len(lora_As) == len(lora_Bs) == 3:
        return False
    return all(lora_ok(x, w, a, b) and w.shape == weights[0].shape
               and a.shape == lora_As[0].shape
               for w, a, b in zip(weights, lora_As, lora_Bs))


def lora_qkv(x, weights, biases, lora_As, lora_Bs, scaling, dropout_p=0.0,
             training=False):
    """[lora_linear(x, W_j, b_j, A_j, B_j) for j in q, k, v], concatenated
    along the last dimension, on the grouped kernels.  The dropout counter
    advances by 3 and the three masks are drawn at the values three
    lora_linear calls in q, k, v order would have read, so the forward has
    their bits and every later draw of the stream is where it was."""
    p = float(dropout_p) if training else 0.0
    if p > 0.0:
        counter = _counter_for(x.device)
        counter.add_(3)
        seed, offset_t = _DROPOUT_STATE["seed"], counter
    else:
        seed, offset_t = 0, None
    return LoraQkvFn.apply(x, *weights, *biases, *lora_As, *lora_Bs,
                           float(scaling), p, seed, offset_t)


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


class AttnTiledFn(Function):
    """Tiled MFMA attention (attention_tiled.hip): one forward launch with an
    online softmax, two backward launches that recompute the probabilities
    from lse and redraw the dropout mask from the offset the forward read.
    Saves q, k, v, out, lse [BH,S] and that one-element offset tensor (plus
    the [B,S] bias): nothing of size S^2."""

    bf16 = False   # which kernels: AttnTiledBf16Fn sets it

    @classmethod
    def forward(cls, ctx, q, k, v, scale, p, seed, offset_t, key_bias=None,
                heads=1, is_causal=False):
        out, lse, used = native().attn_tiled_fwd(q, k, v, scale, p, seed,
                                                 offset_t, key_bias, heads,
                                                 is_causal, cls.bf16)
        ctx.save_for_backward(q, k, v, out, lse, used, key_bias)
        ctx.args = (scale, float(p), seed, heads, is_causal)
        return out

    @classmethod
    def backward(cls, ctx, gy):
        q, k, v, out, lse, used, key_bias = ctx.saved_tensors
        scale, p, seed, heads, is_causal = ctx.args
        gq, gk, gv = native().attn_tiled_bwd(gy, q, k, v, out, lse, scale, p,
                                             seed, used, key_bias, heads,
                                             is_causal, cls.bf16)
        return gq, gk, gv, None, None, None, None, None, None, None


class AttnTiledBf16Fn(AttnTiledFn):
    """AttnTiledFn on the bf16-operand kernels (attention_tiled_bf16.hip):
    same arguments, same saved state, same dropout decisions."""
    bf16 = True


# SLK_ATTN=bf16 makes "bf16" the default `compute` of attention_tiled() and
# attention_heads(): the calls that take the tiled route anyway run its
# bf16-operand kernels.  It never changes which route a caller takes.
_ATTN_DEFAULT = "bf16" if os.environ.get("SLK_ATTN", "") == "bf16" else "fp32"


def _attn_bf16(compute, ok: bool, rule: str) -> bool:
    """do the tiled kernels run with bf16 operands?  compute as in linear();
    an explicit "bf16" must (ValueError naming the precondition, `rule`, if
    `ok` does not hold); the SLK_ATTN=bf16 default never raises."""
    if compute not in (None, "fp32", "bf16"):
        raise ValueError(f"compute must be None, 'fp32' or 'bf16', got {compute!r}")
    if compute == "bf16":
        if not ok:
            raise ValueError(f"compute='bf16': needs {' '.join(rule.split())}")
        return True
    return compute is None and _ATTN_DEFAULT == "bf16" and ok


def attn_tiled_ok(q, k, v) -> bool:
    """tiled path precondition: three [BH, S, hd in {32, 64}] fp32 CUDA
    tensors of one shape; any S >= 1."""
    return (torch.is_tensor(q) and torch.is_tensor(k) and torch.is_tensor(v)
            and q.is_cuda and q.dim() == 3 and q.dtype == torch.float32
            and q.shape[2] in (32, 64) and q.shape[1] >= 1
            and k.shape == q.shape and v.shape == q.shape
            and k.dtype == q.dtype and v.dtype == q.dtype)


def attention_tiled(q, k, v, scale, dropout_p=0.0, training=False,
                    key_bias=None, heads=1, is_causal=False, compute=None):
    """attention() on the tiled kernels: same arguments, same dropout counter
    and keep decisions, any S.  is_causal: query row i attends to keys <= i
    (the kernels skip the key tiles above the diagonal; no mask tensor).
    compute: "fp32", "bf16" (the bf16-operand kernels; ValueError unless
    attn_tiled_ok holds) or None (the default: "fp32", or "bf16" under
    SLK_ATTN=bf16)."""
    fn = AttnTiledBf16Fn if _attn_bf16(
        compute, attn_tiled_ok(q, k, v), attn_tiled_ok.__doc__) else AttnTiledFn
    p = float(dropout_p) if training else 0.0
    if p > 0.0:
        counter = _counter_for(q.device)
        counter.add_(1)
        seed, offset_t = _DROPOUT_STATE["seed"], counter
    else:
        seed, offset_t = 0, None
    return fn.apply(q.contiguous(), k.contiguous(), v.contiguous(),
                    float(scale), p, seed, offset_t, _key_bias_arg(key_bias),
                    int(heads), bool(is_causal))


class AttnHeadsFn(Function):
    """The tiled kernels on the projections' own layout (attention_tiled.hip,
    head-strided instantiations): q, k, v are [B,S,E] views with a unit last
    stride, out is [B,S,E] dense, no permute copy on either side.

    x is q, or, with k and v None, the dense [B,S,3E] tensor whose three
    E-wide column slices are q, k, v: its gradient is then the one [B,S,3E]
    buffer the backward kernels fill, and autograd has nothing to assemble.
    Saves the operand views, out, lse [B*heads,S], the used-offset tensor and
    the bias: nothing of size S^2."""

    bf16 = False   # which kernels: AttnHeadsBf16Fn sets it

    @classmethod
    def forward(cls, ctx, x, k, v, heads, scale, p, seed, offset_t,
                key_bias=None, is_causal=False):
        ctx.packed = k is None
        q, k, v = x.split(x.shape[-1] // 3, dim=-1) if ctx.packed else (x, k, v)
        out, lse, used = native().attn_heads_fwd(q, k, v, heads, scale, p, seed,
                                                 offset_t, key_bias, is_causal,
                                                 cls.bf16)
        ctx.save_for_backward(q, k, v, out, lse, used, key_bias)
        ctx.args = (heads, scale, float(p), seed, is_causal)
        return out

    @classmethod
    def backward(cls, ctx, gy):
        q, k, v, out, lse, used, key_bias = ctx.saved_tensors
        heads, scale, p, seed, is_causal = ctx.args
        g = native().attn_heads_bwd(gy, q, k, v, out, lse, heads, scale, p,
                                    seed, used, key_bias, is_causal, cls.bf16)
        if ctx.packed:
            return (g[3],) + (None,) * 9
        return g[0], g[1], g[2], None, None, None, None, None, None, None


class AttnHeadsBf16Fn(AttnHeadsFn):
    """AttnHeadsFn on the bf16-operand kernels (attention_tiled_bf16.hip)."""
    bf16 = True


def attn_heads_ok(q, k, v, heads) -> bool:
    """attention_heads' precondition: three [B, S, E = heads * hd] fp32 CUDA
    tensors of one shape, hd in {32, 64}, S >= 1, B * heads within the grid;
    unit last stride, row and batch strides multiples of 4 floats and
    16-byte-aligned bases (the kernels move float4s)."""
    if not (torch.is_tensor(q) and torch.is_tensor(k) and torch.is_tensor(v)
            and q.is_cuda and q.dim() == 3 and q.dtype == torch.float32
            and heads >= 1 and q.shape[2] % heads == 0
            and q.shape[2] // heads in (32, 64) and q.shape[1] >= 1
            and q.shape[0] * heads <= 65535):
        return False
    return all(t.shape == q.shape and t.dtype == q.dtype
               and t.device == q.device and t.stride(2) == 1
               and (t.shape[1] == 1 or t.stride(1) % 4 == 0)
               and (t.shape[0] == 1 or t.stride(0) % 4 == 0)
               and t.data_ptr() % 16 == 0 for t in (q, k, v))


def _packed_base(q, k, v, base):
    """base (default: the tensor q is a view of) if it is a dense [B,S,3E]
    tensor whose column thirds are exactly q, k, v; else None"""
    base = q._base if base is None else base
    B, S, E = q.shape
    if (base is None or tuple(base.shape) != (B, S, 3 * E)
            or base.dtype != q.dtype or not base.is_contiguous()):
        return None
    at = base.data_ptr()
    step = E * q.element_size()
    if ((q.data_ptr(), k.data_ptr(), v.data_ptr())
            == (at, at + step, at + 2 * step)
            and q.stride() == k.stride() == v.stride() == base.stride()):
        return base
    return None


def attention_heads(q, k, v, heads, scale, dropout_p=0.0, training=False,
                    key_bias=None, packed=None, is_causal=False, compute=None):
    """attention_tiled() without the head permutes: q, k, v [B,S,E] as the
    projections wrote them (three tensors, or three column views of one packed
    [B,S,3E]), result [B,S,E] as the output projection reads it.  Head h is
    columns [h*hd, (h+1)*hd); key_bias is [B,S].  Same dropout counter and
    keep decisions as attention_tiled on the permuted operands; is_causal as
    there.

    packed names the [B,S,3E] tensor q, k, v were split from, for a caller
    whose q._base is not that tensor (a view of a view reports the root).
    compute: as in attention_tiled, against attn_heads_ok."""
    fn = AttnHeadsBf16Fn if _attn_bf16(
        compute, attn_heads_ok(q, k, v, int(heads)),
        attn_heads_ok.__doc__) else AttnHeadsFn
    p = float(dropout_p) if training else 0.0
    if p > 0.0:
        counter = _counter_for(q.device)
        counter.add_(1)
        seed, offset_t = _DROPOUT_STATE["seed"], counter
    else:
        seed, offset_t = 0, None
    base = _packed_base(q, k, v, packed)
    if base is not None:
        q, k, v = base, None, None
    return fn.apply(q, k, v, int(heads), float(scale), p, seed, offset_t,
                    _key_bias_arg(key_bias), bool(is_causal))


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
