"""Plain float64 definitions of the ops, on the CPU.

Each function is the textbook formula in torch double, a few lines, with no
call into the package under test and no call to the torch op it stands for
(tests/test_f64_reference.py checks each against that torch op in double).
Inputs are fp32 test inputs; every function upcasts what it is given.
tests/test_small_kernels_f64_gpu.py, tests/test_gemm_conv_f64_gpu.py and
tests/test_wino_f64_gpu.py compare the HIP kernels with these.  The Winograd
functions at the end take a dtype: they are the conv again, by the kernels'
algorithm.
"""

import math

import torch


def _d(t):
    return t.detach().to(device="cpu", dtype=torch.float64)


# ---------------- optimizers ----------------

def sgd_step(p, g, buf, lr, momentum, weight_decay, first):
    """torch.optim.SGD, dampening 0: returns (p, buf)."""
    p, g, buf = _d(p), _d(g), _d(buf)
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        buf = g.clone() if first else momentum * buf + g
        g = buf
    return p - lr * g, buf


def adamw_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay):
    """torch.optim.AdamW (decoupled decay): returns (p, m, v)."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    p = p * (1.0 - lr * weight_decay)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    mhat = m / (1.0 - beta1 ** step)
    vhat = v / (1.0 - beta2 ** step)
    return p - lr * mhat / (vhat.sqrt() + eps), m, v


# ---------------- softmax / cross-entropy ----------------

def softmax(x):
    x = _d(x)
    e = torch.exp(x - x.max(dim=-1, keepdim=True).values)
    return e / e.sum(dim=-1, keepdim=True)


def softmax_bwd(gy, y):
    gy, y = _d(gy), _d(y)
    return y * (gy - (gy * y).sum(dim=-1, keepdim=True))


def cross_entropy(logits, labels, upstream=1.0):
    """mean over rows of logsumexp(row) - row[label]; returns (loss,
    upstream * dloss/dlogits)."""
    x = _d(logits)
    lab = labels.detach().cpu().long()
    B = x.shape[0]
    m = x.max(dim=1, keepdim=True).values
    lse = m.squeeze(1) + torch.log(torch.exp(x - m).sum(dim=1))
    loss = (lse - x[torch.arange(B), lab]).sum() / B
    grad = softmax(x)
    grad[torch.arange(B), lab] -= 1.0
    return loss, grad * (upstream / B)


# ---------------- LayerNorm ----------------

def layer_norm(x, gamma, beta, eps):
    """returns (y, mean, invstd) over the last dim, biased variance."""
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    mean = x.sum(dim=-1, keepdim=True) / x.shape[-1]
    var = ((x - mean) ** 2).sum(dim=-1, keepdim=True) / x.shape[-1]
    invstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * invstd * gamma + beta, mean.squeeze(-1), invstd.squeeze(-1)


def layer_norm_bwd(gy, x, gamma, eps):
    """returns (gx, dgamma, dbeta)."""
    gy, x, gamma = _d(gy), _d(x), _d(gamma)
    D = x.shape[-1]
    mean = x.sum(dim=-1, keepdim=True) / D
    invstd = 1.0 / torch.sqrt(((x - mean) ** 2).sum(dim=-1, keepdim=True) / D + eps)
    xhat = (x - mean) * invstd
    gg = gy * gamma
    gx = invstd * (gg - gg.sum(dim=-1, keepdim=True) / D
                   - xhat * (gg * xhat).sum(dim=-1, keepdim=True) / D)
    return gx, (gy * xhat).sum(dim=0), gy.sum(dim=0)


# ---------------- BatchNorm2d ----------------

def _chan(t):
    return t.reshape(1, -1, 1, 1)


def batch_norm_train(x, gamma, beta, running_mean, running_var, momentum, eps):
    """returns (y, mean, invstd, new_running_mean, new_running_var): biased
    variance normalises, unbiased variance feeds the running estimate."""
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    n = x.numel() // x.shape[1]
    mean = x.sum(dim=(0, 2, 3)) / n
    var = ((x - _chan(mean)) ** 2).sum(dim=(0, 2, 3)) / n
    invstd = 1.0 / torch.sqrt(var + eps)
    y = (x - _chan(mean)) * _chan(invstd * gamma) + _chan(beta)
    rm = (1.0 - momentum) * _d(running_mean) + momentum * mean
    rv = (1.0 - momentum) * _d(running_var) + momentum * var * (n / max(n - 1, 1))
    return y, mean, invstd, rm, rv


def batch_norm_train_bwd(gy, x, gamma, eps):
    """returns (gx, ggamma, gbeta) of training-mode batch norm."""
    gy, x, gamma = _d(gy), _d(x), _d(gamma)
    n = x.numel() // x.shape[1]
    mean = x.sum(dim=(0, 2, 3)) / n
    invstd = 1.0 / torch.sqrt(((x - _chan(mean)) ** 2).sum(dim=(0, 2, 3)) / n + eps)
    xhat = (x - _chan(mean)) * _chan(invstd)
    gbeta = gy.sum(dim=(0, 2, 3))
    ggamma = (gy * xhat).sum(dim=(0, 2, 3))
    gx = _chan(gamma * invstd) * (gy - _chan(gbeta) / n - xhat * _chan(ggamma) / n)
    return gx, ggamma, gbeta


def batch_norm_eval(x, gamma, beta, running_mean, running_var, eps):
    x = _d(x)
    invstd = 1.0 / torch.sqrt(_d(running_var) + eps)
    return (x - _chan(_d(running_mean))) * _chan(invstd * _d(gamma)) + _chan(_d(beta))


# ---------------- activations ----------------

def relu(x):
    x = _d(x)
    return torch.where(x < 0, torch.zeros_like(x), x)  # NaN stays NaN


def relu_bwd(gy, x):
    return torch.where(_d(x) <= 0, torch.zeros_like(_d(gy)), _d(gy))


def gelu(x):
    x = _d(x)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_bwd(gy, x):
    x = _d(x)
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return _d(gy) * (cdf + x * pdf)


def tanh(x):
    x = _d(x)
    # (e^x - e^-x)/(e^x + e^-x) written so that neither exp overflows
    e = torch.exp(-2.0 * x.abs())
    return torch.sign(x) * (1.0 - e) / (1.0 + e)


def tanh_bwd(gy, x):
    t = tanh(x)
    return _d(gy) * (1.0 - t * t)


# ---------------- maxpool 2x2 stride 2 ----------------

def maxpool2x2(x):
    """floor mode: the odd last row/column is dropped."""
    x = _d(x)
    B, C, H, W = x.shape
    w = x[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2)
    return w.permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4).max(dim=-1).values


# ---------------- matmul / linear ----------------

def matmul(a, b, trans_a=False, trans_b=False):
    """C[..., m, n] = sum_k A[..., m, k] B[..., k, n], one rank-1 term per k."""
    a, b = _d(a), _d(b)
    if trans_a:
        a = a.transpose(-1, -2)
    if trans_b:
        b = b.transpose(-1, -2)
    c = torch.zeros(*a.shape[:-1], b.shape[-1], dtype=torch.float64)
    for k in range(a.shape[-1]):
        c += a[..., :, k, None] * b[..., k, None, :]
    return c


def linear(x, w, bias=None):
    """y[m, n] = sum_k x[m, k] w[n, k] + bias[n]"""
    y = matmul(x, w, trans_b=True)
    return y if bias is None else y + _d(bias)


# ---------------- conv2d ----------------
# x [B, Ci, H, W], w [Co, Ci, KH, KW], y [B, Co, OH, OW] with
# OH = (H + 2 pad - KH) // stride + 1; tap (kh, kw) of output (oh, ow) reads
# the zero-padded input at (oh stride + kh, ow stride + kw).

def _taps(w_shape, OH, OW, stride):
    """(kh, kw, row slice, column slice) of the padded plane for every tap"""
    for kh in range(w_shape[2]):
        for kw in range(w_shape[3]):
            yield (kh, kw, slice(kh, kh + (OH - 1) * stride + 1, stride),
                   slice(kw, kw + (OW - 1) * stride + 1, stride))


def _padded(x, pad):
    B, C, H, W = x.shape
    xp = torch.zeros(B, C, H + 2 * pad, W + 2 * pad, dtype=torch.float64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    return xp


def conv_out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def conv2d(x, w, bias=None, stride=1, pad=0):
    x, w = _d(x), _d(w)
    OH, OW = conv_out_hw(x.shape[2], x.shape[3], w.shape[2], w.shape[3], stride, pad)
    xp = _padded(x, pad)
    y = torch.zeros(x.shape[0], w.shape[0], OH, OW, dtype=torch.float64)
    for kh, kw, rows, cols in _taps(w.shape, OH, OW, stride):
        # [B, 1, Ci, OH, OW] * [1, Co, Ci, 1, 1] summed over Ci
        y += (xp[:, None, :, rows, cols] * w[None, :, :, kh, kw, None, None]).sum(dim=2)
    return y if bias is None else y + _chan(_d(bias))


def conv2d_bwd_data(gy, w, stride, pad, H, W):
    """gx: every tap scatters gy * w back to the input position it read."""
    gy, w = _d(gy), _d(w)
    OH, OW = gy.shape[2], gy.shape[3]
    gxp = torch.zeros(gy.shape[0], w.shape[1], H + 2 * pad, W + 2 * pad,
                      dtype=torch.float64)
    for kh, kw, rows, cols in _taps(w.shape, OH, OW, stride):
        # [B, Co, 1, OH, OW] * [1, Co, Ci, 1, 1] summed over Co
        gxp[:, :, rows, cols] += (gy[:, :, None] * w[None, :, :, kh, kw, None, None]).sum(dim=1)
    return gxp[:, :, pad:pad + H, pad:pad + W]


def conv2d_bwd_weight(gy, x, KH, KW, stride, pad):
    gy, x = _d(gy), _d(x)
    OH, OW = gy.shape[2], gy.shape[3]
    xp = _padded(x, pad)
    gw = torch.zeros(gy.shape[1], x.shape[1], KH, KW, dtype=torch.float64)
    for kh, kw, rows, cols in _taps(gw.shape, OH, OW, stride):
        # [B, Co, 1, OH, OW] * [B, 1, Ci, OH, OW] summed over B, OH, OW
        gw[:, :, kh, kw] = (gy[:, :, None] * xp[:, None, :, rows, cols]).sum(dim=(0, 3, 4))
    return gw


def conv2d_bwd_bias(gy):
    return _d(gy).sum(dim=(0, 2, 3))


# ---------------- Winograd F(2x2, 3x3) ----------------
# The 3x3 stride-1 conv as the Winograd kernels compute it, from the three
# matrices in the header of csrc/wino_math.h, in the dtype asked for: float64
# to tie the algebra to conv2d above, float32 as the comparison implementation
# of the tolerance rule (the same algorithm as the kernels, in plain torch).
# Tile (th, tw) owns output pixels (2 th.., 2 tw..) and reads the 4x4 patch of
# the zero-padded input whose corner is (2 th, 2 tw).  The _abs forms apply
# |B^T|, |G|, |A| to |x|, |w|, |gy|: the sum of the magnitudes of every term
# an output is made of, which bounds what rounding can do to it.

WINO_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
WINO_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
WINO_A = [[1, 0], [1, 1], [1, -1], [0, -1]]


def _wino_operands(dtype, absolute, *tensors):
    """(B^T, G, A) and the tensors, on the CPU in dtype; |.| of all if asked"""
    ts = [torch.tensor(m, dtype=dtype) for m in (WINO_BT, WINO_G, WINO_A)]
    ts += [None if t is None else t.detach().to(device="cpu", dtype=dtype)
           for t in tensors]
    return [t.abs() if absolute and t is not None else t for t in ts]


def _wino_V(x, pad, Bt):
    """B^T d B of every tile's patch: [B, Ci, tH, tW, 4, 4]"""
    B, C, H, W = x.shape
    assert (H + 2 * pad) % 2 == 0 and (W + 2 * pad) % 2 == 0, "even outputs only"
    xp = torch.zeros(B, C, H + 2 * pad, W + 2 * pad, dtype=x.dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)
    return torch.einsum("ij,bcthjk,lk->bcthil", Bt, d, Bt)


def _wino_conv2d(x, w, bias, pad, dtype, absolute):
    Bt, G, A, x, w, bias = _wino_operands(dtype, absolute, x, w, bias)
    V = _wino_V(x, pad, Bt)
    U = torch.einsum("ij,ocjk,lk->ocil", G, w, G)             # G g G^T
    M = torch.einsum("ocil,bcthil->bothil", U, V)
    Y = torch.einsum("ji,bothjk,kl->bothil", A, M, A)         # A^T M A
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(x.shape[0], w.shape[0],
                                            2 * Y.shape[2], 2 * Y.shape[3])
    return y if bias is None else y + _chan(bias)


def _wino_conv2d_bwd_weight(gy, x, pad, dtype, absolute):
    Bt, G, A, gy, x = _wino_operands(dtype, absolute, gy, x)
    V = _wino_V(x, pad, Bt)
    assert gy.shape[2:] == (2 * V.shape[2], 2 * V.shape[3]), "geometry"
    g = gy.unfold(2, 2, 2).unfold(3, 2, 2)                    # [B, Co, tH, tW, 2, 2]
    Wg = torch.einsum("ij,bothjk,lk->bothil", A, g, A)        # A gy A^T
    dU = torch.einsum("bothil,bcthil->ocil", Wg, V)
    return torch.einsum("ji,ocjk,kl->ocil", G, dU, G)         # G^T dU G


def wino_conv2d(x, w, bias=None, pad=1, dtype=torch.float64):
    """y = A^T [ (G g G^T) .* (B^T d B) ] A, summed over Ci, per 2x2 tile"""
    return _wino_conv2d(x, w, bias, pad, dtype, False)


def wino_conv2d_abs(x, w, bias=None, pad=1, dtype=torch.float64):
    return _wino_conv2d(x, w, bias, pad, dtype, True)


def wino_conv2d_bwd_weight(gy, x, pad=1, dtype=torch.float64):
    """gw = G^T [ (A gy A^T) .* (B^T d B) ] G, summed over the tiles"""
    return _wino_conv2d_bwd_weight(gy, x, pad, dtype, False)


def wino_conv2d_bwd_weight_abs(gy, x, pad=1, dtype=torch.float64):
    return _wino_conv2d_bwd_weight(gy, x, pad, dtype, True)


# ---------------- embedding ----------------

def embedding(ids, w):
    return _d(w)[ids.detach().cpu().long()]


def embedding_bwd(ids, gy, num_embeddings, padding_idx=None):
    ids = ids.detach().cpu().long().reshape(-1)
    gy = _d(gy).reshape(ids.numel(), -1)
    if padding_idx is not None:
        gy = gy * (ids != padding_idx).unsqueeze(1)
    gw = torch.zeros(num_embeddings, gy.shape[1], dtype=torch.float64)
    return gw.index_add_(0, ids, gy)
