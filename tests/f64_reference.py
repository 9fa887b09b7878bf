"""Plain float64 definitions of the small ops, on the CPU.

Each function is the textbook formula in torch double, a few lines, with no
call into the package under test and no call to the torch op it stands for
(tests/test_f64_reference.py checks each against that torch op in double).
Inputs are fp32 test inputs; every function upcasts what it is given.
tests/test_small_kernels_f64_gpu.py compares the HIP kernels with these.
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
