"""fp64 references of the optimiser's extras (csrc/optim.hip): the global gradient norm with torch.nn.utils.clip_grad_norm_'s
coefficient, and the chain coefficient -> Adam or AdamW -> moving average of the weights.  tests/test_optim_host.py
holds the chain to torch.optim.Adam / AdamW in fp64; tests/test_gpu_optim.py holds the kernels to the chain."""
import numpy as np
import torch

from oracle import seld_oracle as O

CLIP_EPS = float(np.float32(1e-6))          # the constant the kernel adds to the norm, as fp32 holds it


def scaled_gradient(g32, grad_scale):
    """g * grad_scale rounded to fp32 (the product the kernels form), as fp64."""
    return (g32.float() * torch.tensor(grad_scale, dtype=torch.float32)).double()


def grad_norm(g32, grad_scale):
    """||fl32(g * grad_scale)||_2 with the squares and the sum in fp64 (a Python float; may be inf or nan)."""
    x = scaled_gradient(g32, grad_scale)
    return float((x * x).sum().sqrt())


def clip_coefficient(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1) -- 0 for an infinite norm, nan for nan."""
    c = torch.tensor(max_norm, dtype=torch.float64) / (torch.tensor(norm, dtype=torch.float64) + CLIP_EPS)
    return float(torch.clamp(c, max=1.0))


def ema_decay_at(step, ema_decay):
    """d_t = min(ema_decay, (1 + step) / (10 + step)) for the 1-based step."""
    return min(float(ema_decay), (1.0 + step) / (10.0 + step))


def adam_ex_step(p, g, m, v, ema, step, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False,
                 grad_scale=1.0, coef=1.0, ema_decay=0.0):
    """One step of the chain on fp64 tensors: (p, m, v, ema) afterwards (ema None stays None).  The gradient is
    (g * grad_scale) * coef; weight decay joins it (L2, torch.optim.Adam) or, decoupled, shrinks p by 1 - lr * wd first
    (torch.optim.AdamW); then the moments and the update (oracle.adam_step); then ema <- d ema + (1 - d) p_new."""
    g = (g * grad_scale) * coef
    if decoupled:
        p = p * (1.0 - lr * weight_decay)
        weight_decay = 0.0
    p, m, v = O.adam_step(p, g, m, v, step, lr=lr, b1=b1, b2=b2, eps=eps, weight_decay=weight_decay, grad_scale=1.0)
    if ema is not None:
        d = ema_decay_at(step, ema_decay)
        ema = d * ema + (1.0 - d) * p
    return p, m, v, ema
