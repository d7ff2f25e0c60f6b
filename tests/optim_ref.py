"""float64 restatements of the Adam / AdamW / RMSProp kernels of csrc/optim.hip (beside kernel_ref.ref_sgd / ref_ema), with every scalar as
the kernel receives it: derived on the host in Python floats (1 - beta, lr / bc1, sqrt(bc2)), then rounded to fp32 once."""
import torch

from kernel_ref import f32r


def _group_lr(w, lr, lr_bias):
    return torch.where(w < 0, torch.full_like(w, f32r(lr_bias)), torch.full_like(w, f32r(lr)))


def ref_adam(p, g, m, v, wd, lr, lr_bias, beta1, beta2, eps, step, decoupled, coef):
    """mgdt_adam_step in float64: returns the new (p, m, v).  wd[i] > 0 decays (coupled: added to the gradient; decoupled: p *= 1 - lr*wd),
    wd[i] < 0 is the bias group stepping with lr_bias, coef the clip coefficient (1 without)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    w = torch.zeros_like(p) if wd is None else wd.double()
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    gi = coef * g
    if decoupled:
        p = torch.where(w > 0, p * (1.0 - f32r(lr) * w), p)
    else:
        gi = gi + torch.where(w > 0, w * p, torch.zeros_like(p))
    m = m + (gi - m) * f32r(1 - beta1)
    v = f32r(beta2) * v + f32r(1 - beta2) * gi * gi
    denom = v.sqrt() / f32r(bc2 ** 0.5) + f32r(eps)
    return p - _group_lr(w, lr / bc1, lr_bias / bc1) * m / denom, m, v


def ref_rmsprop(p, g, sq, buf, wd, lr, lr_bias, alpha, eps, momentum, coef):
    """mgdt_rmsprop_step in float64: returns the new (p, sq, buf); buf is returned unchanged when momentum is 0."""
    p, g, sq = p.double(), g.double(), sq.double()
    w = torch.zeros_like(p) if wd is None else wd.double()
    gi = coef * g + torch.where(w > 0, w * p, torch.zeros_like(p))
    sq = f32r(alpha) * sq + f32r(1 - alpha) * gi * gi
    avg = sq.sqrt() + f32r(eps)
    lrs = _group_lr(w, lr, lr_bias)
    if momentum > 0:
        buf = f32r(momentum) * buf.double() + gi / avg
        return p - lrs * buf, sq, buf
    return p - lrs * gi / avg, sq, buf
