"""Restatement of mode CSP_C3 of mgdt_csp_block_fwd (csrc/csp_c3.hip) and of the launch in front of it, in plain torch on the CPU, built on kernel_ref
like ref_csp_block.  `dt` = float64 is the reference; rnd=False drops every rounding point (the soundness test compares that with the chain of plain
convolutions)."""
import torch

from kernel_ref import BF16, ConvP, _rb, _silu  # noqa: F401


def ref_c3_front(x, cv1, cv2, dt=torch.float64, rnd=True):
    """[a | b] = silu([cv1 | cv2](x)): ONE 1x1 launch over the concatenated weights (mgdt_conv2d_fwd); stored as bf16."""
    ab = torch.cat([_silu(cv1(x.to(dt), dt)), _silu(cv2(x.to(dt), dt))], 1)
    return _rb(ab) if rnd else ab


def ref_c3_block(ab, mids, shortcut, back, dt=torch.float64, rnd=True):
    """ab = [a | b] (B, 2 wd, H, W), mids = ConvP pairs (1x1, 3x3) per bottleneck, back = ConvP of cv3 over [m_n(a) | b]; every conv = Conv + folded BN (or
    bias) + SiLU with zero padding.  Rounding points read off the kernel: P, T and P' live in LDS as bf16 (c3_store4); the shortcut adds the bf16 P to the
    fp32 SiLU output before the one rounding of P'; b is copied.  Returns y BEFORE its final rounding to bf16."""
    r = _rb if rnd else (lambda t: t)
    ab = ab.to(dt)
    wd = mids[0].cout
    p, b = ab[:, :wd], ab[:, wd:]
    for j in range(0, len(mids), 2):
        t = r(_silu(mids[j](p, dt)))
        q = _silu(mids[j + 1](t, dt))
        p = r(q + p if shortcut else q)
    return _silu(back(torch.cat([p, b], 1), dt))
