"""Shared helpers of the per-route kernel tests (test_reverse_kernels.py, test_forward_kernels.py): seeded inputs already representable in a kernel's
dtype, NHWC device buffers and channel-slice views, and the stated comparison bounds.  A plain module, not a conftest."""
import zlib

import torch

DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rand(gen, *shape, dt=F32, scale=1.0, shift=0.0):
    """CPU fp64 values already representable in dt."""
    return (torch.randn(*shape, generator=gen) * scale + shift).to(dt).double()


def _q(t, dt):
    return t.to(dt).double()


def _dev(t):
    """CPU (B,C,H,W) -> device NHWC buffer allocated the way ops.new_act allocates (a 1x1 map keeps NHWC pixel strides, which
    .contiguous(memory_format=channels_last) would not give it)."""
    out = torch.empty(t.shape, dtype=t.dtype, device=DEV, memory_format=torch.channels_last)
    out.copy_(t)
    return out


def _nhwc(t, dt, off=0, extra=0, gen=None):
    """t (CPU, B,C,H,W) -> NHWC device tensor of dtype dt; with off/extra it is the channel slice [off, off + C) of a buffer with off + extra more
    channels, whose other channels hold random values (zeros without a generator).  Returns (view, whole buffer)."""
    b, c, h, w = t.shape
    if off == 0 and extra == 0:
        v = _dev(t.to(dt))
        return v, v
    big = torch.randn(b, c + off + extra, h, w, generator=gen).to(dt) if gen is not None else torch.zeros(b, c + off + extra, h, w, dtype=dt)
    big[:, off:off + c] = t.to(dt)
    big = _dev(big)
    return big[:, off:off + c], big


def _out_buf(b, c, h, w, dt, off, extra, gen):
    """Output buffer: a channel slice of a wider NHWC buffer pre-filled with random values; returns (view, buffer, CPU copy of the buffer)."""
    big0 = torch.randn(b, c + off + extra, h, w, generator=gen).to(dt)
    big = _dev(big0)
    return big[:, off:off + c], big, big0


def _borders_untouched(big, big0, off, c):
    got = big.cpu()
    assert torch.equal(got[:, :off], big0[:, :off]) and torch.equal(got[:, off + c:], big0[:, off + c:]), 'slice borders written'


def _close(got, ref, dt, what=''):
    """The stated bound for an output of dtype dt (see the test modules' docstrings)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    ref = ref.detach().double().cpu()
    assert torch.isfinite(got).all(), (what, 'non-finite output')
    err = (got - ref).abs()
    m = ref.abs().max().item()
    if dt == F32:
        rel = err.norm().item() / max(ref.norm().item(), 1e-300)
        assert err.max().item() <= 1e-4 * m and (rel <= 2e-5 or err.max().item() == 0), (what, 'rel L2', rel, 'max', err.max().item(), m)
    else:
        bound = 2.0 ** -8 * ref.abs() + 1e-3 * m
        worst = (err - bound).max().item()
        assert worst <= 0, (what, 'worst excess over the bf16 bound', worst, 'max err', err.max().item(), 'max ref', m)


def _exact(got, ref, what=''):
    got = got.detach().double().cpu().reshape(ref.shape)
    bad = (got != ref.double()).sum().item()
    assert bad == 0, (what, f'{bad} elements differ, max err {(got - ref).abs().max().item()}')
