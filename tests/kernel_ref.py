"""Shared helpers of the per-route kernel tests (test_reverse_kernels.py, test_forward_kernels.py, test_tood_kernels.py): seeded inputs already representable in a kernel's
dtype, NHWC device buffers and channel-slice views, the stated comparison bounds, and the float64 deformable-conv reference pieces.  A plain module, not a conftest."""
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


# ------------------------------------------------------------------------------------------------ deformable conv (test_tood_kernels.py)
def _dcn_offsets(gen, b, h, w):
    """(B, 18, H, W) offsets k/8, k uniform in [-40, 40]: exact in bf16 and fp32, so every sampling coordinate is exact in fp32 and fp64 alike and
    kernel and reference take floor() on the same side; one coordinate in eight is an integer."""
    return torch.randint(-40, 41, (b, 18, h, w), generator=gen).double() / 8


def _dcn_coords(offset):
    """Sampling coordinates (hy, wx), each (B, 9, H, W), of oracle.tood.modulated_deform_conv3x3."""
    b, _, h, w = offset.shape
    k = torch.arange(9)
    ys = torch.arange(h, dtype=offset.dtype).view(1, 1, h, 1) - 1 + (k // 3).to(offset.dtype).view(1, 9, 1, 1)
    xs = torch.arange(w, dtype=offset.dtype).view(1, 1, 1, w) - 1 + (k % 3).to(offset.dtype).view(1, 9, 1, 1)
    return ys + offset[:, 0:18:2], xs + offset[:, 1:18:2]


def _dcn_census(offset):
    """Number of (pixel, tap) pairs of each kind, from the reference's sampling rule alone: fully outside; exactly on the open gate (-1, H or W);
    inside with exactly 1 / 2 / 4 corners in the image (3 cannot happen); inside on an integer coordinate; inside on the last row / column."""
    _, _, h, w = offset.shape
    hy, wx = _dcn_coords(offset)
    inside = (hy > -1) & (wx > -1) & (hy < h) & (wx < w)
    h0, w0 = torch.floor(hy), torch.floor(wx)
    nh = (h0 >= 0).long() + (h0 + 1 <= h - 1).long()
    nw = (w0 >= 0).long() + (w0 + 1 <= w - 1).long()
    nv = nh * nw
    assert not (inside & (nv == 3)).any() and not (inside & (nv == 0)).any()
    return {'outside': int((~inside).sum()), 'gate': int(((hy == -1) | (hy == h) | (wx == -1) | (wx == w)).sum()),
            'one': int((inside & (nv == 1)).sum()), 'two': int((inside & (nv == 2)).sum()), 'four': int((inside & (nv == 4)).sum()),
            'integer': int((inside & ((hy == h0) | (wx == w0))).sum()), 'last': int((inside & ((hy == h - 1) | (wx == w - 1))).sum()),
            'inside_mask': inside}


def _dcn_kinds(h, w):
    """The kinds a map of this size can contain: a 1-pixel-wide axis always has exactly one valid corner, so 'two' needs one such axis at most and
    'four' none."""
    kinds = ['outside', 'gate', 'integer', 'last']
    if h == 1 and w == 1:
        return kinds + ['one']
    if h == 1 or w == 1:
        return kinds + ['one', 'two']
    return kinds + ['one', 'two', 'four']


def _dcn_draw(key, b, h, w):
    """Seeded offsets whose census holds every kind the map can contain.  Whole maps are redrawn (salt 0, 1, ...) until it does: at 7x5 and above
    the first draw has them all; the nine taps of a 1x1 map need some tens of draws.  Returns (generator to go on drawing from, offsets)."""
    for salt in range(4096):
        gen = _gen(*key, b, h, w, salt)
        off = _dcn_offsets(gen, b, h, w)
        cen = _dcn_census(off)
        if all(cen[k] > 0 for k in _dcn_kinds(h, w)):
            return gen, off
    raise AssertionError(('no offset map with every tap kind', key, b, h, w))


def _dcn_columns(x, offset, mask):
    """The column part of oracle.tood.modulated_deform_conv3x3 (mmcv modulated_deformable_im2col), dtype-generic and differentiable:
    (B, C*9, H, W) in channel-major, tap-minor order, so that the convolution is weight.view(cout, cin*9) @ columns."""
    b, c, h, w = x.shape
    hy, wx = _dcn_coords(offset)
    inside = (hy > -1) & (wx > -1) & (hy < h) & (wx < w)
    h0f, w0f = torch.floor(hy), torch.floor(wx)
    lh, lw = hy - h0f, wx - w0f
    h0, w0 = h0f.long(), w0f.long()
    h1, w1 = h0 + 1, w0 + 1
    xf = x.reshape(b, c, 1, h * w).expand(b, c, 9, h * w)
    val = torch.zeros(b, c, 9, h, w, dtype=x.dtype)
    for hh, ww, cf, ok in ((h0, w0, (1 - lh) * (1 - lw), (h0 >= 0) & (w0 >= 0)), (h0, w1, (1 - lh) * lw, (h0 >= 0) & (w1 <= w - 1)),
                           (h1, w0, lh * (1 - lw), (h1 <= h - 1) & (w0 >= 0)), (h1, w1, lh * lw, (h1 <= h - 1) & (w1 <= w - 1))):
        idx = (hh.clamp(0, h - 1) * w + ww.clamp(0, w - 1)).reshape(b, 1, 9, h * w).expand(b, c, 9, h * w)
        val = val + torch.gather(xf, 3, idx).reshape(b, c, 9, h, w) * (cf * (ok & inside)).unsqueeze(1)
    return (val * mask.unsqueeze(1)).reshape(b, c * 9, h, w)
