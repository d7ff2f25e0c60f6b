"""Shared helpers of the per-route kernel tests (test_reverse_kernels.py, test_forward_kernels.py, test_tood_kernels.py, test_block_kernels.py,
test_conv_kernels.py, test_cnx_kernels.py, test_stem_direct_kernels.py): seeded inputs already representable in a kernel's dtype, NHWC device buffers and channel-slice views, the stated comparison bounds,
the float64 deformable-conv reference pieces, the restatements of the fused forward block kernels, of the fused convolution and of the ConvNeXtV2
kernels with their flip allowance.  A plain module, not a
conftest."""
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


def _bound_use(got, ref, dt):
    """Largest fraction of _close's bound that the error uses (1.0 = at the bound): a figure to print, never a check."""
    got = got.detach().double().cpu().reshape(ref.shape)
    ref = ref.detach().double().cpu()
    err = (got - ref).abs()
    m = max(ref.abs().max().item(), 1e-300)
    if dt == F32:
        return max(err.max().item() / (1e-4 * m), err.norm().item() / max(ref.norm().item(), 1e-300) / 2e-5)
    return (err / (2.0 ** -8 * ref.abs() + 1e-3 * m)).max().item()


def _check(got, ref, dt, what=''):
    """_close, after printing how much of the bound the case uses."""
    print(f'{what}: uses {_bound_use(got, ref, dt):.3f} of the {"fp32" if dt == F32 else "bf16"} bound')
    _close(got, ref, dt, what)


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


# ------------------------------------------------------------------------------------------------ fused forward blocks (test_block_kernels.py)
# Restatements of the five fused bf16 kernels in plain torch on the CPU.  Every function takes the evaluation dtype `dt`: float64 is the reference,
# float32 is what the host-only soundness tests compare with it (same rounding points, another accumulation precision).
def _rb(t):
    """Round to bf16 and come back: a point where the kernel stores bf16 by design."""
    return t.to(BF16).to(t.dtype)


def _fold(w, cb, bn, dt=BF16):
    """BN fold of pack_kernel / fold_kernel (conv_igemm.hip) and pw_chain_pack (mlp_chain.hip), restated in fp32 as they compute it:
    s = gamma / sqrtf(eps + var), packed weight = bf16(w * s), bias = beta - gamma * mean / sqrtf(var + eps) (+ s * conv_bias), the bias kept in
    fp32.  Without BN: packed weight = bf16(w), bias = conv_bias (or 0).  dt = F32: the fp32 panel keeps the fp32 product.  Returns (weights, bias) as fp64."""
    w = w.float()
    if bn is None:
        return w.to(dt).double(), (torch.zeros(w.shape[0]) if cb is None else cb.float()).double()
    g, b, mu, var, eps = bn
    e = torch.tensor(eps, dtype=F32)
    s = g / torch.sqrt(e + var)
    bo = b - g * mu / torch.sqrt(var + e)
    if cb is not None:
        bo = bo + s * cb
    return (w * s.view(-1, 1, 1, 1)).to(dt).double(), bo.double()


class ConvP:
    """One convolution of a case: weights (cout, cin, k, k) representable in `wrep` (bf16 by default), fp32 bias or None, BN tuple or None;
    wq / bq = _fold of them for panels of dtype dt."""

    def __init__(self, gen, cout, cin, k, bn=False, bias=True, gain=1.0, dt=BF16, wrep=BF16):
        self.k, self.cin, self.cout, self.dt = k, cin, cout, dt
        self.w = (torch.randn(cout, cin, k, k, generator=gen) * (gain / (cin * k * k) ** 0.5)).to(wrep).float()
        self.cb = (torch.randn(cout, generator=gen) * 0.2).float() if bias else None
        self.bn = None
        if bn:
            u = lambda: torch.rand(cout, generator=gen) + 0.5
            self.bn = (u(), torch.randn(cout, generator=gen) * 0.2, torch.randn(cout, generator=gen) * 0.2, u(), 1e-3)
        self.wq, self.bq = _fold(self.w, self.cb, self.bn, dt)

    def dev_args(self, perm=None):
        """(weight, conv_bias, bn) on the device, the input channels permuted by `perm` when given."""
        w = self.w if perm is None else self.w[:, perm]
        d = lambda t: None if t is None else t.to(DEV)
        bn = None if self.bn is None else tuple(d(t) for t in self.bn[:4]) + (self.bn[4],)
        return d(w.contiguous()), d(self.cb), bn

    def pack(self, perm=None):
        from mgdt_yolo_amd import ops
        w, cb, bn = self.dev_args(perm)
        return ops.PackedConv(w, cb, bn, self.k, self.dt)

    def pack_fp8(self, xq):
        from mgdt_yolo_amd import ops
        w, cb, bn = self.dev_args()
        return ops.PackedConvFp8(w, cb, bn, self.k, xq)

    def __call__(self, x, dt, stride=1):
        import torch.nn.functional as F
        return F.conv2d(x, self.wq.to(dt), self.bq.to(dt), stride, self.k // 2)


def _silu(t):
    return t * torch.sigmoid(t)


def ref_pw_chain3(x, convs, dt=torch.float64):
    """mgdt_pw_chain3_fwd.  x (B, 3 wd, H, W): sp0 = silu(cv0(x0)), sp_i = silu(cv_i(bf16(bf16(sp_{i-1}) + x_i))).  Rounding points read off the
    kernel: each sp_i is rounded to bf16 when stored and the NEXT conv reads that rounded value (`prev` holds (float)(T)acc); the sum
    sp_{i-1} + x_i is formed in fp32 and rounded to bf16 as the MFMA operand.  Returns the three sp_i BEFORE their final rounding."""
    wd = convs[0].cout
    xs = x.to(dt).split(wd, 1)
    out, prev = [], None
    for i in range(3):
        a = xs[i] if prev is None else _rb(prev + xs[i])
        sp = _silu(convs[i](a, dt))
        out.append(sp)
        prev = _rb(sp)
    return torch.cat(out, 1)


def ref_csp_block(mode, x, front, mids, shortcut, back, dt=torch.float64):
    """mgdt_csp_block_fwd (mode 0 = MSPA_C2f, 1 = C2f), every conv = Conv + folded BN + SiLU with zero padding.
      MSPA front: the pw chain above on x0..x2 -> concat slots sp0, sp1, sp2 (bf16); bottleneck input P = bf16(sp2 + x3).
      C2f front : x = [y0 | y1] is copied to the concat, P = y1.
      bottleneck: T = bf16(silu(cv1(P))), P' = bf16(silu(cv2(T)) (+ P with shortcut)); each P' is a concat slot.
      back      : y = silu(cv(concat)), stored as bf16.
    Rounding points (read off the kernel): the concat slots, P and T live in LDS as bf16 (lds_store4); the shortcut adds the bf16 P to the fp32
    SiLU output before the one rounding of P'.  Returns y BEFORE its final rounding."""
    x = x.to(dt)
    wd = mids[0].cout
    if mode == 0:
        sp = _rb(ref_pw_chain3(x[:, :3 * wd], front, dt))
        cat, p = [sp], _rb(sp[:, 2 * wd:] + x[:, 3 * wd:])
    else:
        cat, p = [x], x[:, wd:]
    for j in range(0, len(mids), 2):
        t = _rb(_silu(mids[j](p, dt)))
        q = _silu(mids[j + 1](t, dt))
        p = _rb(q + p if shortcut else q)
        cat.append(p)
    return _silu(back(torch.cat(cat, 1), dt))


def inj_lerp(osz, isz):
    """inj_lerp of inject_fused.hip for every output index, in fp32 without contraction as the kernel states it: src = max(0, (in/out) * (o + 0.5) -
    0.5), i0 = min(int(src), in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0.  Returns (i0, i1, l1) as numpy arrays."""
    import numpy as np
    f = np.float32
    o = np.arange(osz, dtype=f)
    src = np.maximum(f(f(isz) / f(osz)) * (o + f(0.5)) - f(0.5), f(0))
    i0 = np.minimum(src.astype(np.int64), isz - 1)
    return i0, i0 + (i0 < isz - 1), (src - i0.astype(f)).astype(f)


def inj_bilinear(g, H, W):
    """F.interpolate(g, (H, W), bilinear, align_corners=False) in the association the kernel header states:
    (v00 * lx0 + v01 * lx1) * ly0 + (v10 * lx0 + v11 * lx1) * ly1 with lx0 = 1 - lx1 formed in fp32; indices and weights from inj_lerp."""
    import numpy as np
    dt = g.dtype
    y0, y1, wy = inj_lerp(H, g.shape[2])
    x0, x1, wx = inj_lerp(W, g.shape[3])
    y0, y1, x0, x1 = (torch.from_numpy(a) for a in (y0, y1, x0, x1))
    t = lambda a: torch.from_numpy(a).to(dt)
    lx1, lx0 = t(wx), t(np.float32(1) - wx)
    ly1, ly0 = t(wy).view(-1, 1), t(np.float32(1) - wy).view(-1, 1)
    r0, r1 = g[:, :, y0], g[:, :, y1]
    return (r0[..., x0] * lx0 + r0[..., x1] * lx1) * ly0 + (r1[..., x0] * lx0 + r1[..., x1] * lx1) * ly1


def inj_matrix_bf16(H, W, Hg, Wg):
    """The GCONV form's interpolation operand: row = output pixel, column = source pixel, entry = bf16 of the fp32 sum of the tap weights
    w00 = (1 - ly1)(1 - lx1), w01 = (1 - ly1) lx1, w10 = ly1 (1 - lx1), w11 = ly1 lx1 that fall on that source pixel (coinciding taps add up, in
    this order).  (H W, Hg Wg) fp64 of bf16 values."""
    import numpy as np
    f = np.float32
    y0, y1, wy = inj_lerp(H, Hg)
    x0, x1, wx = inj_lerp(W, Wg)
    M = np.zeros((H * W, Hg * Wg), dtype=f)
    rows = np.arange(H * W)
    for ys, xs, wyy, wxx in ((y0, x0, f(1) - wy, f(1) - wx), (y0, x1, f(1) - wy, wx), (y1, x0, wy, f(1) - wx), (y1, x1, wy, wx)):
        s = (ys[:, None] * Wg + xs[None, :]).reshape(-1)
        M[rows, s] = M[rows, s] + (wyy[:, None] * wxx[None, :]).astype(f).reshape(-1)
    return torch.from_numpy(M).to(BF16).double()


def _hsig(t):
    return (t / 6 + 0.5).clamp(0, 1)


def ref_inject(x, pk, ga, gf, dt=torch.float64, pkg=None, gsrc=None):
    """mgdt_conv1x1_inject_fwd and the injection half of mgdt_conv1x1_inject_conv_fwd: loc * bilinear(h_sigmoid(ga)) + bilinear(gf) with
    loc = bf16(conv1x1(x)) (the kernel keeps the rounding the unfused pair had) and h_sigmoid = clamp(v / 6 + 0.5, 0, 1) applied BEFORE the
    interpolation.  With (pkg, gsrc), the GCONV form: ga | gf = bf16(conv1x1(gsrc)) over the merged panel, the gate bf16(h_sigmoid(ga)) rounded
    once more, and the interpolation a matrix product with the bf16 tap weights of inj_matrix_bf16.  Returns the injected map unrounded."""
    B, _, H, W = x.shape
    loc = _rb(pk(x.to(dt), dt))
    if pkg is None:
        return loc * inj_bilinear(_hsig(ga.to(dt)), H, W) + inj_bilinear(gf.to(dt), H, W)
    c = pk.cout
    gaf = _rb(pkg(gsrc.to(dt), dt))
    hg, gff = _rb(_hsig(gaf[:, :c])), gaf[:, c:]
    M = inj_matrix_bf16(H, W, gsrc.shape[2], gsrc.shape[3]).to(dt)
    ip = lambda m: torch.einsum('ps,bcs->bcp', M, m.reshape(B, c, -1)).reshape(B, c, H, W)
    return loc * ip(hg) + ip(gff)


def ref_inject_conv(x, pk, ga, gf, pk2, dt=torch.float64, pkg=None, gsrc=None):
    """mgdt_conv1x1_inject_conv_fwd: silu(conv1x1_2(bf16(injected map))): the injected map is rounded to bf16 where the stored map would be
    (it is the second MFMA's operand).  Returns the output unrounded."""
    return _silu(pk2(_rb(ref_inject(x, pk, ga, gf, dt, pkg, gsrc)), dt))


def ref_detect_map(tb, tc, pkb, pkc, pk3=None, dt=torch.float64):
    """The raw head map of mgdt_detect_tail_fwd: [conv1x1(tb) | conv1x1(tc)] with bias, no activation; with pk3 the box input goes through
    bf16(silu(conv3x3(tb))) first (Conv + BN + SiLU, zero padding; rounded like the stored map it replaces).  Unrounded."""
    t = tb.to(dt)
    if pk3 is not None:
        t = _rb(_silu(pk3(t, dt)))
    return torch.cat([pkb(t, dt), pkc(tc.to(dt), dt)], 1)


def ref_detect_decode(feat, nc, stride, aug=None):
    """y (B, 4 + nc, H W) in fp64 from a raw map: the DFL softmax expectation, dist2bbox and anchors of oracle.layers, x stride, sigmoid scores;
    aug = (s, flip, img_w): xywh / s, then x = img_w - x when flipped."""
    from oracle import layers as OL
    y = OL.detect_decode([feat.double()], [float(stride)], 4, nc)
    if aug is not None:
        y = y.clone()
        y[:, :4] = y[:, :4] / aug[0]
        if aug[1]:
            y[:, 0] = aug[2] - y[:, 0]
    return y


# ------------------------------------------------------------------------------------------------ fused convolution (test_conv_kernels.py)
_ACTS = {'none': lambda t: t, 'silu': _silu, 'relu': torch.relu, 'gelu': lambda t: 0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752))}


def ref_conv2d(x, cp, stride, act, store, x2=None, in_scale=None, in_shift=None, r1=None, r2=None, dt=torch.float64):
    """mgdt_conv2d_fwd:  y = act(conv((x [+ x2]) [* in_scale[n, c] + in_shift[c]]) + bias) [+ r1] [+ r2], zero padding k // 2, cp = ConvP.
    Rounding points read off conv_igemm_kernel (load_chunk): with bf16 views (`store` = BF16) the sum x + x2 is formed in fp32 and rounded to bf16
    (frag_add), and the affine result is rounded to bf16 once more (frag_affine) - it is the MFMA operand; padding pixels stay zero (the affine is
    applied to in-image taps only).  With fp32 views nothing is rounded.  Returns y BEFORE its final rounding."""
    rnd = _rb if store == BF16 else (lambda t: t)
    a = x.to(dt)
    if x2 is not None:
        a = rnd(a + x2.to(dt))
    if in_scale is not None or in_shift is not None:
        if in_scale is not None:
            a = a * in_scale.to(dt)[:, :, None, None]
        if in_shift is not None:
            a = a + in_shift.to(dt)[None, :, None, None]
        a = rnd(a)
    y = _ACTS[act](cp(a, dt, stride))
    for r in (r1, r2):
        if r is not None:
            y = y + r.to(dt)
    return y


def _e4m3(t):
    """OCP e4m3fn quantisation as the gfx950 conversion does it: round to nearest even after clamping to the finite range (+-448)."""
    return t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def ref_conv2d_fp8(x, cp, stride, act, xq, x2=None, r1=None, r2=None):
    """mgdt_conv2d_fp8_fwd as test_conv_fp8_matches_e4m3_emulation states it: BN folded in fp32, per-output-channel weight scale ws = max|w'| / 448,
    panel = e4m3(w' / ws), activations e4m3(bf16(x [+ x2]) * xq) with the product formed in fp32, the exact product sum times ws / xq plus the
    fp32 bias, activation, residuals.  Float64 from the quantised operands on.
    The master weights of an fp8 case are plain fp32 values (ConvP(wrep=F32)), as in that test: w' / ws of bf16-representable weights is a ratio of
    8-bit integers times 448 and lands EXACTLY on e4m3 rounding ties (19/28 * 448 = 304, between 288 and 320) for a few weights of most channels;
    with a BN fold the fp32 values on either side of such a tie are one ulp apart and the device's 1-ulp sqrtf / division decides them the other
    way (measured: 25 of 36 864 panel bytes of a 64 -> 64 3x3 layer one e4m3 step off, output error 1.006 of the bound at one pixel).  Both
    are correct quantisations; generic fp32 weights do not sit on ties."""
    import torch.nn.functional as F
    w = cp.w.float()
    if cp.bn is not None:
        g, _, _, var, eps = cp.bn
        w = w * (g / torch.sqrt(torch.tensor(eps, dtype=F32) + var)).view(-1, 1, 1, 1)
    ws = w.abs().amax(dim=(1, 2, 3)) / 448.0
    wq = _e4m3(w / ws[:, None, None, None])
    a = x.float()
    if x2 is not None:
        a = (a + x2.float()).to(BF16).float()
    acc = F.conv2d(_e4m3(a * xq).double(), wq.double(), None, stride, cp.k // 2) * (ws / xq).double()[None, :, None, None] + cp.bq[None, :, None, None]
    y = _ACTS[act](acc)
    for r in (r1, r2):
        if r is not None:
            y = y + r.double()
    return y


def _check_fp8(got, ref, what=''):
    """The bound of test_conv_fp8_matches_e4m3_emulation: max |got - ref| < 8e-3 * max(1, max|ref|); prints how much of it the case uses."""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), (what, 'non-finite output')
    err = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f'{what}: uses {err / 8e-3:.3f} of the fp8 bound')
    assert err < 8e-3, (what, err)


# ------------------------------------------------------------------------------------------------ detection loss / assigner (test_loss_kernels.py)
def loss_maps(gen, B, R, nc, levels, dt):
    """Raw head maps, one (B, 4R + nc, H, W) CPU fp64 tensor per level (H, W, stride), every value representable in dt.  The DFL logits lean
    towards the far bins (boxes of a few cells), the class logits sit around -2 as after the head's bias initialisation."""
    out = []
    for h, w, _ in levels:
        f = torch.randn(B, 4 * R + nc, h, w, generator=gen) * 1.2
        f[:, :4 * R] += (torch.arange(R, dtype=F32) / max(R - 1, 1) * 2.5 - 1.0).repeat(4).view(1, -1, 1, 1)
        f[:, 4 * R:] -= 2.0
        out.append(f.to(dt).double())
    return out


def loss_gt_random(gen, B, N, nc, width, height, counts, lo=10.0, hi=60.0):
    """(B, N, 5) fp32 [cls, x1, y1, x2, y2] px: counts[b] random boxes in image b (sides lo..hi px, clipped to the image), the other rows zero
    (padding).  The first two boxes drawn carry the labels 0 and nc - 1."""
    gt = torch.zeros(B, N, 5, dtype=F32)
    k = 0
    for b in range(B):
        for j in range(counts[b]):
            cx, cy = (torch.rand(2, generator=gen) * torch.tensor([width, height])).tolist()
            bw, bh = (torch.rand(2, generator=gen) * (hi - lo) + lo).tolist()
            lab = (0, nc - 1)[k] if k < 2 else int(torch.randint(0, nc, (1,), generator=gen))
            gt[b, j] = torch.tensor([lab, max(cx - bw / 2, 0.0), max(cy - bh / 2, 0.0), min(cx + bw / 2, width), min(cy + bh / 2, height)])
            k += 1
    return gt


def loss_reference(maps, gt, strides, R, nc, call_count, want_grad=True):
    """oracle.loss.detection_loss in float64 on the given (already rounded) maps with the dense fp32 targets upcast as they are; the gradient of
    total (= loss * B) by torch.autograd.  Returns a dict: total, items, grads (list, NCHW), fg, gt_idx, tscore (B, A), tss, aux."""
    from oracle import loss as OLoss
    fs = [m.clone().requires_grad_(want_grad) for m in maps]
    assert all(f.dtype == torch.float64 for f in fs)
    total, items, aux = OLoss.detection_loss(fs, None, [float(s) for s in strides], R, nc, call_count=call_count, targets=gt)
    assert total.dtype == torch.float64 and items.dtype == torch.float64 and aux['target_scores'].dtype == torch.float64
    grads = None
    if want_grad:
        total.backward()
        grads = [f.grad for f in fs]
    ts = aux['target_scores'].sum(-1)
    return dict(total=total.detach(), items=items, grads=grads, fg=aux['fg_mask'], gt_idx=aux['target_gt_idx'], tscore=ts,
                tss=torch.as_tensor(max(float(ts.sum()), 1.0), dtype=torch.float64), aux=aux)


def _rows_identical(gt, b, j1, j2):
    return (gt[b, j1] == gt[b, j2]).all(-1)


def _top2_over_gts(aux, gt):
    """For every (image, anchor): the largest and second largest align metric over the GT rows and whether the two rows are identical."""
    align = aux['align']
    B, N, A = align.shape
    if N < 2:
        z = torch.zeros(B, A, dtype=align.dtype)
        return align[:, 0], z - 1, torch.zeros(B, A, dtype=torch.bool), torch.zeros(B, A, dtype=torch.long), torch.zeros(B, A, dtype=torch.long)
    v, j = align.sort(dim=1, descending=True, stable=True)
    bi = torch.arange(B)[:, None].expand(B, A)
    return v[:, 0], v[:, 1], _rows_identical(gt, bi, j[:, 0], j[:, 1]), j[:, 0], j[:, 1]


def loss_margins(ref, gt, R, what=''):
    """The conditions on the INPUTS under which an fp32 evaluation cannot take another decision than the float64 reference (see
    test_loss_kernels.py): asserted on the reference alone, for every GT and anchor of the case."""
    aux = ref['aux']
    align, raw, in_gts, topk, claims = aux['align'], aux['raw_iou'], aux['in_gts'], aux['topk'], aux['claims']
    B, N, A = align.shape
    assert A > 10, 'top-k margins need more than 10 anchors'
    valid = aux['mask_gt'].bool().squeeze(-1)
    # (a) 10th vs 11th largest align of every valid GT
    srt = align.sort(-1, descending=True)[0]
    a10, a11 = srt[..., 9], srt[..., 10]
    ok_a = (((a10 - a11) >= 1e-4 * a10) & (a10 > 0)) | ((a10 == 0) & (a11 == 0))
    assert ok_a[valid].all(), (what, '(a) top-k boundary within 1e-4', ((a10 - a11) / a10.clamp(min=1e-300))[valid & ~ok_a].tolist())
    # (b) best vs second-best align over the GTs at every multiply claimed anchor
    best, second, same, _, _ = _top2_over_gts(aux, gt)
    multi = claims > 1
    ok_b = (((best - second) >= 1e-4 * best) & (best > 0)) | ((best == second) & same)
    assert ok_b[multi].all(), (what, '(b) multi-claim within 1e-4', int((multi & ~ok_b).sum()))
    # (c) the clamp of the CIoU at 0: no in-box member of a top-k sits on it;  (e) nor does its align metric leave the fp32 normal range
    inbox_k = torch.gather(in_gts, 2, topk) & valid[..., None]
    raw_k, al_k = torch.gather(raw, 2, topk), torch.gather(align, 2, topk)
    assert (raw_k[inbox_k].abs() >= 1e-5).all(), (what, '(c) a CIoU within 1e-5 of its clamp')
    assert (al_k[inbox_k & (al_k > 0)] >= 1e-30).all(), (what, '(e) a positive align metric below 1e-30')
    # (d) min / max ties of the CIoU: no predicted coordinate equals its target's
    fg = ref['fg']
    tb = (aux['target_bboxes'] / aux['stride_tensor'])[fg]
    assert (aux['pred_bboxes'][fg] != tb).all(), (what, '(d) a predicted coordinate equals the target coordinate')


def loss_census(ref, gt, R, nc):
    """How many of each decision edge the reference of one case contains (counts; test_loss_kernels.py sums them over its cases)."""
    aux = ref['aux']
    in_gts, claims, fg, gi = aux['in_gts'], aux['claims'], ref['fg'], ref['gt_idx']
    B, N, A = in_gts.shape
    valid = aux['mask_gt'].bool().squeeze(-1)
    best, second, same, j1, j2 = _top2_over_gts(aux, gt)
    multi = claims > 1
    n_in = in_gts.sum(-1)
    lab = torch.gather(gt[..., 0].long(), 1, gi)
    tb = aux['target_bboxes'] / aux['stride_tensor']
    ltrb = torch.cat((aux['anchor_points'] - tb[..., :2], tb[..., 2:] - aux['anchor_points']), -1)
    has = valid.any(1)
    return {'multi_claim_by_margin': int((multi & (best > second)).sum()),
            'gt_with_1_to_9_anchors': int((valid & (n_in >= 1) & (n_in <= 9)).sum()),
            'gt_without_anchor': int((valid & (n_in == 0)).sum()),
            'padded_gt_row': int((~valid).sum()),
            'empty_image_in_labelled_batch': int((~has).sum()) if has.any() else 0,
            'dfl_target_clamped': int((ltrb[fg] > R - 1 - 0.01).sum()),
            'positive_label_0': int((fg & (lab == 0)).sum()),
            'positive_label_last': int((fg & (lab == nc - 1)).sum()),
            'centre_on_gt_edge': int(((aux['deltas_min'] == 0) & valid[..., None]).sum()),
            'duplicate_rows_tie_to_lower': int((multi & fg & (best == second) & same & (gi == torch.minimum(j1, j2))).sum())}


# ------------------------------------------------------------------------------------------------ optimizer (test_loss_kernels.py)
def f32r(x):
    """A Python scalar as the C ABI receives it: rounded to fp32."""
    return float(torch.tensor(x, dtype=F32))


def ref_clip(g, max_norm):
    """mgdt_grad_clip_coef in float64: (norm, min(1, max_norm / (norm + 1e-6)))."""
    norm = g.double().pow(2).sum().sqrt()
    return norm, torch.clamp(f32r(max_norm) / (norm + f32r(1e-6)), max=1.0)


def ref_sgd(p, g, buf, wd, lr, lr_bias, momentum, nesterov, first, coef):
    """mgdt_sgd_step in float64 (trainer.py:462-470 with the flat per-element groups): returns the new (p, buf).  wd[i] > 0 decays, wd[i] < 0
    is the bias group stepping with lr_bias, coef the clip coefficient (1 without)."""
    p, g, buf = p.double(), g.double(), buf.double()
    w = torch.zeros_like(p) if wd is None else wd.double()
    gi = coef * g + torch.where(w > 0, w * p, torch.zeros_like(p))
    b = gi if first else f32r(momentum) * buf + gi
    step = gi + f32r(momentum) * b if nesterov else b
    return p - torch.where(w < 0, torch.full_like(p, f32r(lr_bias)), torch.full_like(p, f32r(lr))) * step, b


def ref_ema(ema, p, d):
    """mgdt_ema_update in float64 (ModelEMA.update, torch_utils.py:342-361), d as the C ABI receives it."""
    return f32r(d) * ema.double() + (1.0 - f32r(d)) * p.double()


# ------------------------------------------------------------------------------------------------ ConvNeXtV2 forward (test_cnx_kernels.py)
# Restatements of mgdt_dwconv7_ln_fwd, mgdt_cnx_mlp_fwd, mgdt_cnx_block_fwd and mgdt_grn_stats_fwd in plain torch on the CPU, stage by stage, so that
# the flip allowance below can re-enter them behind any of their internal bf16 rounding points.  `dt` is the evaluation dtype as above.
def ref_dwconv7_ln(x, dw, dwb, lnw, lnb, eps, dt=torch.float64):
    """mgdt_dwconv7_ln_fwd / _train_fwd: u = depth-wise 7x7 conv (49 taps, zero padding 3) + bias; y = LayerNorm over the channels in the two-pass form
    (mean, then the centred variance; rstd = 1 / sqrt(var + eps), eps as the fp32 the C ABI receives), computed from the UNROUNDED u.  dw (C, 1, 7, 7).
    Returns (y, u) before their store rounding."""
    import torch.nn.functional as F
    c = x.shape[1]
    u = F.conv2d(x.to(dt), dw.to(dt), dwb.to(dt), 1, 3, 1, c)
    d = u - u.mean(1, keepdim=True)
    var = (d * d).mean(1, keepdim=True)
    y = d * (1.0 / torch.sqrt(var + f32r(eps))) * lnw.to(dt).view(1, -1, 1, 1) + lnb.to(dt).view(1, -1, 1, 1)
    return y, u


def _erf_gelu(t):
    return 0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752))


def _pw(t, w, b):
    """Linear over the channels of an NCHW map: w (cout, cin), b (cout)."""
    return torch.einsum('oc,bchw->bohw', w, t) + b.view(1, -1, 1, 1)


def cnx_h_pre(t, w1, b1, dt):
    """gelu(W1 t + b1) with the exact erf GELU (the kernels' polynomial is held to it by a host-only test), before the bf16 rounding of h."""
    return _erf_gelu(_pw(t.to(dt), w1.to(dt), b1.to(dt)))


def ref_grn_scale(t, gamma, dt=torch.float64):
    """mgdt_grn_stats_fwd and the GRN prologue of the fused kernels: Gx = sqrt(sum_hw t^2), scale = gamma * Gx / (mean_c Gx + 1e-6) + 1; (B, C)."""
    gx = torch.sqrt((t.to(dt) ** 2).sum((2, 3)))
    return gamma.to(dt).view(1, -1) * (gx / (gx.mean(1, keepdim=True) + f32r(1e-6))) + 1.0


def cnx_v_pre(h, scale, beta, dt):
    return h.to(dt) * scale.to(dt)[:, :, None, None] + beta.to(dt).view(1, -1, 1, 1)


def ref_cnx_mlp(t, res, w1, b1, w2, b2, gamma, beta, dt=torch.float64, stages=False):
    """mgdt_cnx_mlp_fwd: h = bf16(gelu(W1 t + b1)); Gx over the ROUNDED h; v = bf16(h * scale + beta); y = W2 v + b2 (+ res).  Weights (4C, C) / (C, 4C)
    bf16-representable, biases / gamma / beta fp32.  Returns y before its store rounding; with stages=True also a dict of the values before and after
    the two internal roundings (h_pre, h, scale, v_pre, v)."""
    h_pre = cnx_h_pre(t, w1, b1, dt)
    h = _rb(h_pre)
    scale = ref_grn_scale(h, gamma, dt)
    v_pre = cnx_v_pre(h, scale, beta, dt)
    v = _rb(v_pre)
    y = _pw(v, w2.to(dt), b2.to(dt))
    if res is not None:
        y = y + res.to(dt)
    return (y, dict(h_pre=h_pre, h=h, scale=scale, v_pre=v_pre, v=v)) if stages else y


def ref_cnx_block(x, dw, dwb, lnw, lnb, eps, w1, b1, w2, b2, gamma, beta, dt=torch.float64, stages=False):
    """mgdt_cnx_block_fwd without the closing conv: ref_cnx_mlp(bf16(ref_dwconv7_ln(x).y), x, ...): t is rounded to bf16 where the kernel stores it to
    LDS as pwconv1's operand.  With stages=True the dict also holds t_pre and t."""
    t_pre = ref_dwconv7_ln(x, dw, dwb, lnw, lnb, eps, dt)[0]
    t = _rb(t_pre)
    out = ref_cnx_mlp(t, x, w1, b1, w2, b2, gamma, beta, dt, stages)
    if stages:
        out[1].update(t_pre=t_pre, t=t)
    return out


def ref_cnx_tail(ymap, cp, act, dt=torch.float64):
    """The closing 1x1 conv of mgdt_cnx_block_fwd on the block's bf16 output map: act(conv1x1_folded(ymap)), cp = ConvP (BN folded by _fold)."""
    return _ACTS[act](cp(ymap.to(dt), dt))


def _bf16_other(pre):
    """For fp64 values `pre`: (nearest bf16 value, the bf16 neighbour on the other side of pre, distance of pre from the rounding boundary between the
    two).  Where pre is itself a bf16 value the neighbour is the next one away from zero and the distance half a step."""
    r = pre.to(BF16)
    bits = r.view(torch.int16).to(torch.int32)
    rd = r.double()
    away = ((pre - rd) * torch.where(rd == 0, pre, rd) >= 0)              # the other neighbour has the larger magnitude
    mag = (bits & 0x7fff) + torch.where(away, 1, -1)
    flip_sign = mag < 0                                                  # stepping down from +-0: the smallest value of the other sign
    mag = torch.where(flip_sign, torch.ones_like(mag), mag)
    sign = (bits & 0x8000) ^ torch.where(flip_sign, 0x8000, 0)
    sign = torch.where((rd == 0) & (pre != 0), torch.where(pre < 0, 0x8000, 0) ^ torch.where(flip_sign, 0x8000, 0), sign)
    ob = (sign | mag)
    ob = torch.where(ob >= 0x8000, ob - 0x10000, ob).to(torch.int16)
    other = ob.view(BF16).double()
    return rd, other, ((rd + other) / 2 - pre).abs()


def cnx_deltas(st, w1, b1, gamma, beta, ln=None):
    """delta_s of the flip allowance for one case, from the restatement alone: 4 x the largest |fp32 - fp64| difference of stage s's pre-rounding value
    when both evaluations are fed the same (float64-rounded) upstream values, + 1e-6 at h for the kernels' polynomial GELU.  ln = (x, dw, dwb, lnw, lnb,
    eps) adds the stage t of the whole block.  The device sums in other orders (tap order, MFMA K order, butterflies, per-tile GRN partials) of the
    same lengths and error magnitudes; the factor 4 covers an ordering-dependent constant."""
    d = {}
    if ln is not None:
        d['t'] = 4 * (ref_dwconv7_ln(*ln, dt=F32)[0].double() - st['t_pre']).abs().max().item()
    t = st['t']
    d['h'] = 4 * (cnx_h_pre(t, w1, b1, F32).double() - st['h_pre']).abs().max().item() + 1e-6
    d['v'] = 4 * (cnx_v_pre(st['h'], ref_grn_scale(st['h'], gamma, F32), beta, F32).double() - st['v_pre']).abs().max().item()
    return d


def cnx_allowance(st, deltas, w1, b1, w2, beta):
    """The flip allowance of mgdt_cnx_mlp_fwd / mgdt_cnx_block_fwd, computed from the float64 reference alone (st = the stages of ref_cnx_mlp /
    ref_cnx_block).  An element of an internal rounding point s (t, h, v) is undecided when its pre-rounding value lies within deltas[s] of a bf16
    rounding boundary: a correct fp32 kernel may round it to the other neighbour.  For every undecided element the stages behind it are evaluated
    again with that ONE element moved to its other neighbour, the image's GRN scale frozen and the later stages rounded to nearest as usual; |delta y|
    is added to the allowance of the element's pixel.  Returns (allowance (B, C, H, W), {stage: number of undecided elements})."""
    B, HD, H, W = st['h'].shape
    w2a = w2.double().abs()
    scale = st['scale'][:, :, None, None]
    bt = beta.double().view(1, -1, 1, 1)
    count = {}
    # v: one element of pwconv2's operand moves by one bf16 step
    _, v_o, v_d = _bf16_other(st['v_pre'])
    und = v_d < deltas['v']
    count['v'] = int(und.sum())
    dv = torch.where(und, (v_o - st['v']).abs(), torch.zeros_like(v_o))
    # h: the element's v is formed and rounded again from the moved h
    _, h_o, h_d = _bf16_other(st['h_pre'])
    und = h_d < deltas['h']
    count['h'] = int(und.sum())
    dv = dv + torch.where(und, (_rb(h_o * scale + bt) - st['v']).abs(), torch.zeros_like(h_o))
    allow = torch.einsum('oc,bchw->bohw', w2a, dv)
    # t: the whole hidden column of the pixel is evaluated again
    if 't' in deltas:
        _, t_o, t_d = _bf16_other(st['t_pre'])
        und = t_d < deltas['t']
        count['t'] = int(und.sum())
        idx = und.nonzero()                                               # (n, 4): b, channel, y, x
        w1d, b1d, w2d = w1.double(), b1.double(), w2.double()
        for s0 in range(0, idx.shape[0], 2048):
            b_, k_, y_, x_ = idx[s0:s0 + 2048].unbind(1)
            tp = st['t'][b_, :, y_, x_].clone()                           # (n, C)
            tp[torch.arange(tp.shape[0]), k_] = t_o[b_, k_, y_, x_]
            h2 = _rb(_erf_gelu(tp @ w1d.t() + b1d))
            v2 = _rb(h2 * st['scale'][b_] + beta.double())
            dy = ((v2 - st['v'][b_, :, y_, x_]) @ w2d.t()).abs()          # (n, C)
            allow.permute(0, 2, 3, 1).index_put_((b_, y_, x_), dy, accumulate=True)
    return allow, count


def _bf16_bound(ref):
    return 2.0 ** -8 * ref.abs() + 1e-3 * ref.abs().max().item()


def _close_allow(got, ref, allow, what=''):
    """_close for a bf16 output whose elements may also move by their flip allowance: |got - ref| <= the unchanged bf16 bound + allowance.  Prints the
    largest share of that bound used, and of the plain bound where the allowance is below a tenth of it."""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), (what, 'non-finite output')
    err, bound = (got - ref).abs(), _bf16_bound(ref)
    use = (err / (bound + allow)).max().item()
    quiet = allow < 0.1 * bound
    plain = (err / bound)[quiet].max().item() if quiet.any() else 0.0
    print(f'{what}: uses {use:.3f} of bound + allowance, {plain:.3f} of the plain bf16 bound where the allowance is below a tenth of it '
          f'({100.0 * quiet.float().mean().item():.1f} % of the elements)')
    assert use <= 1.0, (what, 'worst share of bound + allowance', use, 'elements over', int((err > bound + allow).sum()))
    return use, plain


# ------------------------------------------------------------------------------------------------ stem and direct convolution (test_stem_direct_kernels.py)
def u8_unit(v):
    """A uint8 image as the kernels read it: fp32(v) / fp32(255), one correctly rounded fp32 division (the `lut` entry); fp64 values."""
    return (v.to(F32) / torch.tensor(255.0, dtype=F32)).double()


def ref_stem2(img, cp0, cp1, dt=torch.float64, stages=False):
    """mgdt_stem2_fwd.  img: the image values as stored (fp64; a uint8 image as u8_unit gives it).  Rounding points read off stem2_kernel: the patch is
    staged in LDS as bf16 (X = bf16(value): the 16-byte loader copies bf16, the element-wise one rounds fp32 and lut values when it writes them);
    layer 0 = ConvP(16, 3, 3, BN, no conv bias) folded as PackedStem2 + stem2_pack_kernel do (bf16(w * s), s = gamma / sqrtf(eps + var) in fp32, fp32
    bias: exactly _fold), y0 = bf16(silu(conv stride 2)) stored to LDS, zero outside the H0 x W0 map (layer 1's padding); layer 1 = the mgdt_conv_pack
    bf16 panel, y = silu(conv stride 2 + bias).  Returns y BEFORE its final rounding; with stages=True also {y0_pre, y0}
    (the values before and after the mid-kernel rounding)."""
    x = _rb(img.to(dt))
    y0_pre = _silu(cp0(x, dt, 2))
    y0 = _rb(y0_pre)
    y = _silu(cp1(y0, dt, 2))
    return (y, dict(y0_pre=y0_pre, y0=y0)) if stages else y


def ref_direct(x, cp, stride, act, groups=1, dt=torch.float64):
    """mgdt_conv2d_direct_fwd: act(conv(x, w * s, groups) + bias), zero padding k // 2.  cp = ConvP(cout, cin / groups, k, dt=F32): the direct packer keeps
    the fp32 product w * s and the fp32 bias (_fold(..., dt=F32)); the input is read as stored (a uint8 image as u8_unit gives it, NOT rounded to bf16),
    products and sums are fp32 FMAs, one rounding at the store.  Returns y BEFORE that rounding."""
    import torch.nn.functional as F
    return _ACTS[act](F.conv2d(x.to(dt), cp.wq.to(dt), cp.bq.to(dt), stride, cp.k // 2, 1, groups))


def ref_pack_direct(cp):
    """mgdt_conv_pack_direct in float64 from the unfolded parameters: panel[(tap * cin_g + ci) * cout + co] = w[co][ci][ky][kx] * gamma / sqrt(eps + var),
    bias = beta - gamma * mean / sqrt(var + eps) (+ s * conv_bias); without BN the weights and the conv bias (or 0).  eps as the fp32 the C ABI receives."""
    w = cp.w.double()
    cb = None if cp.cb is None else cp.cb.double()
    if cp.bn is None:
        bias = torch.zeros(cp.cout, dtype=torch.float64) if cb is None else cb
    else:
        g, b, mu, var, eps = (t.double() if torch.is_tensor(t) else f32r(t) for t in cp.bn)
        s = g / torch.sqrt(eps + var)
        w = w * s.view(-1, 1, 1, 1)
        bias = b - g * mu / torch.sqrt(var + eps) + (0 if cb is None else s * cb)
    return w.permute(2, 3, 1, 0).reshape(-1), bias


# ------------------------------------------------------------------------------------------------ conditioning ladder (test_conditioning.py)
# Inputs whose normalisation sets have |mean| / std = R, and the bound that comes from the reference alone: the distance of the same torch functional
# run in float32 on the CPU to its float64 run (the rule of tests/test_train_modules.py and tests/test_rtdetr.py:fp32_bound).
def ladder_map(key, shape, R, dt, std=1.0):
    """(B, C, H, W) fp64 values representable in dt, N(R * std, std) with ONE mean and ONE std for the whole map, so that every channel, every
    (image, group) and every pixel has |mean| / std = R (negative R: a negative mean).  R = 'const': the near-constant rung, mean 1 and std 2^-10
    (variance below every eps in use: the clamp at zero and eps are what is exercised).  Every rung of a case shifts and scales the same draw."""
    gen = _gen('ladder', *key, shape)                      # the same N(0, 1) draw on every rung and in both dtypes
    if R == 'const':
        return _q(torch.randn(*shape, generator=gen, dtype=torch.float64) * 2.0 ** -10 + 1.0, dt)
    return _q(torch.randn(*shape, generator=gen, dtype=torch.float64) * std + R * std, dt)


def cond_bounds(r64, r32):
    """(relative L2 bound, largest-element bound) of an fp32 output: max(2e-5, 8 x d32) and max(1e-4 x max|ref|, 8 x d32_max), d32 / d32_max the
    relative L2 / largest-element distance of the float32 CPU run r32 to the float64 run r64.  With d32 = 0 this is _close's fp32 bound."""
    r64, r32 = r64.detach().double(), r32.detach().double().reshape(r64.shape)
    d = (r32 - r64).abs()
    return max(2e-5, 8 * d.norm().item() / max(r64.norm().item(), 1e-300)), max(1e-4 * r64.abs().max().item(), 8 * d.max().item())


def cond_use(got, r64, r32):
    """Largest fraction of cond_bounds that got uses (1.0 = at the bound)."""
    got, r64 = got.detach().double().cpu().reshape(r64.shape), r64.detach().double()
    rel_b, max_b = cond_bounds(r64, r32)
    err = (got - r64).abs()
    return max(err.norm().item() / max(r64.norm().item(), 1e-300) / rel_b, err.max().item() / max(max_b, 1e-300))


def cond_check(got, r64, r32, dt, what=''):
    """fp32 outputs (dt = F32; every fp32 statistic and parameter gradient of a bf16 run included): within cond_bounds.  bf16 outputs: _close's bf16
    bound unchanged.  Prints the fraction of the bound used first."""
    if dt != F32:
        return _check(got, r64, dt, what)
    g = got.detach().double().cpu().reshape(r64.shape)
    assert torch.isfinite(g).all(), (what, 'non-finite output')
    use = cond_use(g, r64, r32)
    rel_b, max_b = cond_bounds(r64, r32)
    print(f'{what}: uses {use:.3f} of the fp32 ladder bound (rel L2 <= {rel_b:.2e}, max <= {max_b:.2e})')
    assert use <= 1.0 or (g == r64.double()).all(), (what, 'share of the bound', use, 'rel L2 bound', rel_b, 'max bound', max_b)
