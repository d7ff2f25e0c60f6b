"""Every reverse-pass entry point of ops.* against torch autograd in float64 on the CPU, per route.  Needs a real MI355X (-m gpu).

Each case feeds the kernel and the reference the SAME values (rounded to the kernel's dtype first) and forces one route of the C dispatch
by shape or alignment alone; its id names the route.  Misaligned routes use a channel slice at offset 2 (fp32) or 4 (bf16: the MFMA rule is
16-byte alignment) inside a wider NHWC buffer, channel counts that are not multiples of 4, or maps / channel counts above a vector kernel's limit.

Tolerances come from the arithmetic: the kernels accumulate in fp32 and round their output once.
  fp32 outputs (every fp32 parameter gradient of a bf16 run included): relative L2 error <= 2e-5 and every element within 1e-4 * max|ref|.
  bf16 outputs: every element within 2^-8 * |ref| + 1e-3 * max|ref|.
  Integer-exact operations (the max-pool scatter on quantised inputs, nearest, power-of-two average-pool bins in fp32) are compared exactly.
Where a kernel stores an intermediate in the compute dtype by design, the reference rounds that intermediate too (stated at the case).
"""
import pytest
import torch
import torch.nn.functional as F

from kernel_ref import BF16, DEV, F32, _borders_untouched, _close, _exact, _gen, _nhwc, _out_buf, _q, _rand
from mgdt_yolo_amd import ops

pytestmark = pytest.mark.gpu
DTS = [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')]
ACTS = {'silu': (ops.ACT_SILU, F.silu), 'relu': (ops.ACT_RELU, F.relu), 'gelu': (ops.ACT_GELU, F.gelu), 'none': (ops.ACT_NONE, lambda t: t)}


# ------------------------------------------------------------------------------------------------ BatchNorm (+ act) backward
def _ref_bn_act(y, gz, gamma, beta, eps, act):
    yr, ga, be = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = ACTS[act][1](F.batch_norm(yr, None, None, ga, be, True, 0.0, eps))
    z.backward(gz)
    mean = y.mean((0, 2, 3))
    rstd = 1.0 / torch.sqrt(y.var((0, 2, 3), unbiased=False) + eps)
    return yr.grad, ga.grad, be.grad, mean, rstd


# (B, C, H, W, act, off): off = channel offset of the views inside a wider buffer
BN_CASES = [
    pytest.param(2, 16, 10, 12, 'silu', 0, id='bnf_v4-c16-silu'),
    pytest.param(3, 32, 7, 5, 'relu', 0, id='bnf_v4-c32-odd-relu'),
    pytest.param(2, 24, 9, 7, 'gelu', 0, id='bnf_v4-c24-gelu'),
    pytest.param(2, 8, 1, 1, 'silu', 0, id='bnf_v4-1x1-B2'),
    pytest.param(64, 4, 2, 3, 'none', 0, id='bnf_v4-many-images-2x3'),
    pytest.param(2, 4, 64, 64, 'silu', 0, id='bnf_v4-npix8192-64splits'),
    pytest.param(2, 4, 64, 65, 'silu', 0, id='bnf_v4-npix8320-80splits'),
    pytest.param(4, 4, 128, 128, 'relu', 0, id='bnf_v4-npix65536-512splits'),
    pytest.param(1, 4, 256, 257, 'silu', 0, id='bnf_v4-npix65792-capped'),
    pytest.param(2, 1024, 3, 3, 'silu', 0, id='bnf_v4-c1024'),
    pytest.param(2, 1028, 3, 3, 'silu', 0, id='scalar-c1028'),
    pytest.param(2, 6, 9, 11, 'silu', 0, id='scalar-c6'),
    pytest.param(3, 13, 5, 4, 'gelu', 0, id='scalar-c13-gelu'),
    pytest.param(2, 16, 10, 12, 'silu', 2, id='scalar-slice'),
    pytest.param(2, 8, 1, 1, 'relu', 2, id='scalar-1x1-slice'),
    pytest.param(2, 4, 64, 65, 'none', 2, id='scalar-npix8320-slice'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W,act,off', BN_CASES)
def test_bn_act_backward(B, C, H, W, act, off, dt):
    """bn_stats -> bn_act_bwd (Conv.backward's sequence): dy, dgamma, dbeta against autograd of act(batch_norm(y, training=True))."""
    gen = _gen('bn', B, C, H, W, act, off)
    y = _rand(gen, B, C, H, W, dt=dt, scale=1.5, shift=0.5)
    gz = _rand(gen, B, C, H, W, dt=dt)
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = (torch.randn(C, generator=gen, dtype=torch.float64) * 0.3).float().double()
    eps = 1e-3
    dy_ref, dg_ref, db_ref, m_ref, r_ref = _ref_bn_act(y, gz, gamma, beta, eps, act)
    yd, _ = _nhwc(y, dt, off, 8, gen=gen)
    gzd, _ = _nhwc(gz, dt, off, 8, gen=gen)
    mean, rstd = ops.bn_stats(yd, eps, 0.0)
    _close(mean, m_ref, F32, 'mean')
    _close(rstd, r_ref, F32, 'rstd')
    dgamma = torch.full((C,), float('nan'), device=DEV)
    dbeta = torch.full((C,), float('nan'), device=DEV)
    dy = ops.bn_act_bwd(gzd, yd, mean, rstd, gamma.float().to(DEV), beta.float().to(DEV), ACTS[act][0], dgamma, dbeta)
    assert dy.dtype == dt
    _close(dy, dy_ref, dt, 'dy')
    _close(dgamma, dg_ref, F32, 'dgamma')
    _close(dbeta, db_ref, F32, 'dbeta')


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W,off', [pytest.param(2, 64, 6, 5, 0, id='bnf_v4'), pytest.param(2, 64, 6, 5, 2, id='scalar-slice'),
                                         pytest.param(2, 10, 3, 7, 0, id='scalar-c10')])
def test_bias_gelu_backward_no_bn_mode(B, C, H, W, off, dt):
    """The no-BN mode of bn_act_bwd (mean = None, beta = the bias) that ConvNeXt's pwconv1 uses (convnextv2.py: gelu(y + b)): dy and dbias."""
    gen = _gen('bias', B, C, H, W, off)
    y = _rand(gen, B, C, H, W, dt=dt)
    gz = _rand(gen, B, C, H, W, dt=dt)
    b = torch.randn(C, generator=gen, dtype=torch.float64).float().double()
    yr, br = y.clone().requires_grad_(True), b.clone().requires_grad_(True)
    F.gelu(yr + br[None, :, None, None]).backward(gz)
    yd, _ = _nhwc(y, dt, off, 8, gen=gen)
    gzd, _ = _nhwc(gz, dt, off, 8, gen=gen)
    db = torch.full((C,), float('nan'), device=DEV)
    dy = ops.bn_act_bwd(gzd, yd, None, None, None, b.float().to(DEV), ops.ACT_GELU, None, db)
    _close(dy, yr.grad, dt, 'dy')
    _close(db, br.grad, F32, 'dbias')


# ------------------------------------------------------------------------------------------------ MaxPool2d(5, 1, 2) backward
def _ref_maxpool5(x, gy):
    xr = x.clone().contiguous().requires_grad_(True)
    F.max_pool2d(xr, 5, 1, 2).backward(gy)
    return xr.grad


# (B, C, H, W, off, kind); v4 keeps CB = 16 up to 16x16, 8 up to 24x24, 4 up to 36x36 and refuses larger maps
MP_CASES = [
    pytest.param(2, 16, 12, 10, 0, 'rand', id='v4_cb16-c16'),
    pytest.param(2, 20, 9, 7, 0, 'quant', id='v4_cb16-c20-partial-block-ties'),
    pytest.param(1, 12, 1, 1, 0, 'quant', id='v4_cb16-1x1'),
    pytest.param(3, 4, 2, 3, 0, 'quant', id='v4_cb16-2x3'),
    pytest.param(2, 12, 20, 22, 0, 'quant', id='v4_cb8-c12-ties'),
    pytest.param(1, 28, 36, 36, 0, 'pool', id='v4_cb4-36x36-pool-of-pool'),
    pytest.param(2, 8, 10, 10, 0, 'nan', id='v4_cb16-nan'),
    pytest.param(48, 4, 3, 2, 0, 'quant', id='v4-many-images'),
    pytest.param(2, 16, 12, 10, 2, 'rand', id='scalar-slice'),
    pytest.param(2, 6, 9, 7, 0, 'quant', id='scalar-c6-ties'),
    pytest.param(1, 8, 40, 40, 0, 'pool', id='scalar-40x40-pool-of-pool'),
    pytest.param(1, 4, 41, 37, 0, 'quant', id='scalar-41x37-ties'),
    pytest.param(2, 8, 10, 10, 2, 'nan', id='scalar-nan-slice'),
    pytest.param(1, 5, 1, 1, 0, 'quant', id='scalar-1x1-c5'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W,off,kind', MP_CASES)
def test_maxpool5_backward(B, C, H, W, off, kind, dt):
    """maxpool5_bwd against autograd of F.max_pool2d(5, 1, 2): the gradient goes to the FIRST maximum of each window in ATen's (ky, kx) scan, a NaN
    replaces what was found before it.  gy holds small integers, so every gathered sum is exact in fp32 and bf16 and the comparison is exact.
    'quant': inputs on 3 levels (ties everywhere); 'pool': the input is itself a max-pool output (SPPF's second and third pools: plateaus)."""
    gen = _gen('mp', B, C, H, W, off, kind)
    if kind == 'rand':
        x = _rand(gen, B, C, H, W, dt=dt)
    elif kind == 'pool':
        x = F.max_pool2d(torch.randint(0, 4, (B, C, H, W), generator=gen).double(), 5, 1, 2)
    else:
        x = torch.randint(0, 3, (B, C, H, W), generator=gen).double()
    if kind == 'nan':
        x[0, 1, 4, 5] = float('nan')
        x[-1, C - 1, 0, 0] = float('nan')
    gy = torch.randint(-4, 5, (B, C, H, W), generator=gen).double()
    ref = _ref_maxpool5(x, gy)
    xd, _ = _nhwc(x, dt, off, 8, gen=gen)
    gyd, _ = _nhwc(gy, dt, off, 8, gen=gen)
    gx = ops.maxpool5_bwd(xd, gyd)
    assert gx.dtype == dt
    _exact(gx, ref, 'gx')


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W', [pytest.param(2, 16, 12, 10, id='cb16'), pytest.param(1, 8, 30, 26, id='cb4'), pytest.param(2, 12, 1, 1, id='1x1')])
def test_maxpool5_backward_vector_and_scalar_forms_give_the_same_bits(B, C, H, W, dt):
    """train_vec.hip: v4_maxpool5_bwd_kernel and maxpool5_bwd_kernel add the same terms in the same (oy, ox) order.  Random (untied) data and random gy."""
    gen = _gen('mpeq', B, C, H, W)
    x, gy = _rand(gen, B, C, H, W, dt=dt), _rand(gen, B, C, H, W, dt=dt)
    a = ops.maxpool5_bwd(_nhwc(x, dt)[0], _nhwc(gy, dt)[0])
    b = ops.maxpool5_bwd(_nhwc(x, dt, 2, 8, gen=gen)[0], _nhwc(gy, dt, 2, 8, gen=gen)[0])
    assert torch.equal(a, b)
    _close(a, _ref_maxpool5(x, gy), dt, 'gx')


# ------------------------------------------------------------------------------------------------ resampler adjoints
def _ref_resample(x_shape, gy, fn, base=None):
    xr = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    fn(xr).backward(gy)
    return xr.grad if base is None else xr.grad + base


def _resample_case(op, fn, B, C, h, w, oh, ow, off, acc, dt, exact, tag):
    gen = _gen(tag, B, C, h, w, oh, ow, off, acc, str(dt))
    if exact:
        gy = torch.randint(-8, 9, (B, C, oh, ow), generator=gen).double()
        base = torch.randint(-8, 9, (B, C, h, w), generator=gen).double() if acc else None
    else:
        gy = _rand(gen, B, C, oh, ow, dt=dt)
        base = _rand(gen, B, C, h, w, dt=dt) if acc else None
    ref = _ref_resample((B, C, h, w), gy, fn, base)
    gyd, _ = _nhwc(gy, dt, off, 8, gen=gen)
    gx, big, big0 = _out_buf(B, C, h, w, dt, off, 8, gen)
    if acc:
        gx.copy_(base.to(dt).to(DEV))
        big0 = big.cpu()
    op(gyd, gx, **({'accumulate': True} if acc else {}))
    _borders_untouched(big, big0, off, C)
    return gx, ref


# (B, C, h, w, oh, ow, off, accumulate)
NEAREST_CASES = [
    pytest.param(2, 8, 5, 6, 10, 12, 0, id='scalar-2x'), pytest.param(1, 6, 3, 5, 12, 20, 2, id='scalar-4x-slice-c6'),
    pytest.param(3, 4, 5, 4, 13, 11, 0, id='scalar-non-integer'), pytest.param(1, 4, 1, 1, 2, 3, 0, id='scalar-1x1'),
    pytest.param(32, 4, 2, 3, 4, 6, 2, id='scalar-many-images'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,h,w,oh,ow,off', NEAREST_CASES)
def test_nearest_backward(B, C, h, w, oh, ow, off, dt):
    """nearest_bwd (one kernel: there is no vector twin) against autograd of F.interpolate(mode='nearest'); integer gy -> exact; dx into a slice."""
    gx, ref = _resample_case(lambda g, x: ops.nearest_bwd(g, x), lambda t: F.interpolate(t, size=(oh, ow), mode='nearest'),
                             B, C, h, w, oh, ow, off, False, dt, True, 'near')
    _exact(gx, ref, 'gx')


# (B, C, h, w, oh, ow, off, accumulate): avg-pool bins h -> oh; power-of-two bin sizes are exact in fp32
AVG_CASES = [
    pytest.param(2, 8, 8, 8, 4, 4, 0, False, id='v4_int-2x2bins'), pytest.param(2, 8, 16, 8, 4, 2, 0, True, id='v4_int-4x4bins-acc'),
    pytest.param(2, 8, 13, 7, 5, 3, 0, False, id='v4_generic-13to5-7to3'), pytest.param(1, 12, 7, 13, 3, 5, 0, True, id='v4_generic-acc'),
    pytest.param(2, 8, 9, 6, 3, 2, 0, False, id='v4_int-3x3bins'), pytest.param(48, 4, 3, 2, 1, 1, 0, True, id='v4_int-many-images-acc'),
    pytest.param(2, 8, 8, 8, 4, 4, 2, False, id='scalar_int-slice'), pytest.param(2, 8, 16, 8, 4, 2, 2, True, id='scalar_int-slice-acc'),
    pytest.param(2, 6, 13, 7, 5, 3, 0, False, id='scalar_generic-c6'), pytest.param(1, 12, 7, 13, 3, 5, 2, True, id='scalar_generic-slice-acc'),
    pytest.param(1, 4, 1, 1, 1, 1, 2, False, id='scalar-1x1'), pytest.param(1, 4, 2, 3, 2, 3, 0, False, id='v4-identity-2x3'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,h,w,oh,ow,off,acc', AVG_CASES)
def test_adaptive_avgpool_backward(B, C, h, w, oh, ow, off, acc, dt):
    """adaptive_avgpool_bwd against autograd of F.adaptive_avg_pool2d, incl. non-divisible (overlapping) bins and accumulate into random values."""
    pow2 = (h % oh == 0 and w % ow == 0 and ((h // oh) * (w // ow)) & ((h // oh) * (w // ow) - 1) == 0)
    exact = dt == F32 and pow2
    gx, ref = _resample_case(lambda g, x, **k: ops.adaptive_avgpool_bwd(g, x, **k), lambda t: F.adaptive_avg_pool2d(t, (oh, ow)),
                             B, C, h, w, oh, ow, off, acc, dt, exact, 'avg')
    (_exact(gx, ref, 'gx') if exact else _close(gx, ref, dt, 'gx'))


BIL_CASES = [
    pytest.param(2, 8, 10, 12, 20, 24, 0, False, id='v4_2x-stencil'), pytest.param(2, 8, 10, 12, 20, 24, 0, True, id='v4_2x-stencil-acc'),
    pytest.param(2, 8, 10, 12, 23, 17, 0, True, id='v4_generic-acc'), pytest.param(1, 4, 1, 1, 2, 2, 0, False, id='v4_2x-1x1'),
    pytest.param(1, 4, 2, 3, 4, 6, 0, False, id='v4_2x-2x3-edges-only'), pytest.param(2, 8, 12, 10, 5, 7, 0, False, id='v4_generic-downsample'),
    pytest.param(2, 8, 10, 12, 20, 24, 2, True, id='scalar-2x-slice-acc'), pytest.param(2, 6, 10, 12, 23, 17, 0, False, id='scalar-c6'),
    pytest.param(40, 4, 2, 3, 4, 6, 2, False, id='scalar-many-images'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,h,w,oh,ow,off,acc', BIL_CASES)
def test_bilinear_backward(B, C, h, w, oh, ow, off, acc, dt):
    """bilinear_bwd against autograd of F.interpolate(mode='bilinear', align_corners=False)."""
    gx, ref = _resample_case(lambda g, x, **k: ops.bilinear_bwd(g, x, **k),
                             lambda t: F.interpolate(t, size=(oh, ow), mode='bilinear', align_corners=False), B, C, h, w, oh, ow, off, acc, dt, False, 'bil')
    _close(gx, ref, dt, 'gx')


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('which,h,w,oh,ow', [('avg', 8, 8, 4, 4), ('avg', 13, 7, 5, 3), ('bil', 10, 12, 20, 24), ('bil', 10, 12, 23, 17)])
def test_resampler_adjoints_vector_and_scalar_forms_give_the_same_bits(which, h, w, oh, ow, dt):
    """train_vec.hip: mgdt_v4_avgpool_bwd / mgdt_v4_bilinear_bwd repeat their scalar twins' arithmetic in the same order (with accumulate)."""
    gen = _gen('rseq', which, h, w, oh, ow)
    B, C = 2, 8
    gy, base = _rand(gen, B, C, oh, ow, dt=dt), _rand(gen, B, C, h, w, dt=dt)
    op = ops.adaptive_avgpool_bwd if which == 'avg' else ops.bilinear_bwd
    outs = []
    for off in (0, 2):
        gx, _ = _nhwc(base, dt, off, 8, gen=gen)
        op(_nhwc(gy, dt, off, 8, gen=gen)[0], gx, accumulate=True)
        outs.append(gx.cpu())
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ GRN backward (ConvNeXt) + nc_reduce
def _ref_grn(t, gamma, beta, g):
    tr, ga, be = t.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    gx = torch.norm(tr, p=2, dim=(2, 3), keepdim=True)                 # NCHW form of utils.GRN (oracle/layers.convnext_block)
    nx = gx / (gx.mean(dim=1, keepdim=True) + 1e-6)
    out = ga[None, :, None, None] * (tr * nx) + be[None, :, None, None] + tr
    out.backward(g)
    return tr.grad, ga.grad, be.grad


GRN_CASES = [
    pytest.param(2, 64, 7, 5, 0, id='v4'), pytest.param(3, 128, 4, 4, 0, id='v4-c128'), pytest.param(1, 16, 1, 1, 0, id='v4-1x1-B1'),
    pytest.param(40, 8, 2, 3, 0, id='v4-many-images'), pytest.param(2, 64, 7, 5, 2, id='scalar-slice'), pytest.param(2, 12, 3, 9, 4, id='v4-slice4'),
    pytest.param(2, 14, 6, 5, 0, id='scalar-c14'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W,off', GRN_CASES)
def test_grn_backward_and_nc_reduce(B, C, H, W, off, dt):
    """convnextv2.py's sequence: S = nc_reduce(t, t) (forward), A = nc_reduce(g, t), B = nc_reduce(g), grn_bwd -> dt, dgamma, dbeta."""
    gen = _gen('grn', B, C, H, W, off)
    t = _rand(gen, B, C, H, W, dt=dt, scale=0.7, shift=0.2)
    g = _rand(gen, B, C, H, W, dt=dt)
    gamma = torch.randn(C, generator=gen, dtype=torch.float64).float().double()
    beta = torch.randn(C, generator=gen, dtype=torch.float64).float().double()
    dt_ref, dg_ref, db_ref = _ref_grn(t, gamma, beta, g)
    td, _ = _nhwc(t, dt, off, 8, gen=gen)
    gd, _ = _nhwc(g, dt, off, 8, gen=gen)
    S, A, Bs = ops.nc_reduce(td, td), ops.nc_reduce(gd, td), ops.nc_reduce(gd)
    _close(S, (t * t).sum((2, 3)), F32, 'S')
    _close(A, (g * t).sum((2, 3)), F32, 'A')
    _close(Bs, g.sum((2, 3)), F32, 'B')
    dgamma = torch.full((C,), float('nan'), device=DEV)
    dbeta = torch.full((C,), float('nan'), device=DEV)
    dtt = ops.grn_bwd(gd, td, S, A, Bs, gamma.float().to(DEV), dgamma, dbeta)
    _close(dtt, dt_ref, dt, 'dt')
    _close(dgamma, dg_ref, F32, 'dgamma')
    _close(dbeta, db_ref, F32, 'dbeta')
    # the same S / A / B through the other route of the apply pass: mgdt_v4_grn_bwd_apply and grn_bwd_apply_kernel give the same bits
    other = 2 if off == 0 else 0
    if C % 4 == 0:
        td2, gd2 = _nhwc(t, dt, other, 8, gen=gen)[0], _nhwc(g, dt, other, 8, gen=gen)[0]
        dt2 = ops.grn_bwd(gd2, td2, S, A, Bs, gamma.float().to(DEV), torch.empty_like(dgamma), torch.empty_like(dbeta))
        assert torch.equal(dtt.cpu(), dt2.cpu())


# ------------------------------------------------------------------------------------------------ SPR attention backward (MSPA_C2f)
def _ref_spr_block(out, sd, groups, gy):
    """y = out * softmax over groups of SPR(group) (oracle/layers.mspa_c2f's attention), autograd w.r.t. out and the four SPR parameters."""
    from oracle import layers as OL
    o = out.clone().requires_grad_(True)
    prm = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    b, c = o.shape[:2]
    cw = c // groups
    attn = torch.cat([OL.spr(t, prm, 'a') for t in o.chunk(groups, 1)], 1)
    attn = torch.softmax(attn.view(b, groups, cw, 1, 1), 1)
    y = (o.view(b, groups, cw, *o.shape[2:]) * attn).reshape(o.shape)
    y.backward(gy)
    return o.grad, torch.cat([prm[k].grad.reshape(-1) for k in ('a.fc1.weight', 'a.fc1.bias', 'a.fc2.weight', 'a.fc2.bias')])


SPR_CASES = [
    pytest.param(2, 4, 8, 9, 7, 0, id='v4-odd-map'), pytest.param(2, 4, 4, 6, 6, 0, id='v4-cw4'), pytest.param(1, 2, 12, 1, 1, 0, id='v4-1x1'),
    pytest.param(1, 4, 8, 2, 3, 0, id='v4-2x3'), pytest.param(24, 4, 4, 3, 2, 0, id='v4-many-images'),
    pytest.param(2, 4, 8, 9, 7, 2, id='scalar-slice'), pytest.param(1, 2, 12, 5, 3, 2, id='scalar-slice-odd'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,groups,cw,H,W,off', SPR_CASES)
def test_spr_backward(B, groups, cw, H, W, off, dt):
    """MSPA_C2f's sequence: spr_attention_train (forward), dattn = nc_reduce(g, out), spr_bwd -> d out and [dW1 | db1 | dW2 | db2].  The forward's
    pooling kernel takes 4-aligned views only, so the scalar routes (nc_reduce, spr_out_bwd_kernel) are forced by a misaligned gy."""
    gen = _gen('spr', B, groups, cw, H, W, off)
    C, hid = groups * cw, cw // 4
    out = _rand(gen, B, C, H, W, dt=dt)
    gy = _rand(gen, B, C, H, W, dt=dt)
    sd = {'a.fc1.weight': torch.randn(hid, 5 * cw, 1, 1, generator=gen, dtype=torch.float64).float().double() * 0.4,
          'a.fc1.bias': torch.randn(hid, generator=gen, dtype=torch.float64).float().double() * 0.2,
          'a.fc2.weight': torch.randn(cw, hid, 1, 1, generator=gen, dtype=torch.float64).float().double() * 0.5,
          'a.fc2.bias': torch.randn(cw, generator=gen, dtype=torch.float64).float().double() * 0.2}
    gx_ref, pg_ref = _ref_spr_block(out, sd, groups, gy)
    w = [sd[k].float().to(DEV).contiguous() for k in ('a.fc1.weight', 'a.fc1.bias', 'a.fc2.weight', 'a.fc2.bias')]
    od, _ = _nhwc(out, dt)
    gyd, _ = _nhwc(gy, dt, off, 8, gen=gen)
    attn, part = ops.spr_attention_train(od, *w, groups)
    dattn = ops.nc_reduce(gyd, od)
    gx, pg = ops.spr_bwd(gyd, part, attn, dattn, *w, groups)
    _close(gx, gx_ref, dt, 'gx')
    _close(pg, pg_ref, F32, 'param grads')
    # the same attention, pooled sums and dattn through the other route of the output pass (mgdt_v4_spr_out_bwd vs spr_out_bwd_kernel): same bits
    other = 2 if off == 0 else 0
    gx2, _ = ops.spr_bwd(_nhwc(gy, dt, other, 8, gen=gen)[0], part, attn, dattn, *w, groups)
    assert torch.equal(gx.cpu(), gx2.cpu())


# ------------------------------------------------------------------------------------------------ dw7x7 + LayerNorm backward (ConvNeXt)
# vec kernels when C <= 128 and every view is 4-aligned (NQ = cdiv(C/4, 8) in 1..4); the scalar ln_bwd_kernel / dwconv7_* kernels otherwise
DW7_CASES = [
    pytest.param(2, 8, 7, 5, 0, id='vec_nq1-c8'), pytest.param(1, 4, 1, 1, 0, id='vec_nq1-c4-1x1'), pytest.param(2, 48, 6, 9, 0, id='vec_nq2-c48'),
    pytest.param(2, 96, 5, 4, 0, id='vec_nq3-c96'), pytest.param(1, 128, 2, 3, 0, id='vec_nq4-c128-2x3'), pytest.param(40, 32, 2, 2, 0, id='vec-many-images'),
    pytest.param(2, 136, 5, 4, 0, id='scalar-c136'), pytest.param(2, 32, 7, 5, 2, id='scalar-slice'), pytest.param(1, 8, 1, 1, 2, id='scalar-1x1-slice'),
    pytest.param(1, 68, 9, 11, 0, id='vec_nq3-c68'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W,off', DW7_CASES)
def test_dwconv7_layernorm_backward(B, C, H, W, off, dt):
    """dwconv7_ln_train -> dwconv7_ln_bwd: dx, d dw-weight, d dw-bias, d ln-weight, d ln-bias against autograd of
    layer_norm(conv2d(x, w, b, groups=C, padding=3)) over channels.  The forward takes 4-aligned views only: the scalar routes get x and gy as
    misaligned channel slices in the backward alone.  The kernel stores u = dwconv(x) + b and the LayerNorm's input gradient du in
    the compute dtype and reads them back, so the reference takes the stored u and rounds its own du the same way (a no-op in fp32)."""
    gen = _gen('dw7', B, C, H, W, off)
    x = _rand(gen, B, C, H, W, dt=dt)
    w = (torch.randn(C, 1, 7, 7, generator=gen, dtype=torch.float64) / 7).float().double()
    b = (torch.randn(C, generator=gen, dtype=torch.float64) * 0.1).float().double()
    lw = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    lb = (torch.randn(C, generator=gen, dtype=torch.float64) * 0.1).float().double()
    gy = _rand(gen, B, C, H, W, dt=dt)
    eps = 1e-6
    xd, _ = _nhwc(x, dt)
    w49c = w.reshape(C, 49).t().contiguous().float().to(DEV)
    y, u = ops.dwconv7_ln_train(xd, w49c, b.float().to(DEV), lw.float().to(DEV), lb.float().to(DEV), eps)
    u_ref = F.conv2d(x, w, b, 1, 3, 1, C)
    _close(u, u_ref, dt, 'u (forward)')
    # reference backward from the stored u
    ur, lwr, lbr = u.double().cpu().requires_grad_(True), lw.clone().requires_grad_(True), lb.clone().requires_grad_(True)
    F.layer_norm(ur.permute(0, 2, 3, 1), (C,), lwr, lbr, eps).permute(0, 3, 1, 2).backward(gy)
    du = _q(ur.grad, dt)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    F.conv2d(xr, wr, br, 1, 3, 1, C).backward(du)
    d_w = torch.full((C, 1, 7, 7), float('nan'), device=DEV)
    d_b, d_lw, d_lb = (torch.full((C,), float('nan'), device=DEV) for _ in range(3))
    xb, _ = _nhwc(x, dt, off, 8, gen=gen)
    gyd, _ = _nhwc(gy, dt, off, 8, gen=gen)
    dx = ops.dwconv7_ln_bwd(xb, u, gyd, w49c, lw.float().to(DEV), eps, d_w, d_b, d_lw, d_lb)
    _close(dx, xr.grad, dt, 'dx')
    _close(d_w, wr.grad, F32, 'd dw weight')
    _close(d_b, br.grad, F32, 'd dw bias')
    _close(d_lw, lwr.grad, F32, 'd ln weight')
    _close(d_lb, lbr.grad, F32, 'd ln bias')


# ------------------------------------------------------------------------------------------------ convolution data gradient
def _ref_dgrad(dx_shape, w, dy, k, s):
    return torch.nn.grad.conv2d_input(dx_shape, w, dy, stride=s, padding=k // 2)


# (B, cin, cout, H, W, k, s, dy_off, mode); cin = dx channels, cout = dy channels; mode: plain / acc (accumulate into random dx) / r2 / acc_r2
DGRAD_CASES = [
    pytest.param(2, 16, 32, 12, 10, 3, 1, 0, 'plain', id='igemm-k3'), pytest.param(2, 24, 16, 9, 7, 1, 1, 0, 'acc', id='igemm-k1-acc'),
    pytest.param(2, 32, 64, 11, 13, 3, 1, 0, 'r2', id='igemm-k3-r2'), pytest.param(1, 8, 16, 1, 1, 3, 1, 0, 'acc_r2', id='igemm-1x1-acc-r2'),
    pytest.param(32, 16, 16, 2, 3, 3, 1, 0, 'plain', id='igemm-many-images-2x3'),
    pytest.param(2, 16, 32, 12, 10, 3, 2, 0, 'plain', id='phase-s2'), pytest.param(2, 32, 16, 8, 14, 3, 2, 0, 'acc_r2', id='phase-s2-acc-r2'),
    pytest.param(1, 8, 16, 2, 2, 3, 2, 0, 'r2', id='phase-s2-2x2'),
    pytest.param(2, 16, 32, 13, 11, 3, 2, 0, 'plain', id='direct-s2-odd'), pytest.param(2, 16, 24, 9, 7, 3, 2, 0, 'acc_r2', id='direct-s2-odd-acc-r2'),
    pytest.param(2, 8, 16, 11, 9, 5, 1, 0, 'acc', id='direct-k5'), pytest.param(2, 8, 16, 11, 9, 5, 2, 0, 'r2', id='direct-k5-s2'),
    pytest.param(2, 16, 32, 12, 10, 3, 1, 'mis', 'plain', id='direct-dy-misaligned'),
    pytest.param(2, 16, 32, 12, 10, 1, 1, 'mis', 'acc_r2', id='direct-k1-dy-misaligned-acc-r2'),
    pytest.param(2, 16, 32, 12, 10, 3, 2, 'mis', 'r2', id='direct-s2-dy-misaligned'),
    pytest.param(1, 4, 12, 1, 1, 3, 2, 0, 'plain', id='direct-1x1-s2'),
]


def _dgrad_case(B, cin, cout, H, W, k, s, dy_off, mode, dt, gen):
    w = (torch.randn(cout, cin, k, k, generator=gen, dtype=torch.float64) / (cin * k * k) ** 0.5).to(dt).double()   # representable in dt
    Ho, Wo = ops.conv_out_hw(H, W, k, s)
    dy = _rand(gen, B, cout, Ho, Wo, dt=dt)
    off = (2 if dt == F32 else 4) if dy_off == 'mis' else 0
    dyd, _ = _nhwc(dy, dt, off, 8, gen=gen)
    dx, big, big0 = _out_buf(B, cin, H, W, dt, 4, 4, gen)
    acc, r2 = mode in ('acc', 'acc_r2'), mode in ('r2', 'acc_r2')
    r2t = _rand(gen, B, cin, H, W, dt=dt) if r2 else None
    old = big0[:, 4:4 + cin].double()
    ops.conv_dgrad(dyd, w.float().to(DEV), k, s, dx, accumulate=acc, r2=_nhwc(r2t, dt)[0] if r2 else None)
    conv = _ref_dgrad((B, cin, H, W), w, dy, k, s)
    return dx, big, big0, conv, old if acc else None, r2t


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,cin,cout,H,W,k,s,dy_off,mode', DGRAD_CASES)
def test_conv_data_gradient(B, cin, cout, H, W, k, s, dy_off, mode, dt):
    """conv_dgrad against torch.nn.grad.conv2d_input in fp64; dx is a channel slice of a wider buffer of random values (borders must stay),
    accumulate adds to those values, r2 is one more addend.  The MFMA routes (igemm, LDS, phases) add r2 in the convolution's epilogue; the direct
    route stores dx and adds r2 in a second pass (ops.conv_dgrad's docstring), so in bf16 its reference rounds the stored dx before r2 is added."""
    gen = _gen('dgrad', B, cin, cout, H, W, k, s, dy_off, mode)
    dx, big, big0, conv, old, r2t = _dgrad_case(B, cin, cout, H, W, k, s, dy_off, mode, dt, gen)
    ref = conv if old is None else conv + old
    direct = dy_off == 'mis' or k == 5 or (s == 2 and (H % 2 or W % 2)) or (dt == BF16 and cout % 8)
    if r2t is not None:
        ref = (_q(ref, dt) if direct else ref) + r2t
    _close(dx, ref, dt, 'dx')
    _borders_untouched(big, big0, 4, cin)


@pytest.mark.parametrize('cin', [32, 64, 96])
def test_conv_data_gradient_lds_route(cin):
    """bf16 stride-1 3x3 data gradient on a map large enough for the conv3x3_lds kernel (dy 64 channels, >= 16384 pixels, h, w >= 16); plain and with
    accumulate + r2 (the epilogue addends); dx in a channel slice."""
    dt = BF16
    for mode in ('plain', 'acc_r2'):
        gen = _gen('lds', cin, mode)
        dx, big, big0, conv, old, r2t = _dgrad_case(2, cin, 64, 96, 96, 3, 1, 0, mode, dt, gen)
        ref = conv if old is None else conv + old
        if r2t is not None:
            ref = ref + r2t
        _close(dx, ref, dt, f'dx {mode}')
        _borders_untouched(big, big0, 4, cin)


# ------------------------------------------------------------------------------------------------ convolution weight gradient
# (B, cin, cout, H, W, k, s, layout, x2, acc); layout: nhwc / slice (x and dy channel slices) / c_mis (channels % 4 -> generic) / nchw (generic) /
# image (3-channel NCHW -> pad-to-4 path)
WGRAD_CASES = [
    pytest.param(2, 16, 32, 12, 10, 3, 1, 'nhwc', False, False, id='mfma-k3'), pytest.param(2, 4, 8, 9, 7, 3, 2, 'nhwc', False, True, id='mfma-k3-s2-c4-acc'),
    pytest.param(2, 12, 20, 11, 13, 1, 1, 'nhwc', True, False, id='mfma-k1-x2-c12'), pytest.param(1, 36, 16, 1, 1, 3, 1, 'nhwc', False, False, id='mfma-1x1'),
    pytest.param(2, 32, 64, 13, 11, 3, 2, 'slice', True, True, id='mfma-s2-odd-slice-x2-acc'), pytest.param(40, 8, 8, 2, 3, 3, 1, 'nhwc', False, False, id='mfma-many-images'),
    pytest.param(2, 64, 20, 8, 8, 1, 1, 'slice', False, False, id='mfma-k1-slice'),
    pytest.param(2, 8, 16, 11, 9, 5, 1, 'nhwc', False, False, id='valu-k5'), pytest.param(2, 12, 8, 9, 10, 5, 2, 'slice', False, True, id='valu-k5-s2-slice-acc'),
    pytest.param(1, 4, 4, 2, 3, 5, 1, 'nhwc', False, False, id='valu-k5-2x3'),
    pytest.param(2, 6, 8, 9, 7, 3, 1, 'c_mis', False, False, id='generic-c6'), pytest.param(2, 8, 10, 7, 6, 3, 2, 'c_mis', False, True, id='generic-cout10-acc'),
    pytest.param(2, 8, 8, 9, 7, 3, 2, 'nchw', False, False, id='generic-nchw'),
    pytest.param(2, 3, 16, 16, 12, 3, 2, 'image', False, False, id='image-pad4'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,cin,cout,H,W,k,s,layout,with_x2,acc', WGRAD_CASES)
def test_conv_weight_gradient(B, cin, cout, H, W, k, s, layout, with_x2, acc, dt):
    """conv_wgrad (+ dbias) against torch.nn.grad.conv2d_weight in fp64.  bf16: the generic and image routes read x in fp32 (the image is rounded to
    bf16 by the pad-to-4 copy); x + x2 is the forward's pre-add, rounded to bf16 as the forward rounds it."""
    gen = _gen('wgrad', B, cin, cout, H, W, k, s, layout, with_x2, acc)
    Ho, Wo = ops.conv_out_hw(H, W, k, s)
    x_dt = F32 if layout in ('c_mis', 'nchw', 'image') else dt
    x = _rand(gen, B, cin, H, W, dt=x_dt)
    dy = _rand(gen, B, cout, Ho, Wo, dt=dt)
    x2 = _rand(gen, B, cin, H, W, dt=dt) if with_x2 else None
    off = (2 if dt == F32 else 4) if layout == 'slice' else 0
    if layout in ('nchw', 'image'):
        xd = x.float().to(DEV).contiguous()
    else:
        xd, _ = _nhwc(x, x_dt, off, 8, gen=gen)
    dyd, _ = _nhwc(dy, dt, off, 8, gen=gen)
    x2d = _nhwc(x2, dt, off, 8, gen=gen)[0] if with_x2 else None
    base = torch.randn(cout, cin, k, k, generator=gen).float()
    dw = base.to(DEV) if acc else torch.full((cout, cin, k, k), float('nan'), device=DEV)
    db = torch.full((cout,), float('nan'), device=DEV) if not acc else torch.zeros(cout, device=DEV)
    ops.conv_wgrad(xd, dyd, k, s, dw, dbias=db, x2=x2d, accumulate=acc)
    ops.flush_wgrad()
    xin = x if x2 is None else x + x2
    if x2 is not None and dt == BF16:
        xin = _q(xin, dt)
    if layout == 'image':
        xin = _q(xin, dt)
    ref = torch.nn.grad.conv2d_weight(xin, (cout, cin, k, k), dy, stride=s, padding=k // 2)
    _close(dw, ref + base.double() if acc else ref, F32, 'dw')
    _close(db, dy.sum((0, 2, 3)), F32, 'dbias')
    if layout in ('nhwc', 'slice') and not acc:
        # the deferred form (per-split partials left in the workspace, one final-sum launch) gives the same bits
        dw2 = torch.full_like(dw, float('nan'))
        with ops.defer_wgrad():
            ops.conv_wgrad(xd, dyd, k, s, dw2, x2=x2d)
        assert torch.equal(dw2, dw)


# ------------------------------------------------------------------------------------------------ grouped / depth-wise convolution gradients
# (B, cin, cout, groups, H, W, k, s, off, acc)
GCONV_CASES = [
    pytest.param(2, 16, 16, 16, 9, 7, 3, 1, 0, False, id='depthwise-k3'), pytest.param(2, 8, 16, 8, 11, 9, 5, 2, 0, True, id='depthwise-mult2-k5-s2-odd-acc'),
    pytest.param(2, 12, 24, 4, 7, 8, 3, 2, 0, False, id='groups4'), pytest.param(1, 8, 8, 8, 1, 1, 3, 1, 0, True, id='depthwise-1x1-acc'),
    pytest.param(32, 4, 4, 4, 2, 3, 3, 1, 0, False, id='many-images-2x3'), pytest.param(2, 16, 16, 16, 9, 7, 3, 2, 2, True, id='depthwise-s2-slice-acc'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,cin,cout,groups,H,W,k,s,off,acc', GCONV_CASES)
def test_grouped_conv_gradients(B, cin, cout, groups, H, W, k, s, off, acc, dt):
    """gconv_dgrad and gconv_wgrad (DWConv) against autograd of F.conv2d(groups) in fp64, with accumulate into random values."""
    gen = _gen('gconv', B, cin, cout, groups, H, W, k, s, off, acc)
    w = (torch.randn(cout, cin // groups, k, k, generator=gen, dtype=torch.float64) / k).float().double()
    Ho, Wo = ops.conv_out_hw(H, W, k, s)
    x = _rand(gen, B, cin, H, W, dt=dt)
    dy = _rand(gen, B, cout, Ho, Wo, dt=dt)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    F.conv2d(xr, wr, None, s, k // 2, 1, groups).backward(dy)
    xd, _ = _nhwc(x, dt, off, 8, gen=gen)
    dyd, _ = _nhwc(dy, dt, off, 8, gen=gen)
    dx, big, big0 = _out_buf(B, cin, H, W, dt, 4, 4, gen)
    old = big0[:, 4:4 + cin].double()
    ops.gconv_dgrad(dyd, w.float().to(DEV), k, s, groups, dx, accumulate=acc)
    _close(dx, xr.grad + old if acc else xr.grad, dt, 'dx')
    _borders_untouched(big, big0, 4, cin)
    base = torch.randn(w.shape, generator=gen).float()
    dw = base.to(DEV) if acc else torch.full(w.shape, float('nan'), device=DEV)
    ops.gconv_wgrad(xd, dyd, k, s, groups, dw, accumulate=acc)
    _close(dw, wr.grad + base.double() if acc else wr.grad, F32, 'dw')
