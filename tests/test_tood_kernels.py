"""Every kernel of the task-aligned head (tood.hip, tood_train.hip), forward and reverse, against a float64 reference on the CPU, per route.  GPU
cases need a real MI355X (-m gpu); the checks of the reference itself (zero offsets = a plain convolution, the columns reproduce the oracle, the
census of tap kinds of every deformable case) run on the host.

mmcv is absent, so the yardstick of the deformable convolution is oracle.tood.modulated_deform_conv3x3 evaluated in float64 (its column part is
kernel_ref._dcn_columns, held equal to it here); gradients are torch.autograd of it.  GroupNorm + act, the layer attention and the gate are plain
torch in float64, differentiated by autograd.

Each case feeds the kernel and the reference the SAME values (rounded to the kernel's dtype first).  Offsets are k/8, k uniform in [-40, 40]: exact
in bf16 and fp32, so every sampling coordinate is exact in fp32 and fp64, both sides take floor() on the same side and no (pixel, tap) is excluded
from any comparison.  Every deformable case is shown, on the reference alone, to contain each kind of tap its map can contain: fully outside, on the
-1 / H / W gate, one / two / four corners inside the image, an integer coordinate, the last row or column (kernel_ref._dcn_draw).

Bounds are kernel_ref._close, unchanged: fp32 outputs relative L2 <= 2e-5 and every element within 1e-4 * max|ref|; bf16 outputs every element
within 2^-8 * |ref| + 1e-3 * max|ref|.  fp32 runs are compared with pure float64.  bf16 runs restate only the roundings that are stored interfaces
of the kernel chain, named at the test: the bf16 column fragment of dcnv2_mfma, and the gu that gn_act_bwd stores in the activation dtype.  The
bf16 `col` of dcn_im2col and the bf16 outputs are the single final rounding the bf16 bound is made for.
"""
import pytest
import torch
import torch.nn.functional as F

from kernel_ref import (BF16, DEV, F32, _borders_untouched, _close, _dcn_census, _dcn_columns, _dcn_draw, _dcn_kinds, _dev, _exact, _gen, _nhwc, _out_buf,
                        _q, _rand)
from oracle import tood

gpu = pytest.mark.gpu
DTS = [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')]
ACTS = {'silu': F.silu, 'relu': F.relu, 'none': lambda t: t}


def _act_code(name):
    from mgdt_yolo_amd import ops
    return {'silu': ops.ACT_SILU, 'relu': ops.ACT_RELU, 'none': ops.ACT_NONE}[name]


def _f32(t):
    return t.float().to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ deformable cases
# (cin, cout, B, H, W, bias, x channel offset, offset/mask channels)
DCNV2_CASES = [
    pytest.param(4, 20, 2, 7, 5, True, 0, 27, id='c4-20-tail-bias'), pytest.param(4, 20, 2, 7, 5, False, 0, 27, id='c4-20-tail-nobias'),
    pytest.param(32, 32, 2, 13, 11, False, 0, 27, id='c32-32-M286-two-blocks'), pytest.param(8, 16, 1, 1, 1, True, 0, 27, id='c8-16-1x1'),
    pytest.param(128, 16, 1, 5, 4, False, 0, 27, id='c128-16-72KiB-lds-opt-in'), pytest.param(8, 20, 2, 7, 5, True, 8, 28, id='c8-20-x-slice-om28')]
# (cin, cout, B, H, W, x channel offset, y channel offset)
MFMA_CASES = [
    pytest.param(8, 16, 2, 7, 5, 0, 0, id='c8-16-3chunks-3padded-M70'), pytest.param(24, 48, 2, 7, 5, 0, 0, id='c24-48-27pieces-1padded'),
    pytest.param(32, 32, 2, 13, 11, 0, 0, id='c32-32-M286'), pytest.param(64, 64, 1, 6, 5, 0, 0, id='c64-64-72KiB-panel-opt-in'),
    pytest.param(8, 16, 2, 7, 5, 8, 16, id='c8-16-x-slice8-y-slice16')]
# (cin, B, H, W, x channel offset, offset/mask channels)
IM2COL_CASES = [
    pytest.param(4, 2, 7, 5, 0, 27, id='c4-7x5'), pytest.param(8, 1, 13, 11, 0, 28, id='c8-13x11-om28'), pytest.param(32, 2, 7, 5, 0, 27, id='c32-7x5'),
    pytest.param(8, 1, 1, 1, 0, 27, id='c8-1x1'), pytest.param(8, 2, 7, 5, 4, 28, id='c8-7x5-x-slice-om28')]
# (cin, B, H, W): Q = cin/4 quads over 8 lanes - 1 (seven idle lanes), 2, 8, 17 (a second trip of the lane loop); M = 9*B*H*W = 630 is no multiple of 32
COL2IM_CASES = [pytest.param(c, b, h, w, id=f'c{c}-{b}x{h}x{w}') for c in (4, 8, 32, 68) for b, h, w in ((2, 7, 5), (1, 13, 11))]


def _dcn_inputs(name, B, cin, H, W, dt, omc=27):
    """x, offsets, mask logits and the (B, omc, H, W) offset/mask map [18 offsets | 9 logits | padding], all representable in dt; the census of the
    offsets is asserted on the reference's rule alone."""
    gen, off = _dcn_draw((name,), B, H, W)
    cen = _dcn_census(off)
    for kind in _dcn_kinds(H, W):
        assert cen[kind] > 0, (kind, {k: v for k, v in cen.items() if k != 'inside_mask'})
    x = _rand(gen, B, cin, H, W, dt=dt)
    logit = _rand(gen, B, 9, H, W, dt=dt)
    om = torch.cat([off, logit, _rand(gen, B, omc - 27, H, W, dt=dt)], 1)
    assert torch.equal(_q(om, dt), om)
    return gen, x, off, logit, om, cen['inside_mask']


def _all_dcn_geometries():
    out = set()
    for name, cases, sel in (('dcnv2', DCNV2_CASES, (2, 3, 4)), ('mfma', MFMA_CASES, (2, 3, 4)), ('im2col', IM2COL_CASES, (1, 2, 3)), ('col2im', COL2IM_CASES, (1, 2, 3))):
        for p in cases:
            out.add((name,) + tuple(p.values[i] for i in sel))
    return sorted(out)


@pytest.mark.parametrize('name,B,H,W', _all_dcn_geometries())
def test_dcn_cases_hold_every_tap_kind(name, B, H, W):
    """Host: the offsets of every deformable case contain at least one (pixel, tap) fully outside, one exactly on the -1 / H / W gate, one on an
    integer coordinate, one on the last row or column, and one with exactly one, two and four corners inside the image (a 1x1 map: every inside tap
    has exactly one).  They are multiples of 1/8 in [-5, 5]."""
    _, _, off, _, _, inside = _dcn_inputs(name, B, 4, H, W, F32)
    assert off.shape == (B, 18, H, W) and torch.equal(off * 8, torch.round(off * 8)) and off.abs().max() <= 5
    assert inside.shape == (B, 9, H, W) and inside.any() and not inside.all()


@pytest.mark.parametrize('B,C,H,W', [(2, 8, 7, 5), (1, 4, 13, 11), (1, 8, 1, 1)])
def test_reference_columns_reproduce_the_oracle(B, C, H, W):
    """Host: weight.view(cout, cin*9) @ _dcn_columns equals oracle.tood.modulated_deform_conv3x3 - the channel-major, tap-minor column order that
    dcn_im2col is held to is the oracle's - and the columns of fully outside taps are exactly zero."""
    gen, x, off, logit, _, inside = _dcn_inputs('cols', B, C, H, W, F32)
    w = _rand(gen, 6, C, 3, 3)
    mask = torch.sigmoid(logit)
    col = _dcn_columns(x, off, mask)
    ref = tood.modulated_deform_conv3x3(x, off, mask, w)
    got = torch.matmul(w.reshape(6, C * 9), col.reshape(B, C * 9, H * W)).reshape(B, 6, H, W)
    assert (got - ref).abs().max().item() <= 1e-13 * ref.abs().max().item()
    assert (col.reshape(B, C, 9, H, W)[(~inside).unsqueeze(1).expand(B, C, 9, H, W)] == 0).all()


def test_reference_with_zero_offsets_is_a_plain_convolution():
    """Host: with zero offsets the reference is F.conv2d(pad 1) for a unit mask, and for a general mask the sum over the taps of the mask of a tap
    times the convolution with that tap's weights alone."""
    gen = _gen('zero-ref')
    x, w, b = _rand(gen, 2, 8, 7, 5), _rand(gen, 20, 8, 3, 3), _rand(gen, 20)
    zero = torch.zeros(2, 18, 7, 5, dtype=torch.float64)
    ref = tood.modulated_deform_conv3x3(x, zero, torch.ones(2, 9, 7, 5, dtype=torch.float64), w, b)
    assert (ref - F.conv2d(x, w, b, 1, 1)).abs().max().item() <= 1e-13 * ref.abs().max().item()
    mask = torch.sigmoid(_rand(gen, 2, 9, 7, 5))
    ref = tood.modulated_deform_conv3x3(x, zero, mask, w, b)
    acc = b.view(1, -1, 1, 1).expand(2, 20, 7, 5).clone()
    for k in range(9):
        wk = torch.zeros_like(w)
        wk[:, :, k // 3, k % 3] = w[:, :, k // 3, k % 3]
        acc += mask[:, k:k + 1] * F.conv2d(x, wk, None, 1, 1)
    assert (ref - acc).abs().max().item() <= 1e-13 * ref.abs().max().item()


# ------------------------------------------------------------------------------------------------ dcnv2: the scalar kernel, fp32 and bf16
def _w_gemm(w):
    """(cout, cin, 3, 3) -> the GEMM order [(tap * cin + ci)][cout] mgdt_dcnv2_fwd reads (nn/modules/head.py)."""
    return _f32(w.permute(2, 3, 1, 0).reshape(9 * w.shape[1], w.shape[0]))


@gpu
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('cin,cout,B,H,W,bias,xoff,omc', DCNV2_CASES)
def test_dcnv2(cin, cout, B, H, W, bias, xoff, omc, dt):
    """dcnv2 (one thread = one pixel x 16 output channels, fp32 weights in LDS) against the oracle in float64: a guarded tail of output channels and a
    second blockIdx.y (cout 20), a second pixel block (M = 286), a 1x1 map, bias and none, x as a channel slice with a 28-channel offset/mask map,
    and cin 128, whose 72 KiB weight tile needs the raised dynamic-LDS limit.  bf16: fp32 arithmetic on bf16 maps, one rounding of the output."""
    from mgdt_yolo_amd import ops
    gen, x, off, logit, om, _ = _dcn_inputs('dcnv2', B, cin, H, W, dt, omc)
    w = _rand(gen, cout, cin, 3, 3, scale=(9 * cin) ** -0.5)
    b = _rand(gen, cout) if bias else None
    ref = tood.modulated_deform_conv3x3(x, off, torch.sigmoid(logit), w, b)
    xd, _ = _nhwc(x, dt, xoff, 4 if xoff else 0, gen=gen)
    y = ops.dcnv2(xd, _nhwc(om, dt)[0], _w_gemm(w), None if b is None else _f32(b), cout)
    assert y.dtype == dt and y.shape == ref.shape
    _close(y, ref, dt, 'y')


@gpu
@pytest.mark.parametrize('dt', DTS)
def test_dcnv2_zero_offsets(dt):
    """Zero offsets: every tap sits on an integer pixel (one corner with weight 1), so dcnv2 is the mask-weighted plain 3x3 convolution that
    test_reference_with_zero_offsets_is_a_plain_convolution holds the reference to."""
    from mgdt_yolo_amd import ops
    gen = _gen('dcnv2-zero', str(dt))
    B, cin, cout, H, W = 2, 8, 20, 7, 5
    x, logit = _rand(gen, B, cin, H, W, dt=dt), _rand(gen, B, 9, H, W, dt=dt)
    w, b = _rand(gen, cout, cin, 3, 3, scale=(9 * cin) ** -0.5), _rand(gen, cout)
    off = torch.zeros(B, 18, H, W, dtype=torch.float64)
    ref = tood.modulated_deform_conv3x3(x, off, torch.sigmoid(logit), w, b)
    y = ops.dcnv2(_nhwc(x, dt)[0], _nhwc(torch.cat([off, logit], 1), dt)[0], _w_gemm(w), _f32(b), cout)
    _close(y, ref, dt, 'y')


@gpu
def test_dcnv2_refuses_a_weight_tile_beyond_the_lds():
    """cin 288: 9 * 288 * 16 * 4 B = 162 KiB of weights do not fit the 160 KiB of LDS; refused on the host (MGDT_BAD_SHAPE = -1), nothing launched."""
    from mgdt_yolo_amd import ops
    x = torch.zeros(1, 288, 2, 2, device=DEV).contiguous(memory_format=torch.channels_last)
    om = torch.zeros(1, 27, 2, 2, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match=r'dcnv2_fwd failed \(-1\).*does not fit'):
        ops.dcnv2(x, om, torch.zeros(9 * 288, 16, device=DEV), None, 16)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ dcnv2_mfma (bf16)
@gpu
@pytest.mark.parametrize('cin,cout,B,H,W,xoff,yoff', MFMA_CASES)
def test_dcnv2_mfma(cin, cout, B, H, W, xoff, yoff):
    """dcnv2_mfma against the oracle in float64 with ONE rounding restated: the sampled-and-modulated column fragment, which the kernel rounds to
    bf16 to feed the MFMA (the B operand is a stored interface; weights and maps are bf16 already, the accumulation is fp32, the output is rounded
    once).  cin 8: 9 pieces in 3 chunks, the last three lanes' pieces are padding, M = 70 leaves a partial pixel tile; cin 24: 27 pieces, one
    padded; M = 286: a second workgroup; 64 -> 64: the 72 KiB panel behind the dynamic-LDS opt-in; x and y as channel slices of wider buffers."""
    from mgdt_yolo_amd import ops
    gen, x, off, logit, om, _ = _dcn_inputs('mfma', B, cin, H, W, BF16, 28 if xoff else 27)
    w = _rand(gen, cout, cin, 3, 3, dt=BF16, scale=(9 * cin) ** -0.5)
    col = _q(_dcn_columns(x, off, torch.sigmoid(logit)), BF16)
    ref = torch.matmul(w.reshape(cout, cin * 9), col.reshape(B, cin * 9, H * W)).reshape(B, cout, H, W)
    xd, _ = _nhwc(x, BF16, xoff, 8 if xoff else 0, gen=gen)
    pk = ops.PackedConv(_f32(w), None, None, 3, BF16)
    if yoff:
        y, big, big0 = _out_buf(B, cout, H, W, BF16, yoff, 8, gen)
        ops.dcnv2_mfma(xd, _nhwc(om, BF16)[0], pk, out=y)
        _borders_untouched(big, big0, yoff, cout)
    else:
        y = ops.dcnv2_mfma(xd, _nhwc(om, BF16)[0], pk)
    _close(y, ref, BF16, 'y')


# ------------------------------------------------------------------------------------------------ dcn_im2col
@gpu
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('cin,B,H,W,xoff,omc', IM2COL_CASES)
def test_dcn_im2col(cin, B, H, W, xoff, omc, dt):
    """dcn_im2col against the column part of the oracle in float64, in the channel-major, tap-minor order of weight.view(cout, cin*9)
    (test_reference_columns_reproduce_the_oracle).  bf16: the bf16 `col` is the kernel's stored output, rounded once from fp32 - the rounding the
    bf16 bound allows."""
    from mgdt_yolo_amd import ops
    gen, x, off, logit, om, _ = _dcn_inputs('im2col', B, cin, H, W, dt, omc)
    ref = _dcn_columns(x, off, torch.sigmoid(logit))
    xd, _ = _nhwc(x, dt, xoff, 4 if xoff else 0, gen=gen)
    col = ops.dcn_im2col(xd, _nhwc(om, dt)[0])
    assert col.dtype == dt and col.shape == ref.shape
    _close(col, ref, dt, 'col')


# ------------------------------------------------------------------------------------------------ dcn_col2im_bwd
@gpu
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('cin,B,H,W', COL2IM_CASES)
def test_dcn_col2im_bwd(cin, B, H, W, dt):
    """dcn_col2im_bwd against autograd of the oracle's columns in float64 with the loss (columns * gcol).sum(): the input gradient (fp32 atomics,
    rounded once), the 18 offset gradients and the 9 mask-logit gradients (8-lane shuffles over the channel quads), each compared on its own.  The
    offset/mask maps have 28 channels: gom is pre-filled with NaN, every channel must be written, the 28th with exact zeros, and fully outside taps
    give exact zeros.  At an integer coordinate both sides take the derivative towards the next pixel (floor)."""
    from mgdt_yolo_amd import ops
    gen, x, off, logit, om, inside = _dcn_inputs('col2im', B, cin, H, W, dt, 28)
    gcol = _rand(gen, B, 9 * cin, H, W, dt=dt)
    xr, offr, lr = (t.clone().requires_grad_(True) for t in (x, off, logit))
    (_dcn_columns(xr, offr, torch.sigmoid(lr)) * gcol).sum().backward()
    gom = _dev(torch.full((B, 28, H, W), float('nan'), dtype=dt))
    gx, gom2 = ops.dcn_col2im_bwd(_nhwc(gcol, dt)[0], _nhwc(x, dt)[0], _nhwc(om, dt)[0], gom=gom)
    assert gom2 is gom and gx.dtype == dt and gom.dtype == dt
    _close(gx, xr.grad, dt, 'gx')
    _close(gom[:, :18], offr.grad, dt, 'goffset')
    _close(gom[:, 18:27], lr.grad, dt, 'glogit')
    _exact(gom[:, 27:], torch.zeros(B, 1, H, W), 'padding channel')
    got = gom.double().cpu()
    out = ~inside
    assert out.any()
    assert (got[:, 0:18:2][out] == 0).all() and (got[:, 1:18:2][out] == 0).all() and (got[:, 18:27][out] == 0).all(), 'outside taps: non-zero gradient'
    assert (offr.grad[:, 0:18:2][out] == 0).all() and (lr.grad[out] == 0).all()


# ------------------------------------------------------------------------------------------------ nc_affine_act_bwd / relu_mask
@gpu
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('mode', ['silu', 'relu', 'none', 'relu_mask'])
@pytest.mark.parametrize('B,C,H,W,off', [pytest.param(2, 4, 5, 3, 0, id='c4'), pytest.param(2, 64, 6, 5, 0, id='c64'),
                                         pytest.param(2, 64, 6, 5, 4, id='c64-slices'), pytest.param(2, 4, 1, 1, 0, id='c4-1x1')])
def test_nc_affine_act_bwd(B, C, H, W, off, mode, dt):
    """nc_affine_act_bwd: gu = g * act'(y * A[n, c] + B[n, c]) against autograd of the activation in float64, and its A = B = None form (relu_mask) on
    real ReLU outputs, whose exact zeros have derivative 0; g, y and gu as channel slices of wider random buffers whose borders stay untouched."""
    from mgdt_yolo_amd import ops
    gen = _gen('ncaff', B, C, H, W, off, mode, str(dt))
    g = _rand(gen, B, C, H, W, dt=dt)
    if mode == 'relu_mask':
        y = F.relu(_rand(gen, B, C, H, W, dt=dt))
        assert (y == 0).sum() > 0
        A = Bc = None
        u = y.clone().requires_grad_(True)
        act = 'relu'
    else:
        y = _rand(gen, B, C, H, W, dt=dt)
        A = (torch.rand(B, C, generator=gen, dtype=torch.float64) + 0.5).float().double()
        Bc = (torch.randn(B, C, generator=gen, dtype=torch.float64) * 0.3).float().double()
        u = (y * A[:, :, None, None] + Bc[:, :, None, None]).requires_grad_(True)
        act = mode
    ACTS[act](u).backward(g)
    gd, yd = _nhwc(g, dt, off, 4 if off else 0, gen=gen)[0], _nhwc(y, dt, off, 4 if off else 0, gen=gen)[0]
    if off:
        gu, big, big0 = _out_buf(B, C, H, W, dt, off, 4, gen)
        ops.nc_affine_act_bwd(gd, yd, None if A is None else _f32(A), None if A is None else _f32(Bc), _act_code(act), out=gu)
        _borders_untouched(big, big0, off, C)
    elif mode == 'relu_mask':
        gu = ops.relu_mask(gd, yd)
    else:
        gu = ops.nc_affine_act_bwd(gd, yd, _f32(A), _f32(Bc), _act_code(act))
    assert gu.dtype == dt
    _close(gu, u.grad, dt, 'gu')
    if mode == 'relu_mask':
        assert (gu.double().cpu()[y == 0] == 0).all(), 'derivative at an exact zero of the ReLU output'


# ------------------------------------------------------------------------------------------------ GroupNorm + act backward
# (B, C, H, W, groups, act, shift, scale)
GN_CASES = [
    pytest.param(2, 64, 6, 5, 16, 'silu', 0.0, 1.0, id='c64-g16-silu'), pytest.param(2, 16, 9, 7, 16, 'silu', 0.0, 1.0, id='c16-one-channel-per-group'),
    pytest.param(1, 32, 1, 1, 16, 'relu', 0.0, 4e-3, id='c32-1x1-relu'), pytest.param(3, 320, 5, 6, 16, 'silu', 0.0, 1.0, id='c320-second-trip'),
    pytest.param(2, 64, 6, 5, 16, 'silu', 3.0, 1.0, id='c64-mean3')]


@gpu
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('B,C,H,W,groups,act,shift,scale', GN_CASES)
def test_gn_act_bwd(B, C, H, W, groups, act, shift, scale, accumulate, dt):
    """gn_act_bwd (gn_affine -> nc_affine_act_bwd -> nc_reduce -> gn_bwd_coef -> nc_axpby): dy, dgamma and dbeta against autograd of
    act(F.group_norm(y)) in float64; accumulate adds to pre-loaded dgamma / dbeta.  bf16 restates ONE rounding: gu = g * act'(u), which the chain
    stores in the activation dtype, sums for the statistics and then overwrites in place with dy; everything else stays float64.
    The 1x1 map has two values per group.  There dy = rstd * (p1 - p2) / 2 * eps / (var + eps): at unit scale it is 1e-5 of its own terms and no fp32
    evaluation resolves it, so that case draws y with std 4e-3 (var of the order of eps = 1e-5), where the same formula is well conditioned and eps
    itself is in play."""
    from mgdt_yolo_amd import ops
    gen = _gen('gnbwd', B, C, H, W, groups, act, shift, scale, accumulate, str(dt))
    y = _rand(gen, B, C, H, W, dt=dt, scale=scale, shift=shift)
    g = _rand(gen, B, C, H, W, dt=dt)
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = (torch.randn(C, generator=gen, dtype=torch.float64) * 0.3).float().double()
    eps = 1e-5
    yr, ga, be = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    u = F.group_norm(yr, groups, ga, be, eps)
    ud = u.detach().requires_grad_(True)
    ACTS[act](ud).backward(g)
    u.backward(ud.grad if dt == F32 else _q(ud.grad, BF16))
    if accumulate:
        dg0, db0 = _rand(gen, C), _rand(gen, C)
    else:
        dg0 = db0 = torch.full((C,), float('nan'), dtype=torch.float64)
    dgamma, dbeta = _f32(dg0), _f32(db0)
    dy = ops.gn_act_bwd(_nhwc(g, dt)[0], _nhwc(y, dt)[0], _f32(gamma), _f32(beta), groups, eps, _act_code(act), dgamma, dbeta, accumulate)
    assert dy.dtype == dt
    _close(dy, yr.grad, dt, 'dy')
    _close(dgamma, ga.grad + dg0 if accumulate else ga.grad, F32, 'dgamma')
    _close(dbeta, be.grad + db0 if accumulate else be.grad, F32, 'dbeta')


# ------------------------------------------------------------------------------------------------ layer attention backward (fp32)
@gpu
@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C,hid,S', [pytest.param(128, 16, 2, id='c128-hid16-s2'), pytest.param(6, 3, 3, id='c6-hid3-s3'),
                                     pytest.param(8, 300, 2, id='c8-hid300-bias-sums-past-256')])
def test_tood_layer_attn_bwd(C, hid, S, B, accumulate):
    """tood_layer_attn_bwd against autograd in float64 of scale[n, k*feat + j] = sigmoid(W2 relu(W1 (sums/hw) + b1) + b2)[k] with the loss
    (scale * dscale).sum(): dsums, dW1, db1, dW2, db2 each compared, written (over NaN) or accumulated onto pre-loaded values.  hid 300: the sums
    over the images of db1 need more than one 256-thread block."""
    from mgdt_yolo_amd import ops
    gen = _gen('tla-bwd', C, hid, S, B, accumulate)
    hw = 30
    sums = _rand(gen, B, C, scale=hw ** 0.5, shift=0.2 * hw)
    dscale = _rand(gen, B, C)
    w1, b1 = _rand(gen, hid, C, scale=C ** -0.5), _rand(gen, hid, scale=0.1)
    w2, b2 = _rand(gen, S, hid, scale=hid ** -0.5), _rand(gen, S, scale=0.1)
    sr, w1r, b1r, w2r, b2r = (t.clone().requires_grad_(True) for t in (sums, w1, b1, w2, b2))
    wk = torch.sigmoid(torch.relu((sr / hw) @ w1r.T + b1r) @ w2r.T + b2r)
    (wk.repeat_interleave(C // S, 1) * dscale).sum().backward()
    refs = [w1r.grad, b1r.grad, w2r.grad, b2r.grad]
    assert all(r.abs().max() > 0 for r in refs)
    old = [_rand(gen, *r.shape) if accumulate else torch.full(r.shape, float('nan'), dtype=torch.float64) for r in refs]
    bufs = [_f32(o) for o in old]
    dsums = ops.tood_layer_attn_bwd(_f32(sums), _f32(dscale), hw, _f32(w1), _f32(b1), _f32(w2), _f32(b2), S, *bufs, accumulate)
    _close(dsums, sr.grad, F32, 'dsums')
    for name, buf, r, o in zip(('dW1', 'db1', 'dW2', 'db2'), bufs, refs, old):
        _close(buf, r + o if accumulate else r, F32, name)


# ------------------------------------------------------------------------------------------------ probability gate backward
@gpu
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,H,W', [pytest.param(1, 3, 5, id='1x3x5-partial-pixel-group'), pytest.param(2, 9, 7, id='2x9x7')])
@pytest.mark.parametrize('C,off', [pytest.param(4, 0, id='c4'), pytest.param(64, 4, id='c64-x-slice'), pytest.param(68, 0, id='c68-17-quads')])
def test_pixel_gate_bwd(C, off, B, H, W, dt):
    """pixel_gate_bwd against autograd of x * sigmoid(l) in float64: gx, and glogit = s (1 - s) sum_c g x reduced by 16-lane shuffles (M = 15: the
    last pixel group is partial; C 68: 17 quads, a second trip).  glogit is the one-channel view [:, :1] of a zero-filled four-channel buffer, as
    TOODHead.backward passes it; the other three channels stay zero."""
    from mgdt_yolo_amd import ops
    gen = _gen('pg-bwd', C, off, B, H, W, str(dt))
    x, g, l = _rand(gen, B, C, H, W, dt=dt), _rand(gen, B, C, H, W, dt=dt), _rand(gen, B, 1, H, W, dt=dt)
    xr, lr = x.clone().requires_grad_(True), l.clone().requires_grad_(True)
    (xr * torch.sigmoid(lr)).backward(g)
    gp4 = ops.new_act(B, 4, H, W, dt, DEV).zero_()
    gx, gl = ops.pixel_gate_bwd(_nhwc(g, dt)[0], _nhwc(x, dt, off, 4 if off else 0, gen=gen)[0], _nhwc(l, dt)[0], glogit=gp4[:, :1])
    assert gx.dtype == dt
    _close(gx, xr.grad, dt, 'gx')
    _close(gp4[:, :1], lr.grad, dt, 'glogit')
    _exact(gp4[:, 1:], torch.zeros(B, 3, H, W), 'padding channels of the logit gradient')
