"""The pooling kernels of the YOLOv3 graphs (csrc/pool.hip) and the layers on top of them.  Needs a real MI355X (-m gpu).

mgdt_maxpool2d_fwd / mgdt_maxpool2d_bwd (kernel 2, stride 2 and 1) and mgdt_spp_pool_bwd against F.max_pool2d and its autograd on the same device values
(in float64, so torch's own sums are exact), in fp32 and bf16.  The comparison is test_maxpool5_backward's: inputs on three levels, so ties are everywhere
and the argmax rule (first maximum in (ky, kx) scan order, a NaN replaces what came before, -0.0 == 0.0) decides every element; gy in small integers, so
every gathered sum is exact and the results must be EQUAL.  Each case id names the route it forces by shape or alignment alone: `v` 16-byte accesses,
`s` one element per lane; for the SPP reverse pass `lds` (plane in LDS, `v4` / `s` loads) and `glob` (the global-memory route, past 1638 pixels).
ops.sppf_pools' second and third slot against the direct 9x9 / 13x13 windows.  Every kernel gives the same bits on a second run and under capture.
Layers: MaxPool2d, ZeroPad2d and SPP forward and backward() against float64 torch modules with the same weights, under test_train_modules.py's bounds
(fp32 min(cap, max(2e-5, 8 x d32)), bf16 3 x dbf, both from the CPU restatement alone; the parameter-free layers under kernel_ref._close).
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import inputs as GI
import yolov3_ref as Y3
from kernel_ref import BF16, DEV, F32, _borders_untouched, _close, _gen, _nhwc, _out_buf
from mgdt_yolo_amd import ops

pytestmark = pytest.mark.gpu
DTS = [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')]


def _same(got, ref, what=''):
    """equal element for element, a NaN matching a NaN"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~((got == ref) | (got.isnan() & ref.isnan()))
    assert not bad.any(), (what, f'{int(bad.sum())} of {bad.numel()} elements differ', (got - ref).abs().nan_to_num().max().item())


def _bits(a, b):
    """the same bits (torch.equal calls a NaN unequal to itself)"""
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _ints(gen, *shape):
    return torch.randint(-4, 5, shape, generator=gen).double()


def _autograd(xd, fn, gys):
    """fn(x) -> outputs, on the device in float64 from the values the kernel reads; returns (outputs, dx)"""
    xr = xd.detach().double().requires_grad_(True)
    ys = fn(xr)
    torch.autograd.backward(ys, [g.detach().double() for g in gys])
    return [y.detach() for y in ys], xr.grad


# ------------------------------------------------------------------------------------------------ MaxPool2d(2, 2)
# (B, C, H, W, off, kind); bf16 takes 16-byte accesses at C % 8 == 0, fp32 at C % 4 == 0, both only on aligned views
S2_CASES = [
    pytest.param(2, 8, 2, 2, 0, 'quant', id='v-2x2'),
    pytest.param(2, 8, 2, 3, 0, 'quant', id='v-2x3-odd-w'),
    pytest.param(2, 8, 7, 9, 0, 'quant', id='v-7x9-odd-both'),
    pytest.param(2, 16, 12, 10, 0, 'quant', id='v-c16-12x10'),
    pytest.param(2, 6, 9, 7, 0, 'quant', id='s-c6-9x7'),
    pytest.param(2, 16, 12, 10, 2, 'rand', id='s-slice-at-2'),
    pytest.param(2, 8, 10, 10, 0, 'nan', id='v-nan'),
    pytest.param(2, 6, 5, 4, 0, 'nan', id='s-nan'),
    pytest.param(48, 8, 4, 6, 0, 'quant', id='v-48-images'),
]


def _pool_case(B, C, H, W, off, kind, dt, s, pad):
    """forward into a channel slice of a wider buffer and into a fresh map, backward into a slice and into a fresh map; all against autograd"""
    gen = _gen('pool2', B, C, H, W, off, kind, s, pad)
    x = Y3.pool_input(gen, B, C, H, W, kind)
    xd, _ = _nhwc(x, dt, off, 8 if off else 0, gen=gen)
    if pad:
        from mgdt_yolo_amd.nn.modules import ZeroPad2d
        padm = ZeroPad2d((0, 1, 0, 1))
        xin = padm(xd)
        assert tuple(xin.shape) == (B, C, H + 1, W + 1) and (xin[:, :, -1, :] == 0).all() and (xin[:, :, :, -1] == 0).all()
        fn = lambda t: [F.max_pool2d(F.pad(t, (0, 1, 0, 1)), 2, s)]
    else:
        xin = xd
        fn = lambda t: [F.max_pool2d(t, 2, s)]
    oh, ow = (xin.shape[2] - 2) // s + 1, (xin.shape[3] - 2) // s + 1
    gy = _ints(gen, B, C, oh, ow)
    gyd, _ = _nhwc(gy, dt, off, 8 if off else 0, gen=gen)
    (y_ref,), gx_ref = _autograd(xd, fn, [gyd])
    y = ops.maxpool2d(xin, 2, s)
    assert y.dtype == dt and tuple(y.shape) == (B, C, oh, ow)
    _same(y, y_ref, 'y')
    out, big, big0 = _out_buf(B, C, oh, ow, dt, 2, 6, gen)
    assert ops.maxpool2d(xin, 2, s, out=out).data_ptr() == out.data_ptr()
    _same(out, y_ref, 'y into a slice')
    _borders_untouched(big, big0, 2, C)
    gxin = ops.maxpool2d_bwd(xin, gyd, 2, s)
    assert gxin.dtype == dt and gxin.shape == xin.shape
    gx = padm.backward(gxin) if pad else gxin
    _same(gx, gx_ref, 'gx')
    assert _bits(ops.maxpool2d_bwd(xin, gyd, 2, s), gxin) and _bits(ops.maxpool2d(xin, 2, s), y), 'a second run gives other bits'
    gout, gbig, gbig0 = _out_buf(B, C, xin.shape[2], xin.shape[3], dt, 2, 6, gen)
    ops.maxpool2d_bwd(xin, gyd, 2, s, gx=gout)
    assert torch.equal(gout, gxin)
    _borders_untouched(gbig, gbig0, 2, C)
    return xin, gyd, gxin, gx


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W,off,kind', S2_CASES)
def test_maxpool2d_stride2_forward_and_backward(B, C, H, W, off, kind, dt):
    """floor((H - 2) / 2) + 1 rows: an odd trailing row / column is not read and gets a zero gradient"""
    _, _, gx, _ = _pool_case(B, C, H, W, off, kind, dt, 2, False)
    if H % 2:
        assert (gx[:, :, -1, :] == 0).all()
    if W % 2:
        assert (gx[:, :, :, -1] == 0).all()


def test_maxpool2d_refuses_an_empty_output_and_other_geometries():
    x = torch.zeros(1, 8, 1, 1, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match='smaller than the window'):
        ops.maxpool2d(x, 2, 2)
    with pytest.raises(RuntimeError, match='smaller than the window'):
        ops.maxpool2d_bwd(x, x, 2, 1)
    x = torch.zeros(1, 8, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match='max pooling: only kernel 2'):
        ops.maxpool2d(x, 3, 2)
    with pytest.raises(RuntimeError, match='maxpool2d_fwd failed'):
        ops.maxpool2d(x, 2, 2, out=torch.zeros(1, 8, 3, 2, device=DEV).contiguous(memory_format=torch.channels_last))


# ------------------------------------------------------------------------------------------------ ZeroPad2d((0, 1, 0, 1)) + MaxPool2d(2, 1)
S1_CASES = [
    pytest.param(2, 8, 1, 1, 0, 'quant', id='v-1x1'),
    pytest.param(2, 8, 2, 3, 0, 'quant', id='v-2x3'),
    pytest.param(2, 6, 3, 3, 0, 'quant', id='s-c6-3x3'),
    pytest.param(2, 24, 20, 20, 0, 'quant', id='v-c24-20x20'),
    pytest.param(2, 8, 6, 5, 0, 'neg', id='v-all-negative'),
    pytest.param(2, 8, 6, 5, 0, 'zeros', id='v-zeros-and-minus-zeros'),
    pytest.param(2, 6, 6, 5, 2, 'zeros', id='s-zeros-slice'),
    pytest.param(2, 8, 10, 10, 0, 'nan', id='v-nan'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W,off,kind', S1_CASES)
def test_zeropad_then_maxpool2d_stride1_forward_and_backward(B, C, H, W, off, kind, dt):
    """The pool sees the pad as ordinary zeros.  All-negative input: every right / bottom border window's maximum is a pad zero, its gradient goes to the pad
    and the interior view drops it.  Zeros and -0.0 on the border: they tie with the pad, the pixel comes first in the scan and keeps the gradient."""
    xin, gyd, gxin, gx = _pool_case(B, C, H, W, off, kind, dt, 1, True)
    if kind == 'neg':
        assert gxin[:, :, :, -1].abs().sum() > 0 and gxin[:, :, -1, :].abs().sum() > 0, 'the pad took no gradient'
        assert torch.equal(gxin[:, :, :-1, -1], gyd[:, :, :, -1]), 'a right border window: the first maximum is the pad zero of its first row'
    if kind == 'zeros':
        assert (gxin[:, :, :-1, -1] == 0).all(), 'a +-0 border pixel comes first in the scan: the pad column gets nothing from these windows'


# ------------------------------------------------------------------------------------------------ SPP reverse pass
SPP_CASES = [
    pytest.param(2, 8, 1, 1, 'quant', False, id='lds_v4-1x1'),
    pytest.param(3, 4, 2, 3, 'quant', False, id='lds_v4-2x3-smaller-than-every-window'),
    pytest.param(2, 6, 9, 7, 'quant', False, id='lds_s-c6-9x7-ties'),
    pytest.param(2, 16, 20, 20, 'quant', False, id='lds_v4-c16-20x20'),
    pytest.param(1, 24, 20, 20, 'pool', False, id='lds_v4-c24-20x20-plateaus-partial-block'),
    pytest.param(1, 4, 41, 37, 'quant', False, id='lds_v4-41x37'),
    pytest.param(1, 8, 40, 40, 'pool', False, id='lds_v4-40x40-plateaus'),
    pytest.param(1, 4, 44, 40, 'quant', False, id='glob-44x40'),
    pytest.param(1, 3, 45, 38, 'pool', False, id='glob-c3-45x38-plateaus'),
    pytest.param(2, 8, 12, 10, 'quant', True, id='lds_v4-slices-of-the-concat-buffers'),
    pytest.param(2, 6, 12, 10, 'quant', True, id='lds_s-slices-c6'),
    pytest.param(2, 8, 10, 10, 'nan', False, id='lds_v4-nan'),
    pytest.param(1, 4, 44, 40, 'nan', False, id='glob-nan'),
]


def _spp_operands(B, C, H, W, kind, slices, dt):
    gen = _gen('spp', B, C, H, W, kind, slices)
    x = Y3.pool_input(gen, B, C, H, W, kind)
    gs = [_ints(gen, B, C, H, W) for _ in range(3)]
    if slices:              # as SPP.backward passes them: x = slot 0 of the 4 c_ concat buffer, g_k = slots 1 - 3 of cv2's input gradient
        cat = torch.randn(B, 4 * C, H, W, generator=gen).double()
        cat[:, :C] = x
        catd, _ = _nhwc(cat, dt)
        gcatd, _ = _nhwc(torch.cat([_ints(gen, B, C, H, W)] + gs, 1), dt)
        return catd[:, :C], [gcatd[:, (i + 1) * C:(i + 2) * C] for i in range(3)]
    return _nhwc(x, dt)[0], [_nhwc(g, dt)[0] for g in gs]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W,kind,slices', SPP_CASES)
def test_spp_pool_backward(B, C, H, W, kind, slices, dt):
    """gx = sum over k of the adjoint of MaxPool2d(k, 1, k // 2) at x applied to g_k, against autograd of the three direct pools"""
    xd, gds = _spp_operands(B, C, H, W, kind, slices, dt)
    _, gx_ref = _autograd(xd, lambda t: [F.max_pool2d(t, k, 1, k // 2) for k in (5, 9, 13)], gds)
    gx = ops.spp_pool_bwd(xd, *gds)
    assert gx.dtype == dt and tuple(gx.shape) == (B, C, H, W) and gx.is_contiguous(memory_format=torch.channels_last)
    _same(gx, gx_ref.to(dt), 'gx')           # up to 275 windows x |g| <= 4: exact in fp32; the one bf16 store rounds sums past 256 (the reference likewise)
    assert torch.equal(ops.spp_pool_bwd(xd, *gds), gx), 'a second run gives other bits'


@pytest.mark.parametrize('dt', DTS)
def test_three_chained_5x5_adjoints_are_not_the_direct_result(dt):
    """Why the kernel exists: on tied inputs SPPF's chain maxpool5_bwd(x, g5 + maxpool5_bwd(y1, g9 + maxpool5_bwd(y2, g13))) routes to other pixels than
    the first maximum of the direct 9x9 / 13x13 window, although the forward values agree bit for bit."""
    xd, gds = _spp_operands(2, 16, 20, 20, 'quant', False, dt)
    y1, y2, y3 = (ops.like(xd) for _ in range(3))
    ops.sppf_pools(xd, y1, y2, y3)
    chain = ops.maxpool5_bwd(xd, ops.add(gds[0], ops.maxpool5_bwd(y1, ops.add(gds[1], ops.maxpool5_bwd(y2, gds[2])))))
    direct = ops.spp_pool_bwd(xd, *gds)
    if dt == F32:
        assert chain.double().sum().item() == direct.double().sum().item(), 'both conserve the gradient mass'
    assert not torch.equal(chain, direct)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('B,C,H,W', [pytest.param(3, 8, 2, 3, id='2x3'), pytest.param(2, 16, 20, 20, id='20x20'), pytest.param(1, 8, 41, 37, id='41x37')])
def test_sppf_pools_slots_are_the_direct_9x9_and_13x13_windows(B, C, H, W, dt):
    gen = _gen('sppfwd', B, C, H, W)
    xd, _ = _nhwc(torch.randn(B, C, H, W, generator=gen).double(), dt)
    ys = [ops.like(xd) for _ in range(3)]
    ops.sppf_pools(xd, *ys)
    for y, k in zip(ys, (5, 9, 13)):
        _same(y, F.max_pool2d(xd.double(), k, 1, k // 2), f'k={k}')


@pytest.mark.parametrize('dt', DTS)
def test_pool_kernels_give_the_same_bits_under_capture(dt):
    gen = _gen('capture')
    xd, _ = _nhwc(Y3.pool_input(gen, 2, 16, 20, 20, 'quant'), dt)
    g2, _ = _nhwc(_ints(gen, 2, 16, 10, 10), dt)
    g1, _ = _nhwc(_ints(gen, 2, 16, 19, 19), dt)
    gs = [_nhwc(_ints(gen, 2, 16, 20, 20), dt)[0] for _ in range(3)]

    def run():
        return (ops.maxpool2d(xd, 2, 2), ops.maxpool2d(xd, 2, 1), ops.maxpool2d_bwd(xd, g2, 2, 2), ops.maxpool2d_bwd(xd, g1, 2, 1), ops.spp_pool_bwd(xd, *gs))
    eager = run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ layers
def _as_layer(m, dt):
    from mgdt_yolo_amd.nn.modules.conv import HipModule
    m = m.to(DEV).train()
    for sub in m.modules():
        if isinstance(sub, HipModule):
            sub._cdtype = dt
    return m


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('s,H,W', [pytest.param(2, 7, 10, id='s2-7x10'), pytest.param(1, 5, 6, id='s1-5x6')])
def test_maxpool2d_layer_against_float64(s, H, W, dt):
    """train-mode forward + backward() on untied values against nn.MaxPool2d in float64 (the layer keeps only x: no index tensor); eval keeps nothing"""
    from mgdt_yolo_amd.nn.modules import MaxPool2d
    gen = _gen('mp-layer', s, H, W)
    x = torch.randn(2, 16, H, W, generator=gen).to(dt).double()
    ref = nn.MaxPool2d(2, s, 0)
    xr = x.clone().requires_grad_(True)
    y_ref = ref(xr)
    gy = torch.randn(y_ref.shape, generator=gen).to(dt).double()
    y_ref.backward(gy)
    m = _as_layer(MaxPool2d(2, s, 0), dt)
    assert isinstance(m, nn.MaxPool2d) and not list(m.parameters()) and not m.state_dict()
    xd, gd = _nhwc(x, dt)[0], _nhwc(gy, dt)[0]
    with ops.force_ctx():
        y = m(xd)
    assert len(m._ctx) == 1 and m._ctx[0] is xd
    dx = m.backward(gd)
    assert not m._ctx and y.dtype == dt and dx.dtype == dt
    _same(y, y_ref.detach(), 'y')
    _close(dx, xr.grad, dt, 'dx')
    with torch.no_grad():
        assert torch.equal(m.eval()(xd), y) and not m.__dict__.get('_ctx')


@pytest.mark.parametrize('dt', DTS)
def test_zeropad_maxpool_layers_on_post_silu_values_against_float64(dt):
    """yolov3-tiny rows 11 - 12 on values as SiLU leaves them (down to -0.278): windows whose maximum is a pad zero are live, their gradient is dropped"""
    from mgdt_yolo_amd.nn.modules import MaxPool2d, ZeroPad2d
    gen = _gen('pad-layer')
    x = F.silu(torch.randn(2, 16, 6, 5, generator=gen) * 1.5 - 0.5).to(dt).double()
    assert (x[:, :, -1, :] < 0).any() and (x[:, :, :, -1] > 0).any()
    xr = x.clone().requires_grad_(True)
    y_ref = nn.MaxPool2d(2, 1, 0)(nn.ZeroPad2d((0, 1, 0, 1))(xr))
    gy = torch.randn(y_ref.shape, generator=gen).to(dt).double()
    y_ref.backward(gy)
    pad, pool = _as_layer(ZeroPad2d((0, 1, 0, 1)), dt), _as_layer(MaxPool2d(2, 1, 0), dt)
    assert isinstance(pad, nn.ZeroPad2d) and not pad.state_dict()
    xd, gd = _nhwc(x, dt)[0], _nhwc(gy, dt)[0]
    with ops.force_ctx():
        y = pool(pad(xd))
    gp = pool.backward(gd)
    dx = pad.backward(gp)
    assert tuple(dx.shape) == tuple(xd.shape) and dx.data_ptr() == gp.data_ptr(), 'the interior view, no copy'
    assert gp[:, :, :, -1].abs().sum() > 0 and gp[:, :, -1, :].abs().sum() > 0, 'no window had a pad zero as its maximum: the case is not live'
    _same(y, y_ref.detach(), 'y')
    _close(dx, xr.grad, dt, 'dx')
    asym = _as_layer(ZeroPad2d((2, 0, 1, 3)), dt)
    _same(asym(xd), F.pad(x, (2, 0, 1, 3)), 'asymmetric pad')
    g = _nhwc(torch.randn(2, 16, 10, 7, generator=gen).to(dt).double(), dt)[0]
    assert torch.equal(asym.backward(g), g[:, :, 1:7, 2:7])


_SPP = {}


def _spp_case():
    """(cpu module, x, gz, {'ref', 'gscale', F32: bounds, BF16: bounds}) computed once from the restatement alone (test_yolov6._repeat_case's recipe)"""
    if not _SPP:
        from mgdt_yolo_amd.nn.modules import SPP
        from mgdt_yolo_amd.seeding import seed_state_dict_
        from test_train_modules import gscale_of, is_grad, rel_err
        m = SPP(32, 32)
        for sub in m.modules():
            if isinstance(sub, nn.BatchNorm2d):
                sub.eps, sub.momentum = 1e-3, 0.03
        seed_state_dict_(m, GI.MODULE_SEED).train()
        r = np.random.default_rng([GI.MODULE_SEED, 33])
        x, gz = (torch.from_numpy(r.standard_normal((2, 32, 7, 9), dtype=np.float32)) for _ in range(2))
        q = {mode: Y3.spp_step(m.state_dict(), x, gz, mode, 0.03) for mode in ('f64', 'f32', 'bf16')}
        ref, gs = q['f64'], gscale_of(q['f64'])
        b32 = {k: min(2e-3 if is_grad(k) else 2e-4, max(2e-5, 8 * rel_err(k, q['f32'][k], v, gs))) for k, v in ref.items()}
        bbf = {k: 3 * rel_err(k, q['bf16'][k], v, gs) for k, v in ref.items()}
        _SPP['case'] = (m, x, gz, {'ref': ref, 'gscale': gs, F32: b32, BF16: bbf})
    return _SPP['case']


@pytest.mark.parametrize('dt', DTS)
def test_spp_training_step_against_float64_autograd(dt):
    """SPP train-mode forward + backward(): output, dx, every parameter gradient and running statistic against the restatement with the three DIRECT pools;
    the module tree and the state-dict keys are the reference's (cv1, cv2, m = three nn.MaxPool2d); a second step gives the same bits."""
    from mgdt_yolo_amd.nn.modules import SPPF
    from test_train_modules import rel_err
    cpu, x, gz, b = _spp_case()
    ref, gs, bnd = b['ref'], b['gscale'], b[dt]
    assert all(0 < b[BF16][k] for k in ref) and b[BF16]['y0'] <= 5e-2, 'vacuous bounds'
    assert isinstance(cpu, SPPF) and [type(p) for p in cpu.m] == [nn.MaxPool2d] * 3 and [p.kernel_size for p in cpu.m] == [5, 9, 13]
    assert list(cpu.state_dict()) == [f'{c}.{k}' for c in ('cv1', 'cv2') for k in ('conv.weight', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var',
                                                                                  'bn.num_batches_tracked')]
    m = _as_layer(copy.deepcopy(cpu), dt)
    xd, gd = _nhwc(x, dt)[0], _nhwc(gz, dt)[0]
    run0 = {k: v.clone() for k, v in m.state_dict().items() if 'running' in k}

    def step():
        m.load_state_dict(run0, strict=False)
        with ops.force_ctx():
            y = m(xd)
        with ops.defer_wgrad():
            dx = m.backward(gd)
        assert m._cat is None and all(not mod.__dict__.get('_ctx') for mod in m.modules())
        got = {'y0': y.clone(), 'dx0': dx.clone()}
        got.update({'g:' + k: p.grad.clone() for k, p in m.named_parameters()})
        for k, sub in m.named_modules():
            if isinstance(sub, nn.BatchNorm2d):
                got['rm:' + k], got['rv:' + k] = sub.running_mean.clone(), sub.running_var.clone()
        return got
    got = step()
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    bad = []
    for k, r in ref.items():
        e = rel_err(k, got[k].float(), r, gs)
        print(f'SPP {str(dt)[6:]} {k}: err {e:.3e}  bound {bnd[k]:.3e}  share {e / bnd[k]:.2f}')
        if not e <= bnd[k]:
            bad.append((k, e, bnd[k]))
    assert not bad, bad
    again = step()
    assert all(torch.equal(again[k], got[k]) for k in got)
