"""Every forward pointwise, pool and norm entry point of ops.* against a float64 reference on the CPU, per route.  GPU cases need a real MI355X
(-m gpu); test_route_predicates runs on the host.

Each case feeds the kernel and the reference the SAME values (rounded to the kernel's dtype first) and forces one route of the C dispatch by
shape or alignment alone; its id names the route.  Channel slices sit inside wider NHWC buffers whose other channels hold random values: offset 2
(fp32, scalar routes), 4 (bf16: drops an 8-wide route to the 4-wide one; fp32: keeps 16-byte alignment) or 8 (keeps the 8-wide route).  Output
buffers are filled with random values and their borders must stay untouched.

Tolerances come from the arithmetic: the kernels compute in fp32 and round their output once.
  fp32 outputs (every fp32 statistic of a bf16 run included): relative L2 error <= 2e-5 and every element within 1e-4 * max|ref|.
  bf16 outputs: every element within 2^-8 * |ref| + 1e-3 * max|ref|.
  Exact operations (max pools, nearest, casts, a single correctly rounded fp32 multiply or add) are compared exactly, NaN against NaN.
Where a kernel stores an intermediate in the compute dtype by design, the reference rounds that intermediate too (stated at the case).
Statistics run on mean-shifted inputs (per-channel mean = 8 x std): E[x^2] - mean^2 formed from fp32 sums loses (mean/std)^2 of precision there.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_ref import BF16, DEV, F32, _borders_untouched, _close, _exact, _gen, _nhwc, _out_buf, _q, _rand

ACTS = {'silu': F.silu, 'relu': F.relu, 'gelu': F.gelu, 'none': lambda t: t}
gpu = pytest.mark.gpu


def _act_code(name):
    from mgdt_yolo_amd import ops
    return {'silu': ops.ACT_SILU, 'relu': ops.ACT_RELU, 'gelu': ops.ACT_GELU, 'none': ops.ACT_NONE}[name]


def _dt_id(dt):
    return 'f32' if dt == F32 else 'bf16'


def _exact_nan(got, ref, what=''):
    """Exact, with NaN equal to NaN (and only to NaN)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    ref = ref.double()
    same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    bad = (~same).sum().item()
    assert bad == 0, (what, f'{bad} elements differ', got[~same][:8].tolist(), ref[~same][:8].tolist())


# ------------------------------------------------------------------------------------------------ host route predicates (mirror the C dispatch)
def sppf_route(dt, c, h, w, all8):
    """mgdt_sppf_pool_fwd: the two-phase kernel when its LDS (rows + three row-maximum planes in the storage type) fits 64 KiB, V = 8 for bf16 views
    that are all 16-byte aligned; else the chained three-pass fp32 plane kernel with 8 or 4 channels per workgroup; else refused."""
    es = 4 if dt == F32 else 2
    v3 = 8 if (dt == BF16 and all8) else 4
    lds3 = (h * (w + 12) + 3 * (h + 12) * w) * v3 * es
    if lds3 <= 64 * 1024:
        return f'two_phase_v{v3}'
    pp = (h + 4) * (w + 4)
    cg = 8 if (c % 8 == 0 and pp * 8 * 2 * 4 <= 64 * 1024) else 4
    return f'chained_cg{cg}' if pp * cg * 2 * 4 <= 64 * 1024 else 'refused'


def decode_route(reg_max, nc):
    """detect_decode_launch: the LDS-transposing tile kernel (fp32 tile [128][no + 1]) for 4-aligned channel counts up to 144 KiB, above 64 KiB with
    the raised dynamic-LDS limit; the scalar kernel otherwise."""
    no = 4 * reg_max + nc
    lds = 128 * (no + 1) * 4
    if no % 4 == 0 and lds <= 144 * 1024:
        return 'tile_big' if lds > 64 * 1024 else 'tile'
    return 'scalar_c4' if no % 4 else 'scalar_lds'


def groupnorm_route(c):
    """mgdt_groupnorm_fwd: pixels spread over the block's threads for C <= 256 (Q = C/4 <= 64), one thread per channel quad otherwise."""
    return 'wide' if c // 4 <= 64 else 'narrow'


def spr_fast_prologue(c, groups):
    """mgdt_spr_attn_scale_fwd with per-tile sums: the latency-lean prologue when C <= 256 and its LDS plus the staged fc weights fit 48 KiB."""
    cw = c // groups
    hid = cw // 4
    lds = (c * 5 + groups * hid + 2 * c) * 4
    wbytes = (hid * (5 * cw + 4) + cw * (hid + 1) + hid + cw + 4) * 4
    return c <= 256 and lds + wbytes <= 48 * 1024


def spr_scale_k(dt, c, h, w, v8):
    """mgdt_spr_attn_scale_fwd: workgroups per image."""
    v = 8 if (dt == BF16 and v8) else 4
    return max(1, min(12, h * w * (c // v) // 2048))


# ------------------------------------------------------------------------------------------------ SPPF: three chained MaxPool2d(5, 1, 2)
# (dt, B, C, H, W, kind); every view is a channel slice of one concat buffer [x | y1 | y2 | y3 | 8 spare channels] (nn/modules/block.py:260)
SPPF_CASES = [
    pytest.param(BF16, 2, 16, 20, 20, 'rand', id='sppf-two_phase_v8-20x20-bf16'),
    pytest.param(BF16, 2, 16, 13, 11, 'ties', id='sppf-two_phase_v8-13x11-ties-bf16'),
    pytest.param(BF16, 1, 8, 1, 1, 'rand', id='sppf-two_phase_v8-1x1-bf16'),
    pytest.param(BF16, 2, 16, 9, 7, 'nan', id='sppf-two_phase_v8-nan-bf16'),
    pytest.param(BF16, 2, 12, 27, 27, 'inf', id='sppf-two_phase_v4-27x27-c12-inf-bf16'),
    pytest.param(BF16, 1, 12, 9, 7, 'nan', id='sppf-two_phase_v4-nan-bf16'),
    pytest.param(BF16, 1, 16, 27, 27, 'ties', id='sppf-chained_cg8-27x27-bf16'),
    pytest.param(BF16, 1, 16, 27, 27, 'nan', id='sppf-chained_cg8-27x27-nan-bf16'),
    pytest.param(BF16, 1, 16, 30, 30, 'inf', id='sppf-chained_cg4-30x30-bf16'),
    pytest.param(BF16, 1, 12, 40, 40, 'nan', id='sppf-chained_cg4-40x40-c12-nan-bf16'),
    pytest.param(F32, 2, 16, 20, 20, 'rand', id='sppf-two_phase_v4-20x20-f32'),
    pytest.param(F32, 2, 12, 13, 11, 'ties', id='sppf-two_phase_v4-13x11-ties-f32'),
    pytest.param(F32, 1, 4, 1, 1, 'rand', id='sppf-two_phase_v4-1x1-f32'),
    pytest.param(F32, 24, 8, 3, 2, 'ties', id='sppf-two_phase_v4-many-images-f32'),
    pytest.param(F32, 2, 8, 9, 7, 'nan', id='sppf-two_phase_v4-nan-f32'),
    pytest.param(F32, 2, 8, 9, 7, 'inf', id='sppf-two_phase_v4-inf-f32'),
    pytest.param(F32, 1, 16, 27, 27, 'rand', id='sppf-chained_cg8-27x27-f32'),
    pytest.param(F32, 1, 16, 27, 27, 'nan', id='sppf-chained_cg8-27x27-nan-f32'),
    pytest.param(F32, 1, 16, 30, 30, 'ties', id='sppf-chained_cg4-30x30-f32'),
    pytest.param(F32, 1, 12, 31, 29, 'nan', id='sppf-chained_cg4-31x29-c12-nan-f32'),
    pytest.param(F32, 1, 8, 44, 44, 'rand', id='sppf-refused-44x44-f32'),
    pytest.param(BF16, 1, 8, 44, 44, 'rand', id='sppf-refused-44x44-bf16'),
]


def _sppf_input(gen, kind, B, C, H, W):
    if kind == 'ties':
        return torch.randint(0, 3, (B, C, H, W), generator=gen).double()
    x = torch.randn(B, C, H, W, generator=gen).double()
    if kind == 'inf':
        m = torch.rand(B, C, H, W, generator=gen)
        x[m < 0.05] = float('inf')
        x[m > 0.9] = float('-inf')
    if kind == 'nan':
        x[0, 1, H // 2, W // 2] = float('nan')             # interior pixel
        x[-1, C - 1, H - 1, 0] = float('nan')              # a corner
        x[-1, 0, 0, W - 1] = float('nan')
    return x


@gpu
@pytest.mark.parametrize('dt,B,C,H,W,kind', SPPF_CASES)
def test_sppf_pools(dt, B, C, H, W, kind):
    """y1, y2, y3 of sppf_pools against three chained F.max_pool2d(5, 1, 2) in fp64 (which propagate NaN, as ATen's max_pool2d does):
    exact, ties, +-inf and NaN included.  The spare channels of the concat buffer and x itself must stay untouched."""
    from mgdt_yolo_amd import ops
    gen = _gen('sppf', str(dt), B, C, H, W, kind)
    x = _q(_sppf_input(gen, kind, B, C, H, W), dt)
    big0 = torch.randn(B, 4 * C + 8, H, W, generator=gen).to(dt)
    big0[:, :C] = x.to(dt)
    big = torch.empty(big0.shape, dtype=dt, device=DEV, memory_format=torch.channels_last)
    big.copy_(big0)
    xs, ys = big[:, :C], [big[:, (i + 1) * C:(i + 2) * C] for i in range(3)]
    route = sppf_route(dt, C, H, W, dt == BF16 and C % 8 == 0)
    if route == 'refused':
        with pytest.raises(RuntimeError, match='sppf_pool'):
            ops.sppf_pools(xs, *ys)
        return
    ops.sppf_pools(xs, *ys)
    refs = [x]
    for _ in range(3):
        refs.append(F.max_pool2d(refs[-1], 5, 1, 2))
    for i in range(3):
        _exact_nan(ys[i], refs[i + 1], f'y{i + 1}')
    got = big.cpu()
    assert torch.equal(got[:, 4 * C:], big0[:, 4 * C:]), 'spare channels written'
    _exact_nan(got[:, :C].double(), x, 'x')


# ------------------------------------------------------------------------------------------------ resamplers (forward)
def _vec_route(dt, off, c):
    """pointwise.hip resamplers / inject / scale: V = 8 for bf16 views that are 16-byte aligned with c % 8 == 0, else V = 4."""
    return 'v8' if (dt == BF16 and off % 8 == 0 and c % 8 == 0) else 'v4'


def _layouts(cases, kinds=('dense', 'slice8', 'slice4')):
    """(dt, off, *case) params with an id that names the vector route: dense and slice8 keep bf16 8-wide (c % 8 == 0), slice4 drops it."""
    out = []
    for dt in (F32, BF16):
        for tag, *case in cases:
            for k in kinds:
                off = {'dense': 0, 'slice8': 8, 'slice4': 4}[k]
                if dt == F32 and k == 'slice8':
                    continue
                c = case[1]
                out.append(pytest.param(dt, off, *case, id=f'{_vec_route(dt, off, c)}-{tag}-{k}-{_dt_id(dt)}'))
    return out


# (tag, B, C, h, w, oh, ow)
AVG_CASES = [('13to5-7to3', 2, 16, 13, 7, 5, 3), ('2x2bins', 2, 8, 8, 8, 4, 4), ('to1x1', 3, 8, 5, 7, 1, 1), ('1x1', 1, 8, 1, 1, 1, 1),
             ('up5to13', 1, 8, 5, 4, 13, 9), ('many-images', 40, 8, 3, 2, 2, 1)]
BIL_CASES = [('5to13', 2, 16, 5, 4, 13, 9), ('7to20', 1, 8, 7, 7, 20, 20), ('2x', 2, 8, 10, 12, 20, 24), ('down13to5', 2, 8, 13, 11, 5, 4),
             ('1x1src', 2, 8, 1, 1, 3, 5), ('to1x1', 1, 8, 6, 5, 1, 1), ('many-images', 40, 8, 2, 3, 4, 6)]
NEAR_CASES = [('2x', 2, 16, 5, 6, 10, 12), ('5to13', 1, 8, 5, 4, 13, 9), ('7to20', 1, 8, 7, 7, 20, 20), ('down13to5', 2, 8, 13, 11, 5, 4),
              ('1x1src', 2, 8, 1, 1, 2, 3), ('many-images', 40, 8, 2, 3, 4, 6)]


def _resample_fwd(op, B, C, h, w, oh, ow, off, dt, tag):
    gen = _gen(tag, B, C, h, w, oh, ow, off, str(dt))
    x = _rand(gen, B, C, h, w, dt=dt)
    xd, _ = _nhwc(x, dt, off, 8, gen=gen)
    y, big, big0 = _out_buf(B, C, oh, ow, dt, off, 8, gen)
    op(xd, y)
    _borders_untouched(big, big0, off, C)
    return x, y


@gpu
@pytest.mark.parametrize('dt,off,B,C,h,w,oh,ow', _layouts(AVG_CASES))
def test_adaptive_avgpool_forward(dt, off, B, C, h, w, oh, ow):
    """adaptive_avgpool against F.adaptive_avg_pool2d (non-dividing bins overlap)."""
    from mgdt_yolo_amd import ops
    x, y = _resample_fwd(ops.adaptive_avgpool, B, C, h, w, oh, ow, off, dt, 'avgf')
    _close(y, F.adaptive_avg_pool2d(x, (oh, ow)), dt, 'y')


@gpu
@pytest.mark.parametrize('dt,off,B,C,h,w,oh,ow', _layouts(BIL_CASES))
def test_bilinear_forward(dt, off, B, C, h, w, oh, ow):
    """bilinear against F.interpolate(mode='bilinear', align_corners=False)."""
    from mgdt_yolo_amd import ops
    x, y = _resample_fwd(ops.bilinear, B, C, h, w, oh, ow, off, dt, 'bilf')
    _close(y, F.interpolate(x, size=(oh, ow), mode='bilinear', align_corners=False), dt, 'y')


@gpu
@pytest.mark.parametrize('dt,off,B,C,h,w,oh,ow', _layouts(NEAR_CASES))
def test_nearest_forward(dt, off, B, C, h, w, oh, ow):
    """nearest against F.interpolate(mode='nearest'): a gather, exact."""
    from mgdt_yolo_amd import ops
    x, y = _resample_fwd(ops.nearest, B, C, h, w, oh, ow, off, dt, 'nearf')
    _exact(y, F.interpolate(x, size=(oh, ow), mode='nearest'), 'y')


# ------------------------------------------------------------------------------------------------ injection tail (InjectionMultiSum_Auto_pool)
# (tag, B, C, h, w, hg, wg): local map h x w, global map hg x wg; pool branch when h < hg
INJ_CASES = [('pool-13to5', 2, 16, 5, 4, 13, 9), ('pool-odd-global', 1, 8, 3, 3, 7, 7), ('bilinear-5to13', 2, 16, 13, 9, 5, 4),
             ('bilinear-odd-global', 1, 8, 20, 20, 7, 7), ('bilinear-same-size', 1, 8, 6, 5, 6, 5)]


@gpu
@pytest.mark.parametrize('dt,off,B,C,h,w,hg,wg', _layouts(INJ_CASES))
def test_inject_forward(dt, off, B, C, h, w, hg, wg):
    """inject(local, ga, gf) against block.py:368-397 with its 1x1 convs factored out: local * pool(ga) + pool(gf) when the local map is smaller
    (no h_sigmoid on that branch, as in the reference), else local * bilinear(h_sigmoid(ga)) + bilinear(gf)."""
    from mgdt_yolo_amd import ops
    gen = _gen('inj', B, C, h, w, hg, wg, off, str(dt))
    loc = _rand(gen, B, C, h, w, dt=dt)
    ga = _rand(gen, B, C, hg, wg, dt=dt, scale=3.0)
    gf = _rand(gen, B, C, hg, wg, dt=dt)
    if h < hg:
        sig, feat = F.adaptive_avg_pool2d(ga, (h, w)), F.adaptive_avg_pool2d(gf, (h, w))
    else:
        sig = F.interpolate(F.relu6(ga + 3) / 6, size=(h, w), mode='bilinear', align_corners=False)
        feat = F.interpolate(gf, size=(h, w), mode='bilinear', align_corners=False)
    ref = loc * sig + feat
    y, big, big0 = _out_buf(B, C, h, w, dt, off, 8, gen)
    ops.inject(_nhwc(loc, dt, off, 8, gen=gen)[0], _nhwc(ga, dt, off, 8, gen=gen)[0], _nhwc(gf, dt, off, 8, gen=gen)[0], out=y)
    _close(y, ref, dt, 'y')
    _borders_untouched(big, big0, off, C)


# ------------------------------------------------------------------------------------------------ MSPA attention: scale_channels, spr_attention(_scale)
def _spr_params(gen, cw):
    hid = cw // 4
    sd = {'a.fc1.weight': torch.randn(hid, 5 * cw, 1, 1, generator=gen, dtype=torch.float64).float().double() * 0.4,
          'a.fc1.bias': torch.randn(hid, generator=gen, dtype=torch.float64).float().double() * 0.2,
          'a.fc2.weight': torch.randn(cw, hid, 1, 1, generator=gen, dtype=torch.float64).float().double() * 0.5,
          'a.fc2.bias': torch.randn(cw, generator=gen, dtype=torch.float64).float().double() * 0.2}
    w = [sd[k].float().to(DEV).contiguous() for k in ('a.fc1.weight', 'a.fc1.bias', 'a.fc2.weight', 'a.fc2.bias')]
    return sd, w


def _ref_spr_attn(x, sd, groups, softmax=True):
    """SPRModule (spr_module.py:20-31) on each channel group with shared weights, then MSPA_C2f's softmax over the groups (block.py:278)."""
    from oracle import layers as OL
    b, c = x.shape[:2]
    cw = c // groups
    attn = torch.cat([OL.spr(t, sd, 'a') for t in x.chunk(groups, 1)], 1).reshape(b, groups, cw)
    if softmax:
        attn = torch.softmax(attn, 1)
    return attn.reshape(b, c)


@gpu
@pytest.mark.parametrize('dt,off,B,C,H,W', [pytest.param(dt, off, 2, 16, 7, 5, id=f'{_vec_route(dt, off, 16)}-{k}-{_dt_id(dt)}')
                                             for dt in (F32, BF16) for k, off in (('dense', 0), ('slice4', 4), ('slice8', 8))
                                             if not (dt == F32 and off == 8)] +
                         [pytest.param(F32, 0, 1, 8, 1, 1, id='v4-1x1-f32'), pytest.param(BF16, 0, 1, 8, 1, 1, id='v8-1x1-bf16')])
def test_scale_channels(dt, off, B, C, H, W):
    """x * attn[n, c]: one fp32 multiply, rounded once to the storage dtype - exact in fp32 and bf16 (the fp64 product of a bf16 / fp32 value and
    an fp32 weight is exact, so rounding it to fp32 and then to the storage dtype is what the kernel does)."""
    from mgdt_yolo_amd import ops
    gen = _gen('scale', B, C, H, W, off, str(dt))
    x = _rand(gen, B, C, H, W, dt=dt)
    a = torch.rand(B, C, generator=gen, dtype=torch.float64).float()
    y, big, big0 = _out_buf(B, C, H, W, dt, off, 8, gen)
    ops.scale_channels(_nhwc(x, dt, off, 8, gen=gen)[0], a.to(DEV), out=y)
    _exact(y, _q(_q(x * a.double()[:, :, None, None], F32), dt), 'y')
    _borders_untouched(big, big0, off, C)


@gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
@pytest.mark.parametrize('B,groups,cw,H,W,softmax', [
    pytest.param(2, 4, 8, 9, 7, True, id='g4-cw8-odd-softmax'), pytest.param(2, 2, 12, 6, 6, False, id='g2-cw12-sigmoid'),
    pytest.param(1, 1, 16, 1, 1, True, id='g1-1x1'), pytest.param(1, 2, 96, 5, 3, True, id='g2-cw96'),
    pytest.param(24, 4, 4, 3, 2, True, id='g4-many-images')])
def test_spr_attention(B, groups, cw, H, W, softmax, dt):
    """spr_attention (pooling pass + MLP kernel) against SPRModule per group, with and without the softmax over groups."""
    from mgdt_yolo_amd import ops
    gen = _gen('spra', B, groups, cw, H, W, softmax, str(dt))
    C = groups * cw
    x = _rand(gen, B, C, H, W, dt=dt, shift=0.3)
    sd, w = _spr_params(gen, cw)
    attn = ops.spr_attention(_nhwc(x, dt)[0], *w, groups, softmax=softmax)
    _close(attn, _ref_spr_attn(x, sd, groups, softmax), F32, 'attn')


def _tile_part(x, tiles_x, tiles_y):
    """The per-tile channel sums a producing kernel leaves for spr_attention_scale: fp32 [b][tiles][c], tile = ty * tiles_x + tx (one slot per tile)."""
    b, c, h, w = x.shape
    th, tw = h // tiles_y, w // tiles_x
    t = x.reshape(b, c, tiles_y, th, tiles_x, tw).sum((3, 5))             # b, c, ty, tx
    return t.permute(0, 2, 3, 1).reshape(b, tiles_y * tiles_x, c).float().contiguous()


# (route, B, groups, cw, H, W, tiles (x, y) or None, pool factors, layout); route = prologue-Kworkgroups
SPRS_CASES = [
    ('general_splits-k1', 2, 4, 8, 9, 7, None, (), 'dense'),
    ('general_splits-k1', 2, 2, 12, 8, 8, None, (2,), 'dense'),
    ('general_splits-k1', 1, 1, 16, 8, 8, None, (4, 2), 'slice4'),
    ('general_splits-k12', 2, 4, 12, 64, 64, None, (), 'dense'),
    ('general_splits-k12', 1, 2, 24, 64, 64, None, (4, 2), 'dense'),
    ('fast_tiles-k1', 2, 4, 8, 8, 8, (4, 2), (2,), 'dense'),
    ('fast_tiles-k1', 1, 2, 80, 8, 4, (2, 2), (), 'dense'),
    ('fast_tiles-k12', 1, 4, 12, 64, 64, (4, 4), (4, 2), 'dense'),
    ('fast_tiles-k12', 1, 1, 48, 64, 64, (8, 4), (4,), 'slice4'),
    ('general_tiles-k1', 1, 2, 128, 8, 4, (2, 2), (2,), 'dense'),
    ('general_tiles-k1', 1, 1, 96, 4, 4, (2, 2), (), 'dense'),
]


def _sprs_params():
    out = []
    for dt in (F32, BF16):
        for route, B, g, cw, H, W, tiles, pools, lay in SPRS_CASES:
            off = 4 if lay == 'slice4' else 0
            v = _vec_route(dt, off, g * cw)
            k = spr_scale_k(dt, g * cw, H, W, v == 'v8')
            assert route.endswith(f'-k{k}'), (route, k)
            pid = f"{route}-{v}-g{g}-cw{cw}-{H}x{W}-pools{''.join(map(str, pools)) or 0}-{lay}-{_dt_id(dt)}"
            out.append(pytest.param(dt, B, g, cw, H, W, tiles, pools, off, id=pid))
    return out


@gpu
@pytest.mark.parametrize('dt,B,groups,cw,H,W,tiles,pools,off', _sprs_params())
def test_spr_attention_scale(dt, B, groups, cw, H, W, tiles, pools, off):
    """spr_attention_scale: out = x * softmax_over_groups(SPR(x_group)), the attention from the general prologue (its own pooling pass over 64 row
    splits, or per-tile sums of a producing kernel) or the fast per-tile prologue (c <= 256, cw <= 80), and up to two F x F average-pooled copies in
    the same launch.  The pooled copies pool the STORED scaled map (every value rounded to the storage dtype first), so the reference pools
    the rounded reference output."""
    from mgdt_yolo_amd import ops
    gen = _gen('sprs', B, groups, cw, H, W, tiles, pools, off, str(dt))
    C = groups * cw
    x = _rand(gen, B, C, H, W, dt=dt, shift=0.2)
    sd, w = _spr_params(gen, cw)
    attn = _ref_spr_attn(x, sd, groups)
    ref = x * attn[:, :, None, None]
    xd, _ = _nhwc(x, dt, off, 8, gen=gen)
    out, big, big0 = _out_buf(B, C, H, W, dt, off, 8, gen)
    pviews = [_out_buf(B, C, H // f, W // f, dt, off, 8, gen) for f in pools]
    kw = {}
    if tiles is not None:
        part = _tile_part(x, *tiles).to(DEV)
        kw = dict(part=part, nsplit=tiles[0] * tiles[1], tiles=tiles)
    ops.spr_attention_scale(xd, *w, groups, out=out, pools=[p[0] for p in pviews], **kw)
    _close(out, ref, dt, 'out')
    _borders_untouched(big, big0, off, C)
    for f, (pv, pb, pb0) in zip(pools, pviews):
        _close(pv, F.adaptive_avg_pool2d(_q(ref, dt), (H // f, W // f)), dt, f'pool F={f}')
        _borders_untouched(pb, pb0, off, C)


# ------------------------------------------------------------------------------------------------ BatchNorm statistics (+ running stats) and bn_act
# (route, B, C, H, W, off, act, residuals): off = channel offset of the views inside a wider buffer; residuals: '' / 'r1' / 'r1r2' / 'r1mis'
BNF_CASES = [
    ('bnf_v4', 4, 16, 128, 128, 0, 'silu', ''), ('bnf_v4', 4, 16, 128, 128, 0, 'gelu', 'r1'), ('bnf_v4', 1, 256, 256, 256, 0, 'relu', 'r1r2'),
    ('bnf_v4', 2, 8, 1, 1, 0, 'none', ''), ('bnf_v4', 64, 8, 3, 2, 0, 'gelu', 'r1r2'),
    ('scalar', 4, 16, 128, 128, 2, 'silu', 'r1r2'), ('scalar', 2, 6, 181, 181, 0, 'gelu', ''), ('scalar', 2, 16, 9, 7, 2, 'relu', 'r1'),
    ('bnf_v4_stats-scalar_act', 2, 16, 64, 64, 0, 'gelu', 'r1mis'),
]


def _bn_params():
    out = []
    for dt in (F32, BF16):
        for route, B, C, H, W, off, act, res in BNF_CASES:
            out.append(pytest.param(dt, B, C, H, W, off, act, res, id=f'{route}-c{C}-{H}x{W}-B{B}-{act}-{res or "nores"}-{_dt_id(dt)}'))
    return out


@gpu
@pytest.mark.parametrize('dt,B,C,H,W,off,act,res', _bn_params())
def test_bn_stats_and_bn_act(dt, B, C, H, W, off, act, res):
    """bn_stats (momentum 0.03, running mean / var updated in place) then bn_act against F.batch_norm(training=True) on fp64 running buffers and
    the activation in fp64 (exact GELU), on a mean-shifted input: per-channel mean = 8 x std.  The vector kernels (bn_fast.hip) run for
    pixel-linear 4-aligned views, the scalar ones (train.hip) for channel slices at offset 2 or channel counts that are not multiples of 4;
    'bnf_v4_stats-scalar_act': a misaligned residual sends bn_act alone to the scalar kernel."""
    from mgdt_yolo_amd import ops
    gen = _gen('bnf', B, C, H, W, off, act, res, str(dt))
    std = torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    y = _q(torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) * std[None, :, None, None] + 8 * std[None, :, None, None], dt)
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = (torch.randn(C, generator=gen, dtype=torch.float64) * 0.3).float().double()
    rm0 = torch.randn(C, generator=gen, dtype=torch.float64).float().double()
    rv0 = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    eps, mom = 1e-3, 0.03
    rm, rv = rm0.clone(), rv0.clone()
    u = F.batch_norm(y, rm, rv, gamma, beta, True, mom, eps)
    ref = ACTS[act](u)
    mean_ref = y.mean((0, 2, 3))
    rstd_ref = 1.0 / torch.sqrt(y.var((0, 2, 3), unbiased=False) + eps)
    yd, _ = _nhwc(y, dt, off, 8, gen=gen)
    rmd, rvd = rm0.float().to(DEV), rv0.float().to(DEV)
    mean, rstd = ops.bn_stats(yd, eps, mom, rmd, rvd)
    _close(mean, mean_ref, F32, 'mean')
    _close(rstd, rstd_ref, F32, 'rstd')
    _close(rmd, rm, F32, 'running_mean')
    _close(rvd, rv, F32, 'running_var')
    r1 = r2 = None
    if res:
        r1 = _rand(gen, B, C, H, W, dt=dt)
        ref = ref + r1
        r1 = _nhwc(r1, dt, 2 if res == 'r1mis' else off, 8, gen=gen)[0]
    if res == 'r1r2':
        r2 = _rand(gen, B, C, H, W, dt=dt)
        ref = ref + r2
        r2 = _nhwc(r2, dt, off, 8, gen=gen)[0]
    z, big, big0 = _out_buf(B, C, H, W, dt, off, 8, gen)
    ops.bn_act(yd, mean, rstd, gamma.float().to(DEV), beta.float().to(DEV), _act_code(act), out=z, r1=r1, r2=r2)
    _close(z, ref, dt, 'z')
    _borders_untouched(big, big0, off, C)


@gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
@pytest.mark.parametrize('act', list(ACTS))
@pytest.mark.parametrize('route,C,off', [pytest.param('bnf_v4', 64, 0, id='bnf_v4'), pytest.param('scalar', 64, 2, id='scalar-slice'),
                                         pytest.param('scalar', 10, 0, id='scalar-c10')])
def test_bn_act_bias_only(route, C, off, act, dt):
    """The bias-only mode of bn_act (mean = None): act(y + bias), e.g. ConvNeXt's pwconv1 + GELU, over +-6 so that every activation's tails show."""
    from mgdt_yolo_amd import ops
    gen = _gen('bias', C, off, act, str(dt))
    y = _rand(gen, 2, C, 9, 7, dt=dt, scale=3.0)
    b = (torch.randn(C, generator=gen, dtype=torch.float64)).float().double()
    z, big, big0 = _out_buf(2, C, 9, 7, dt, off, 8, gen)
    ops.bn_act(_nhwc(y, dt, off, 8, gen=gen)[0], None, None, None, b.float().to(DEV), _act_code(act), out=z)
    _close(z, ACTS[act](y + b[None, :, None, None]), dt, 'z')
    _borders_untouched(big, big0, off, C)


# ------------------------------------------------------------------------------------------------ GroupNorm (TOODHead) and gn_affine
# (B, C, H, W, groups, act)
GN_CASES = [
    (1, 64, 160, 160, 16, 'relu'), (2, 256, 40, 40, 32, 'none'), (2, 32, 9, 7, 1, 'relu'), (2, 16, 5, 3, 16, 'none'), (40, 16, 3, 2, 4, 'relu'),
    (1, 320, 160, 160, 32, 'relu'), (2, 512, 20, 20, 16, 'none'), (1, 272, 13, 11, 272, 'relu'), (2, 1024, 3, 2, 1, 'none'),
]


def _gn_params():
    out = []
    for dt in (F32, BF16):
        for B, C, H, W, g, act in GN_CASES:
            out.append(pytest.param(dt, B, C, H, W, g, act, id=f'groupnorm-{groupnorm_route(C)}-c{C}-g{g}-{H}x{W}-B{B}-{act}-{_dt_id(dt)}'))
    return out


def _mean_shifted(gen, B, C, H, W, dt):
    """One std and one mean = 8 x std for every channel, so that every group, whatever its channels, has mean / std = 8."""
    std = torch.rand(1, generator=gen, dtype=torch.float64).item() + 0.5
    return _q(torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) * std + 8 * std, dt)


@gpu
@pytest.mark.parametrize('dt,B,C,H,W,groups,act', _gn_params())
def test_groupnorm_forward(dt, B, C, H, W, groups, act):
    """groupnorm (the TOODHead inference path) against F.group_norm + the activation on a mean-shifted input (per-channel mean = 8 x std);
    160 x 160 maps make one thread of the narrow route walk a 1 600-pixel row band.  The output is a channel slice of a random buffer."""
    from mgdt_yolo_amd import ops
    gen = _gen('gn', B, C, H, W, groups, act, str(dt))
    x = _mean_shifted(gen, B, C, H, W, dt)
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = (torch.randn(C, generator=gen, dtype=torch.float64) * 0.3).float().double()
    ref = ACTS[act](F.group_norm(x, groups, gamma, beta, 1e-5))
    y, big, big0 = _out_buf(B, C, H, W, dt, 4, 4, gen)
    ops.groupnorm(_nhwc(x, dt)[0], gamma.float().to(DEV), beta.float().to(DEV), groups, 1e-5, _act_code(act), out=y)
    _close(y, ref, dt, 'y')
    _borders_untouched(big, big0, 4, C)


@gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
@pytest.mark.parametrize('B,C,H,W,groups', [pytest.param(2, 64, 40, 40, 16, id='c64-g16'), pytest.param(1, 256, 80, 80, 32, id='c256-g32'),
                                            pytest.param(2, 16, 3, 5, 16, id='c16-gC'), pytest.param(2, 32, 9, 7, 1, id='c32-g1')])
def test_gn_affine(B, C, H, W, groups, dt):
    """gn_affine (the TOODHead training path: GroupNorm as u = y * A + B from nc_reduce sums) against the fp64 statistics of a mean-shifted input:
    A = gamma * rstd, B = beta - mean * rstd * gamma, and the per-(image, group) mean and rstd."""
    from mgdt_yolo_amd import ops
    gen = _gen('gnaff', B, C, H, W, groups, str(dt))
    y = _mean_shifted(gen, B, C, H, W, dt)
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = (torch.randn(C, generator=gen, dtype=torch.float64) * 0.3).float().double()
    yg = y.reshape(B, groups, -1)
    mean = yg.mean(-1)
    rstd = 1.0 / torch.sqrt(yg.var(-1, unbiased=False) + 1e-5)
    rc, mc = rstd.repeat_interleave(C // groups, 1), mean.repeat_interleave(C // groups, 1)
    A, Bc, m, r = ops.gn_affine(_nhwc(y, dt)[0], gamma.float().to(DEV), beta.float().to(DEV), groups, 1e-5)
    _close(m, mean, F32, 'mean')
    _close(r, rstd, F32, 'rstd')
    _close(A, gamma[None] * rc, F32, 'A')
    _close(Bc, beta[None] - mc * rc * gamma[None], F32, 'B')


# ------------------------------------------------------------------------------------------------ TaskDecomposition layer attention, pixel gate
@gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
@pytest.mark.parametrize('B,C,stacked,la_down,H,W,big', [
    pytest.param(2, 384, 6, 8, 10, 8, False, id='n_head-c384-s6'), pytest.param(1, 768, 6, 8, 5, 4, False, id='s_head-c768-s6'),
    pytest.param(2, 200, 4, 8, 7, 3, False, id='c200-s4'), pytest.param(2, 200, 4, 8, 7, 3, True, id='c200-s4-large-logits')])
def test_tood_layer_attn(B, C, stacked, la_down, H, W, big, dt):
    """tood_layer_attn (from nc_reduce sums) against TaskDecomposition's layer attention (head.py): sigmoid(W2 relu(W1 avgpool(feat) + b1) + b2)
    per stacked block, broadcast to the block's input channels."""
    from mgdt_yolo_amd import ops
    gen = _gen('tla', B, C, stacked, la_down, H, W, big, str(dt))
    hid = C // la_down
    feat = _rand(gen, B, C, H, W, dt=dt, shift=0.2)
    s = 30.0 if big else 1.0
    w1 = (torch.randn(hid, C, generator=gen, dtype=torch.float64) * s / C ** 0.5).float().double()
    b1 = (torch.randn(hid, generator=gen, dtype=torch.float64) * 0.1).float().double()
    w2 = (torch.randn(stacked, hid, generator=gen, dtype=torch.float64) * s / hid ** 0.5).float().double()
    b2 = (torch.randn(stacked, generator=gen, dtype=torch.float64) * 0.1).float().double()
    avg = feat.mean((2, 3))
    wk = torch.sigmoid(torch.relu(avg @ w1.T + b1) @ w2.T + b2)
    ref = wk.repeat_interleave(C // stacked, 1)
    sc = ops.tood_layer_attn(_nhwc(feat, dt)[0], *(t.float().to(DEV).contiguous() for t in (w1, b1, w2, b2)), stacked)
    _close(sc, ref, F32, 'scale')


@gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
@pytest.mark.parametrize('B,C,H,W,scale', [pytest.param(2, 16, 9, 7, 1.0, id='c16'), pytest.param(1, 4, 1, 1, 1.0, id='1x1'),
                                           pytest.param(2, 36, 5, 6, 40.0, id='c36-large-logits')])
def test_pixel_gate(B, C, H, W, scale, dt):
    """pixel_gate: x * sigmoid(gate[n, h, w]) with the gate a one-channel view of a wider buffer; output into a channel slice."""
    from mgdt_yolo_amd import ops
    gen = _gen('pg', B, C, H, W, scale, str(dt))
    x = _rand(gen, B, C, H, W, dt=dt)
    g = _rand(gen, B, 1, H, W, dt=dt, scale=scale)
    y, big, big0 = _out_buf(B, C, H, W, dt, 4, 4, gen)
    ops.pixel_gate(_nhwc(x, dt)[0], _nhwc(g, dt, 3, 4, gen=gen)[0], out=y)
    _close(y, x * torch.sigmoid(g), dt, 'y')
    _borders_untouched(big, big0, 4, C)


# ------------------------------------------------------------------------------------------------ Detect decode (DFL + dist2bbox + sigmoid)
# (route, reg_max, nc, B, H, W, a_off, a_extra, aug): a_total = a_off + H * W + a_extra
DEC_CASES = [
    ('tile', 4, 80, 2, 13, 11, 5, 7, None), ('tile', 4, 80, 1, 16, 16, 0, 0, None), ('tile', 4, 80, 3, 1, 1, 2, 1, (0.83, True, 536.0)),
    ('tile', 4, 80, 2, 9, 7, 3, 0, (0.67, False, 640.0)),
    ('tile_big', 16, 80, 2, 13, 11, 9, 4, None), ('tile_big', 16, 80, 1, 20, 20, 0, 3, (0.83, True, 536.0)),
    ('scalar_c4', 16, 3, 2, 13, 11, 6, 2, None), ('scalar_c4', 16, 3, 1, 7, 5, 0, 0, (0.67, True, 640.0)),
    ('scalar_lds', 16, 224, 1, 12, 11, 4, 4, None), ('scalar_lds', 16, 224, 2, 5, 3, 0, 1, (0.83, False, 536.0)),
]


def _dec_params():
    out = []
    for dt in (F32, BF16):
        for route, R, nc, B, H, W, a_off, extra, aug in DEC_CASES:
            pid = f'decode-{route}-R{R}-nc{nc}-{H}x{W}-off{a_off}-{"aug" if aug else "plain"}-{_dt_id(dt)}'
            out.append(pytest.param(dt, route, R, nc, B, H, W, a_off, extra, aug, id=pid))
    return out


def _ref_decode(f, R, nc, stride, aug):
    """f: (B, 4R+nc, H, W) fp64 -> (B, 4+nc, H*W): DFL softmax expectation per side, dist2bbox (xywh), x stride; sigmoid of the class logits;
    with aug = (s, flip, img_w): xywh / s, x = img_w - x when flipped (nn/tasks.py _descale_pred)."""
    B, _, H, W = f.shape
    box = f[:, :4 * R].reshape(B, 4, R, H * W)
    d = (torch.softmax(box, 2) * torch.arange(R, dtype=torch.float64)[None, None, :, None]).sum(2)      # B, 4, A
    oy, ox = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    ax, ay = ox.reshape(-1) + 0.5, oy.reshape(-1) + 0.5
    x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
    xywh = torch.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], 1) * stride
    if aug is not None:
        xywh = xywh / aug[0]
        if aug[1]:
            xywh[:, 0] = aug[2] - xywh[:, 0]
    return torch.cat([xywh, torch.sigmoid(f[:, 4 * R:].reshape(B, nc, H * W))], 1)


@gpu
@pytest.mark.parametrize('dt,route,R,nc,B,H,W,a_off,extra,aug', _dec_params())
def test_detect_decode(dt, route, R, nc, B, H, W, a_off, extra, aug):
    """detect_decode (plain and aug=) into columns [a_off, a_off + H*W) of a random y[B, 4+nc, a_total]; the other columns stay untouched.  Bin
    logits up to +-80 (one dominant bin per side on some anchors), class ties on some anchors.  The best-class keys of aug= are compared exactly
    against keys recomputed from the STORED scores: first maximal class, key = (~bits(score) << 32) | (anchor * nc + class)."""
    from mgdt_yolo_amd import ops
    assert decode_route(R, nc) == route
    gen = _gen('dec', R, nc, B, H, W, a_off, extra, aug, str(dt))
    no, A = 4 * R + nc, H * W
    f = torch.randn(B, no, H, W, generator=gen, dtype=torch.float64) * 2
    hot = torch.rand(B, 1, H, W, generator=gen) < 0.3
    f[:, :4 * R] = torch.where(hot, f[:, :4 * R] * 40, f[:, :4 * R]).clamp(-80, 80)
    f[:, 4 * R + nc - 1] = f[:, 4 * R]                         # a tie between the first and the last class everywhere ...
    f[:, 4 * R + nc // 2] = torch.where(hot[:, 0], f[:, 4 * R] + 0.0, f[:, 4 * R + nc // 2])   # ... and with a middle one on some anchors
    f = _q(f, dt)
    stride = 8.0
    a_total = a_off + A + extra
    y0 = torch.randn(B, 4 + nc, a_total, generator=gen).float()
    y = y0.to(DEV)
    best0 = torch.randint(0, 2 ** 62, (B, a_total), generator=gen, dtype=torch.int64)
    best = best0.to(DEV)
    ops.detect_decode(_nhwc(f, dt)[0], R, nc, stride, a_off, y, aug=aug, best=best if aug else None)
    got = y.cpu()
    ref = _ref_decode(f, R, nc, stride, aug)
    _close(got[:, :4, a_off:a_off + A], ref[:, :4], F32, 'boxes')
    _close(got[:, 4:, a_off:a_off + A], ref[:, 4:], F32, 'scores')
    assert torch.equal(got[:, :, :a_off], y0[:, :, :a_off]) and torch.equal(got[:, :, a_off + A:], y0[:, :, a_off + A:]), 'other anchors written'
    bk = best.cpu()
    if aug is None:
        assert torch.equal(bk, best0)
        return
    sc = got[:, 4:, a_off:a_off + A].numpy()                                     # B, nc, A as stored (fp32)
    cls = sc.argmax(1)                                                           # first maximal class
    s = np.take_along_axis(sc, cls[:, None], 1)[:, 0]
    anchor = np.arange(a_off, a_off + A, dtype=np.uint64)[None]
    key = ((np.uint64(0xFFFFFFFF) - s.view(np.uint32).astype(np.uint64)) << np.uint64(32)) | (anchor * np.uint64(nc) + cls.astype(np.uint64))
    assert np.array_equal(bk[:, a_off:a_off + A].numpy().view(np.uint64), key), 'best-class keys'
    assert torch.equal(bk[:, :a_off], best0[:, :a_off]) and torch.equal(bk[:, a_off + A:], best0[:, a_off + A:]), 'other keys written'


# ------------------------------------------------------------------------------------------------ copy / add / ew / channel_affine / nc_axpby
@gpu
@pytest.mark.parametrize('src,dst,layout', [
    (s, d, lay) for s in ('f32', 'bf16') for d in ('f32', 'bf16') for lay in ('nhwc', 'nchw_to_nhwc', 'nhwc_to_nchw', 'slice2')] +
    [('u8', d, lay) for d in ('f32', 'bf16') for lay in ('nchw_to_nhwc', 'nhwc')])
def test_copy(src, dst, layout):
    """copy: strided copy with cast, round-to-nearest-even, exact; uint8 is divided by 255 in fp32 first.  The 8-wide vector kernel runs for NHWC views
    on both sides with 8 | c and 16-byte alignment (layout 'nhwc', non-uint8), the scalar one otherwise."""
    from mgdt_yolo_amd import ops
    dts = {'f32': F32, 'bf16': BF16, 'u8': torch.uint8}
    gen = _gen('copy', src, dst, layout)
    B, C, H, W = 2, 16, 7, 5
    if src == 'u8':
        x = torch.randint(0, 256, (B, C, H, W), generator=gen, dtype=torch.uint8)
        ref = _q(x.float() / 255.0, dts[dst])
    else:
        x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64).to(dts[src])
        ref = _q(x.double(), dts[dst])
    off = 2 if layout == 'slice2' else 0
    if layout in ('nchw_to_nhwc',):
        xd = x.to(DEV).contiguous()
    elif src == 'u8':
        xd = _nhwc(x.double(), torch.uint8)[0]
    else:
        xd = _nhwc(x.double(), dts[src], off, 8, gen=gen)[0]
    if layout == 'nhwc_to_nchw':
        big0 = torch.randn(B, C + 8, H, W, generator=gen).to(dts[dst])
        big = big0.to(DEV)
        y = big[:, 4:4 + C]
        ops.copy(xd, y)
        _exact(y, ref, 'y')
        _borders_untouched(big, big0, 4, C)
        return
    y, big, big0 = _out_buf(B, C, H, W, dts[dst], off, 8, gen)
    ops.copy(xd, y)
    _exact(y, ref, 'y')
    _borders_untouched(big, big0, off, C)


def _pair_layouts():
    out = []
    for dt in (F32, BF16):
        for tag, off, C in (('v4', 0, 16), ('v4-slice4', 4, 16), ('scalar-slice2', 2, 16), ('scalar-c6', 0, 6)):
            out.append(pytest.param(dt, off, C, id=f'{tag}-{_dt_id(dt)}'))
    return out


@gpu
@pytest.mark.parametrize('dt,off,C', _pair_layouts())
def test_add(dt, off, C):
    """add: one fp32 add rounded once to the storage dtype - exact (an fp64 sum of two fp32 values of similar size is exact)."""
    from mgdt_yolo_amd import ops
    gen = _gen('add', off, C, str(dt))
    a, b = _rand(gen, 2, C, 9, 7, dt=dt), _rand(gen, 2, C, 9, 7, dt=dt)
    y, big, big0 = _out_buf(2, C, 9, 7, dt, off, 8, gen)
    ops.add(_nhwc(a, dt, off, 8, gen=gen)[0], _nhwc(b, dt, off, 8, gen=gen)[0], out=y)
    _exact(y, _q(_q(a + b, F32), dt), 'y')
    _borders_untouched(big, big0, off, C)


@gpu
@pytest.mark.parametrize('mode', ['mul', 'hsig_grad', 'mul_hsig', 'hsig'])
@pytest.mark.parametrize('dt,off,C', _pair_layouts())
def test_ew(dt, off, C, mode):
    """ew: a*b (exact: one fp32 multiply), a * h_sigmoid'(b), a * h_sigmoid(b), h_sigmoid(b) with h_sigmoid = relu6(x + 3) / 6, b over +-5 so that
    both clamps and the open interval (-3, 3) of the derivative are hit."""
    from mgdt_yolo_amd import ops
    code = {'mul': ops.EW_MUL, 'hsig_grad': ops.EW_HSIG_GRAD, 'mul_hsig': ops.EW_MUL_HSIG, 'hsig': ops.EW_HSIG}[mode]
    gen = _gen('ew', off, C, mode, str(dt))
    a, b = _rand(gen, 2, C, 9, 7, dt=dt), _rand(gen, 2, C, 9, 7, dt=dt, scale=2.5)
    b[0, 0, 0, :4] = torch.tensor([-3.0, 3.0, -3.5, 2.5])
    hs = F.relu6(b + 3) / 6
    ref = {'mul': a * b, 'hsig_grad': a * ((b > -3) & (b < 3)).double() / 6, 'mul_hsig': a * hs, 'hsig': hs}[mode]
    y, big, big0 = _out_buf(2, C, 9, 7, dt, off, 8, gen)
    ops.ew(_nhwc(a, dt, off, 8, gen=gen)[0], _nhwc(b, dt, off, 8, gen=gen)[0], code, out=y)
    if mode == 'mul':
        _exact(y, _q(_q(ref, F32), dt), 'y')
    else:
        _close(y, ref, dt, 'y')
    _borders_untouched(big, big0, off, C)


@gpu
@pytest.mark.parametrize('dt,off,C', _pair_layouts())
def test_channel_affine(dt, off, C):
    """channel_affine: x * scale[n, c] + shift[c], either term optional (the materialised GRN of the ConvNeXt training path)."""
    from mgdt_yolo_amd import ops
    gen = _gen('caff', off, C, str(dt))
    x = _rand(gen, 2, C, 9, 7, dt=dt)
    s, t = torch.randn(2, C, generator=gen).double(), torch.randn(C, generator=gen).double()
    for use_s, use_t in ((True, True), (True, False), (False, True)):
        y, big, big0 = _out_buf(2, C, 9, 7, dt, off, 8, gen)
        ops.channel_affine(_nhwc(x, dt, off, 8, gen=gen)[0], s.float().to(DEV) if use_s else None, t.float().to(DEV) if use_t else None, out=y)
        ref = (x * s[:, :, None, None] if use_s else x) + (t[None, :, None, None] if use_t else 0.0)
        _close(y, ref, dt, f'y scale={use_s} shift={use_t}')
        _borders_untouched(big, big0, off, C)


@gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
@pytest.mark.parametrize('terms', ['a_sa', 'a_sa_b_sb', 'a_b_sb_shift', 'all'])
@pytest.mark.parametrize('off', [pytest.param(0, id='dense'), pytest.param(4, id='slice4')])
def test_nc_axpby(off, terms, dt):
    """nc_axpby: a * sa[n, c] (+ b * sb[n, c]) (+ shift[n, c]) with sa = None meaning 1; output into a channel slice."""
    from mgdt_yolo_amd import ops
    gen = _gen('axpby', off, terms, str(dt))
    B, C, H, W = 2, 12, 7, 5
    a, b = _rand(gen, B, C, H, W, dt=dt), _rand(gen, B, C, H, W, dt=dt)
    sa, sb, sh = (torch.randn(B, C, generator=gen).double() for _ in range(3))
    use_sa, use_b, use_sh = terms != 'a_b_sb_shift', 'b' in terms.split('_') or terms == 'all', 'shift' in terms or terms == 'all'
    ref = a * (sa[:, :, None, None] if use_sa else 1.0)
    if use_b:
        ref = ref + b * sb[:, :, None, None]
    if use_sh:
        ref = ref + sh[:, :, None, None]
    y, big, big0 = _out_buf(B, C, H, W, dt, off, 8, gen)
    dev = lambda t: t.float().to(DEV).contiguous()
    ops.nc_axpby(_nhwc(a, dt, off, 8, gen=gen)[0], dev(sa) if use_sa else None, _nhwc(b, dt, off, 8, gen=gen)[0] if use_b else None,
                 dev(sb) if use_b else None, dev(sh) if use_sh else None, out=y)
    _close(y, ref, dt, 'y')
    _borders_untouched(big, big0, off, C)


# ------------------------------------------------------------------------------------------------ host: the ids name the routes the C dispatch takes
def _ids_of(cases):
    return [(p.id, p.values) for p in cases]


def test_route_predicates():
    """Host only.  Recomputes the LDS and alignment predicates of mgdt_sppf_pool_fwd, detect_decode_launch and mgdt_groupnorm_fwd from each case's
    shape and asserts the route its id names, so that a changed threshold fails an id instead of quietly testing another route."""
    seen = set()
    for pid, (dt, B, C, H, W, kind) in _ids_of(SPPF_CASES):
        route = sppf_route(dt, C, H, W, dt == BF16 and C % 8 == 0)
        assert pid.split('-')[1] == route, (pid, route)
        seen.add(route)
    assert seen == {'two_phase_v8', 'two_phase_v4', 'chained_cg8', 'chained_cg4', 'refused'}
    # the examples the dispatch comment and the issue of this file name: 20x20 two-phase, 27x27 c16 chained cg8, 30x30 chained cg4, 44x44 refused (fp32)
    assert [sppf_route(F32, 16, s, s, False) for s in (20, 26, 27, 30, 44)] == ['two_phase_v4', 'two_phase_v4', 'chained_cg8', 'chained_cg4', 'refused']
    seen = set()
    for p in _dec_params():
        dt, route, R, nc = p.values[:4]
        assert decode_route(R, nc) == route and p.id.split('-')[1] == route, p.id
        seen.add(route)
    assert seen == {'tile', 'tile_big', 'scalar_c4', 'scalar_lds'}
    seen = set()
    for p in _gn_params():
        dt, B, C = p.values[:3]
        assert p.id.split('-')[1] == groupnorm_route(C), p.id
        seen.add(groupnorm_route(C))
    assert seen == {'wide', 'narrow'}
    # the narrow route's longest sequential walk: one thread per channel quad over a row band of H / 16 rows
    assert max(-(-H // 16) * W for (_, B, C, H, W, g, a) in (p.values for p in _gn_params()) if groupnorm_route(C) == 'narrow') >= 1600
    for p in _sprs_params():
        dt, B, g, cw, H, W, tiles, pools, off = p.values
        fast = tiles is not None and spr_fast_prologue(g * cw, g)
        assert p.id.startswith('fast_tiles' if fast else ('general_tiles' if tiles else 'general_splits')), p.id
