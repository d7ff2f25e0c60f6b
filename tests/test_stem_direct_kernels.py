"""The kernels that take the image in, against float64 restatements, per route: mgdt_stem2_fwd (stem_fused.hip), mgdt_conv2d_direct_fwd with its two
kernels and its packer mgdt_conv_pack_direct (conv_direct.hip), mgdt_image_pad4_fwd (pointwise.hip).  The GPU tests are marked `gpu`; the rest runs
anywhere.

Routes.  Every GPU case names the route it is there for in its id; test_census_* holds each id to the library's host-side queries
(mgdt_stem2_route, mgdt_conv2d_direct_route) on views of the same sizes, strides and offsets, so a dispatch change that moves a case fails the census
instead of shrinking coverage.  The GPU tests ask the same queries about the device views they launch on.

Bounds.  kernel_ref._close of the output dtype everywhere, _exact where the operation is a copy (image_pad4).  conv2d_direct and the packer round once
(the store; fp32 FMAs before it).  stem2 rounds y0 to bf16 mid-kernel: a correct fp32 kernel may round a y0 element next to a rounding boundary to the
other neighbour than the float64 reference.  test_fp32_restatement_inside_the_bound shows on the host that the plain bound leaves room for that (the
fp32 evaluation of the restatement uses at most 0.75 of it over the GPU cases); on an MI355X the kernel used at most 0.75 as well, so the bound carries
no flip allowance.

Inputs and outputs are slices of wider buffers pre-filled with random values; what lies outside the output view must come back bit-identical.  The
weights are ConvP draws with BatchNorm (never a model's): gains 1 and 3 for stem2, so that pre-activations reach about +-10."""
import collections
import functools

import numpy as np
import pytest
import torch

from kernel_ref import (BF16, DEV, F32, ConvP, _borders_untouched, _check, _exact, _gen, ref_direct, ref_pack_direct, ref_stem2, u8_unit)

gpu = pytest.mark.gpu
U8 = torch.uint8
CUS = 256                       # compute units the census plans for (MI355X)
DT = {'u8': U8, 'bf16': BF16, 'f32': F32}
OK, BAD_SHAPE, BAD_DTYPE = 0, -1, -2            # mgdt_status


def cdiv(a, b):
    return (a + b - 1) // b


def _buf(b, c, h, w, layout, dt, gen):
    """CPU (b, c, h, w) tensor with the strides of `layout` ('nchw' / 'nhwc'), random values of dtype dt (images: mean 0.5, negative values and values
    above 1 included; uint8: all of 0..255)."""
    if dt == U8:
        vals = torch.randint(0, 256, (b, c, h, w), generator=gen, dtype=U8)
    else:
        vals = (torch.randn(b, c, h, w, generator=gen) * 0.7 + 0.5).to(dt)
    strides = (c * h * w, h * w, w, 1) if layout == 'nchw' else (h * w * c, 1, w * c, c)
    t = torch.empty_strided((b, c, h, w), strides, dtype=dt)
    t.copy_(vals)
    return t


def _place(t, device):
    """The same sizes and strides on `device` ('meta': no values)."""
    out = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=device)
    if device != 'meta':
        out.copy_(t)
    return out


def _values(t):
    """fp64 values of a stored tensor as the kernels read it."""
    return u8_unit(t) if t.dtype == U8 else t.double()


# ================================================================================================ stem2
S2 = collections.namedtuple('S2', 'note loader xdt b h w layout wgs gain')
S2_OFF, S2_EXTRA, S2_ROW0, S2_ROWX = 8, 24, 1, 2          # the output view: channels [8, 40) of 64, rows [1, 1 + H1) of H1 + 3
S2_SIZES = [(1, 1, 1, '1-tile-1px'), (1, 1, 8, '1-tile-W-8-is-0'), (1, 8, 8, '1-tile-W-8-is-0'), (1, 29, 61, '1-tile-H0-W0-odd'),
            (1, 32, 64, 'exactly-1-tile'), (1, 33, 65, '2x2-tiles-last-1-row-1-col'), (1, 35, 72, '2x2-tiles-partial'),
            (3, 40, 136, '18-tiles-ranges-cross-images')]


def _s2_loader(xdt, h, w, layout):
    return 'fast' if xdt == 'bf16' and layout == 'nchw' and w % 8 == 0 else 'generic'


S2_CASES = [S2(note, _s2_loader(xdt, h, w, 'nchw'), xdt, b, h, w, 'nchw', None, gain)
            for (b, h, w, note) in S2_SIZES for xdt in ('u8', 'bf16', 'f32') for gain in (1, 3)]
S2_LAYOUTS = [('channels-last-xsw3', 'f32', 2, 33, 40, 'nhwc'), ('channels-last-xsw3', 'bf16', 2, 33, 40, 'nhwc'), ('hwc-permuted-xsw3', 'u8', 2, 33, 40, 'nhwc'),
              ('crop-at-odd-column', 'bf16', 2, 35, 72, 'crop')]
S2_CASES += [S2(note, 'generic', xdt, b, h, w, layout, None, gain) for (note, xdt, b, h, w, layout) in S2_LAYOUTS for gain in (1, 3)]
# MGDT_STEM_WGS=2: two workgroups walk every tile (the next patch requested one tile ahead on the fast loader)
S2_CASES += [S2(note + '-wgs2', _s2_loader(xdt, h, w, 'nchw'), xdt, b, h, w, 'nchw', '2', 3)
             for (b, h, w, note) in S2_SIZES[5:] for xdt in ('u8', 'bf16', 'f32')]
S2_CASES += [S2(note + '-wgs2', 'generic', xdt, b, h, w, layout, '2', 3) for (note, xdt, b, h, w, layout) in S2_LAYOUTS]


def _s2_id(c):
    return f'{c.loader}-{c.xdt}-{c.b}x{c.h}x{c.w}-{c.layout}-gain{c.gain}-{c.note}'


s2_params = [pytest.param(c, id=_s2_id(c)) for c in S2_CASES]


def _s2_hw(h, w):
    h0, w0 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h0, w0, (h0 - 1) // 2 + 1, (w0 - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def s2_weights(gain):
    gen = _gen('stem2 weights', gain)
    return ConvP(gen, 16, 3, 3, bn=True, bias=False, gain=gain), ConvP(gen, 32, 16, 3, bn=True, bias=False, gain=gain)


@functools.lru_cache(maxsize=None)
def s2_image(xdt, b, h, w, layout):
    """(CPU buffer, function buffer -> image view)."""
    gen = _gen('stem2 image', xdt, b, h, w, layout)
    if layout == 'crop':
        big = _buf(b, 3, h + 5, w + 16, 'nchw', DT[xdt], gen)
        cut = lambda t: t[:, :, 2:2 + h, 3:3 + w]
    else:
        big = _buf(b, 3, h, w, layout, DT[xdt], gen)
        cut = lambda t: t
    if xdt == 'u8':
        flat = cut(big)
        flat[0, 0, 0, 0], flat[-1, -1, -1, -1] = 0, 255
        if h * w > 1:
            flat[0, 1, 0, 0], flat[0, 0, -1, -1] = 255, 0
    return big, cut


@functools.lru_cache(maxsize=None)
def s2_ref(xdt, b, h, w, layout, gain):
    big, cut = s2_image(xdt, b, h, w, layout)
    return ref_stem2(_values(cut(big)), *s2_weights(gain))


def _s2_out(c, device):
    """(output view, whole buffer, its CPU original)."""
    _, _, h1, w1 = _s2_hw(c.h, c.w)
    big0 = _buf(c.b, 32 + S2_OFF + S2_EXTRA, h1 + S2_ROW0 + S2_ROWX, w1, 'nhwc', BF16, _gen('stem2 out', c))
    big = _place(big0, device)
    return big[:, S2_OFF:S2_OFF + 32, S2_ROW0:S2_ROW0 + h1], big, big0


def _s2_expected(c):
    _, _, h1, w1 = _s2_hw(c.h, c.w)
    tx, ty = cdiv(w1, 16), cdiv(h1, 8)
    tiles = c.b * tx * ty
    grid = min(tiles, 3 * CUS, int(c.wgs) if c.wgs else tiles)
    return dict(loader=c.loader, tiles_x=tx, tiles_y=ty, tiles=tiles, grid=grid, per_xcd=cdiv(tiles, min(grid, 8)))


def _set_wgs(monkeypatch, wgs):
    if wgs is None:
        monkeypatch.delenv('MGDT_STEM_WGS', raising=False)
    else:
        monkeypatch.setenv('MGDT_STEM_WGS', wgs)


def test_census_stem2(monkeypatch):
    """Every stem2 id against mgdt_stem2_route on views of the case's sizes, strides and offsets: loader, tile grid, workgroups, XCD ranges.  Both
    loaders, one / four / eighteen tiles, a workgroup that walks nine tiles and the three image dtypes must all be present."""
    from mgdt_yolo_amd import ops
    seen = collections.Counter()
    for c in S2_CASES:
        _set_wgs(monkeypatch, c.wgs)
        big, cut = s2_image(c.xdt, c.b, c.h, c.w, c.layout)
        r = ops.stem2_route(cut(_place(big, 'meta')), _s2_out(c, 'meta')[0], CUS)
        assert r == _s2_expected(c), (_s2_id(c), r)
        seen[(r['loader'], c.xdt)] += 1
        seen[('tiles', r['tiles'])] += 1
        seen[('walk', cdiv(r['tiles'], r['grid']))] += 1
    for key in [('fast', 'bf16'), ('generic', 'bf16'), ('generic', 'u8'), ('generic', 'f32'), ('tiles', 1), ('tiles', 4), ('tiles', 18), ('walk', 2), ('walk', 9)]:
        assert seen[key] > 0, key
    assert len({_s2_id(c) for c in S2_CASES}) == len(S2_CASES)


def test_model_maps_keep_the_fast_routes():
    """The model's own launches: a dense bf16 640 x 640 batch takes stem2's fast loader, and the stem specialisation of the direct convolution keeps
    every dense NHWC map of 16 k channels, in bf16 and fp32."""
    from mgdt_yolo_amd import ops
    x = torch.empty(32, 3, 640, 640, dtype=BF16, device='meta')
    y = torch.empty(32, 32, 160, 160, dtype=BF16, device='meta', memory_format=torch.channels_last)
    r = ops.stem2_route(x, y, CUS)
    assert r['loader'] == 'fast' and r['tiles'] == 32 * 10 * 20 and r['grid'] == 3 * CUS
    for cout in (16, 32, 48, 64, 80):
        for xdt, ydt in ((U8, BF16), (U8, F32), (BF16, BF16), (F32, BF16), (F32, F32)):
            x = torch.empty(2, 3, 64, 64, dtype=xdt, device='meta')
            y = torch.empty(2, cout, 32, 32, dtype=ydt, device='meta', memory_format=torch.channels_last)
            assert ops.conv2d_direct_route(x, y, 3, 2) == dict(family='stem', gx=cdiv(2 * 32 * 32, 256), gy=cout // 16, status=OK), (cout, xdt, ydt)


def test_uint8_table_rounding_hides_the_form_of_the_division():
    """stem2 rounds the table entry fp32(v) / 255 to bf16 when it reaches LDS, and all 256 entries round to the same bf16 value when the division is
    replaced by a multiplication with fp32(1 / 255), although 126 of them differ in fp32: no stem2 case can tell the two forms apart (a mutation trial
    confirmed it).  Where the fp32 value is kept, image_pad4's bit-equal uint8 -> fp32 cases can, and do."""
    v = np.arange(256, dtype=np.float32)
    div, mul = v / np.float32(255), v * (np.float32(1) / np.float32(255))
    assert (div != mul).sum() == 126
    assert torch.equal(torch.from_numpy(div).to(BF16), torch.from_numpy(mul).to(BF16))
    assert np.array_equal(div, u8_unit(torch.arange(256, dtype=U8)).numpy().astype(np.float32))


def _s2_refusals(device):
    """(what, x, x dtype code or None, y) that mgdt_stem2_fwd refuses before any launch."""
    mk = lambda *shape, dt=BF16: _place(_buf(*shape, 'nhwc' if dt == BF16 and shape[1] != 3 else 'nchw', dt, _gen('stem2 refusal', shape)), device)
    y64 = mk(1, 64, 8, 16)
    return [('x.c != 3', mk(1, 4, 32, 64, dt=F32), None, y64[:, 8:40]),
            ('y.c != 32', mk(1, 3, 32, 64, dt=F32), None, y64[:, 8:56]),
            ('y at a 4-byte-aligned pointer', mk(1, 3, 32, 64, dt=F32), None, y64[:, 2:34]),
            ('wrong y shape', mk(1, 3, 32, 64, dt=F32), None, mk(1, 64, 8, 15)[:, 8:40]),
            ('unknown dtype', mk(1, 3, 32, 64, dt=F32), 5, y64[:, 8:40])]


def test_stem2_refusals_reported_by_the_route():
    from mgdt_yolo_amd import ops
    for what, x, code, y in _s2_refusals('meta'):
        r = ops.stem2_route(x, y, CUS, x_dtype=code)
        assert r['loader'] == 'refused' and r['status'] == (BAD_DTYPE if code is not None else BAD_SHAPE), (what, r)


def test_fp32_restatement_inside_the_bound():
    """For every GPU case of stem2 and conv2d_direct: the restatement evaluated in fp32 and rounded to the output dtype stays inside the bound of its
    float64 evaluation - the bound leaves room for a correct fp32 kernel (stem2: a y0 element rounded to the other bf16 neighbour included)."""
    for key in sorted({(c.xdt, c.b, c.h, c.w, c.layout, c.gain) for c in S2_CASES}):
        big, cut = s2_image(*key[:5])
        y32 = ref_stem2(_values(cut(big)), *s2_weights(key[5]), dt=F32).to(BF16)
        _check(y32, s2_ref(*key), BF16, f'stem2 fp32 restatement {key}')
    for c in D_CASES:
        d = d_case(c)
        y32 = ref_direct(d['xv'], d['cp'], c.s, c.act, c.g, dt=F32).to(DT[c.ydt])
        _check(y32, d['ref'], DT[c.ydt], f'direct fp32 restatement {_d_id(c)}')


@gpu
@pytest.mark.parametrize('c', s2_params)
def test_stem2(c, monkeypatch):
    from mgdt_yolo_amd import ops
    cp0, cp1 = s2_weights(c.gain)
    w0, _, bn0 = cp0.dev_args()
    pk0, pk1 = ops.PackedStem2(w0, bn0), cp1.pack()
    big, cut = s2_image(c.xdt, c.b, c.h, c.w, c.layout)
    x = cut(_place(big, DEV))
    y, ybig, ybig0 = _s2_out(c, DEV)
    _set_wgs(monkeypatch, c.wgs)
    r = ops.stem2_route(x, y, CUS)
    assert r == _s2_expected(c), r
    ops._launch('stem2_fwd', 'mgdt_stem2_fwd', ops.vp(x), ops.U8 if x.dtype == U8 else ops.dtype_code(x.dtype), ops.ptr(pk0.blob), ops.ptr(pk0.bias),
                ops.ptr(pk1.w), ops.ptr(pk1.bias), ops.vp(y), ops.stream())
    torch.cuda.synchronize()
    got = ybig.cpu()
    mask = torch.ones(ybig0.shape, dtype=torch.bool)
    mask[:, S2_OFF:S2_OFF + 32, S2_ROW0:S2_ROW0 + y.shape[2]] = False
    assert torch.equal(got[mask], ybig0[mask]), 'wrote outside the output view'
    _check(got[:, S2_OFF:S2_OFF + 32, S2_ROW0:S2_ROW0 + y.shape[2]], s2_ref(c.xdt, c.b, c.h, c.w, c.layout, c.gain), BF16, 'stem2 ' + _s2_id(c))


@gpu
def test_stem2_refuses_before_any_launch():
    from mgdt_yolo_amd import ops
    cp0, cp1 = s2_weights(1)
    w0, _, bn0 = cp0.dev_args()
    pk0, pk1 = ops.PackedStem2(w0, bn0), cp1.pack()
    for what, x, code, y in _s2_refusals(DEV):
        base = y._base if y._base is not None else y
        before = base.cpu()
        if code is None:
            code = ops.dtype_code(x.dtype)
        with pytest.raises(RuntimeError):
            ops._launch('stem2_fwd', 'mgdt_stem2_fwd', ops.vp(x), code, ops.ptr(pk0.blob), ops.ptr(pk0.bias), ops.ptr(pk1.w), ops.ptr(pk1.bias), ops.vp(y),
                        ops.stream())
        torch.cuda.synchronize()
        assert torch.equal(base.cpu(), before), what


# ================================================================================================ conv2d_direct
# xl / yl: layout of the buffers; the views are the channel slices [xo, xo + cin) of xo + cin + xe channels and [yo, yo + cout) of yo + cout + ye
D = collections.namedtuple('D', 'note route xdt ydt cin cout k s g act b h w xl xo xe yl yo ye bn')


def _d(note, route, xdt, ydt, cin, cout, k, s, g, act, bhw, xl='nhwc', xo=0, xe=0, yl='nhwc', yo=0, ye=0, bn='bn'):
    return D(note, route, xdt, ydt, cin, cout, k, s, g, act, *bhw, xl, xo, xe, yl, yo, ye, bn)


BIG, MID, ONE = (2, 17, 19), (1, 5, 7), (1, 1, 1)         # 2x17x19 at stride 1: M = 646, three pixel blocks, the last partial
D_CASES = [
    # ---- the stem specialisation: every dtype pair, cin 1 / 3 / 4, cout 16 / 48, stride 1 / 2 / 3, four activations, three maps, both image layouts
    _d('nchw-image-in-place', 'stem', 'u8', 'bf16', 3, 16, 3, 2, 1, 'silu', BIG, xl='nchw'),
    _d('hwc-permuted-image-y-slice-at-16B', 'stem', 'u8', 'f32', 3, 48, 3, 2, 1, 'silu', BIG, yo=4, ye=12),
    _d('M646-3-pixel-blocks-y-slice-at-16B', 'stem', 'bf16', 'bf16', 3, 16, 3, 1, 1, 'relu', BIG, xl='nchw', xo=1, xe=1, yo=8, ye=8),
    _d('M646-gy3-channels-last-image', 'stem', 'f32', 'bf16', 4, 48, 3, 1, 1, 'gelu', BIG, yo=8, ye=8),
    _d('nchw-image-slice', 'stem', 'f32', 'f32', 1, 16, 3, 3, 1, 'none', BIG, xl='nchw', xo=1, xe=1),
    _d('M646-gy3', 'stem', 'u8', 'bf16', 3, 48, 3, 1, 1, 'gelu', BIG, xl='nchw', bn='both'),
    _d('map-1x1', 'stem', 'u8', 'bf16', 1, 16, 3, 1, 1, 'none', ONE, xl='nchw'),
    _d('map-1x1', 'stem', 'f32', 'bf16', 3, 16, 3, 2, 1, 'silu', ONE, xl='nchw'),
    _d('map-5x7-y-slice-at-16B', 'stem', 'f32', 'f32', 3, 48, 3, 2, 1, 'silu', MID, xl='nchw', yo=4, ye=12, bn='bias'),
    _d('map-5x7-channels-last-image', 'stem', 'bf16', 'bf16', 4, 48, 3, 3, 1, 'silu', MID),
    _d('map-5x7', 'stem', 'u8', 'f32', 4, 16, 3, 3, 1, 'relu', MID, xl='nchw'),
    _d('map-5x7', 'stem', 'bf16', 'bf16', 1, 16, 3, 2, 1, 'none', MID, xl='nchw', bn='none'),
    # ---- views the stem specialisation must leave to the generic kernel
    _d('bf16-to-f32-pair-not-instantiated', 'generic', 'bf16', 'f32', 3, 16, 3, 2, 1, 'silu', BIG, xl='nchw'),
    _d('cout40-not-16k', 'generic', 'f32', 'f32', 3, 40, 3, 2, 1, 'silu', BIG, xl='nchw'),
    _d('y-slice-at-channel-4-8B-aligned', 'generic', 'f32', 'bf16', 3, 16, 3, 2, 1, 'silu', BIG, xl='nchw', yo=4, ye=12),
    _d('y-16-of-28-channels-at-8-odd-pixels-8B-aligned', 'generic', 'bf16', 'bf16', 3, 16, 3, 1, 1, 'silu', BIG, xl='nchw', yo=8, ye=4),
    _d('y-16-of-28-channels-at-8-odd-pixels-8B-aligned', 'generic', 'f32', 'bf16', 3, 16, 3, 2, 1, 'silu', BIG, yo=8, ye=4),
    _d('k1-cin3', 'generic', 'f32', 'f32', 3, 16, 1, 1, 1, 'none', MID, xl='nchw'),
    # ---- generic kernel, groups = 1: cin 5 / 12, partial last cout block, k 1 / 3 / 5 / 7, stride 1 / 2 / 3, four dtype pairs, NCHW output
    _d('cout10-one-partial-block', 'generic', 'f32', 'f32', 5, 10, 1, 1, 1, 'none', (2, 9, 11), xo=3, xe=2, yo=3, ye=1),
    _d('cout17-block-of-1', 'generic', 'f32', 'bf16', 12, 17, 3, 2, 1, 'silu', (2, 9, 11), xo=4, xe=0, yo=1, ye=2),
    _d('cout33-block-of-1', 'generic', 'bf16', 'bf16', 5, 33, 5, 3, 1, 'relu', (2, 9, 11), xo=1, xe=2, yo=0, ye=3),
    _d('cout33-nchw-output', 'generic', 'bf16', 'f32', 12, 33, 7, 1, 1, 'gelu', (2, 9, 11), yl='nchw', yo=2, ye=1, bn='both'),
    _d('map-1x1-k7-all-taps-but-one-outside', 'generic', 'f32', 'f32', 12, 17, 7, 2, 1, 'silu', ONE, yo=1, ye=2),
    _d('map-1x1-nchw-output', 'generic', 'bf16', 'bf16', 5, 10, 3, 1, 1, 'silu', ONE, yl='nchw', yo=1, ye=1, bn='bias'),
    _d('nchw-input-stride3', 'generic', 'f32', 'bf16', 5, 17, 5, 3, 1, 'none', (2, 9, 11), xl='nchw', xo=1, xe=1, yl='nchw', bn='none'),
    # ---- grouped branch
    _d('depthwise', 'generic', 'f32', 'f32', 8, 8, 3, 1, 8, 'silu', (2, 9, 11), xo=2, xe=2, yo=2, ye=2),
    _d('depthwise', 'generic', 'bf16', 'bf16', 24, 24, 5, 2, 24, 'silu', (2, 9, 11), xo=8, xe=0, yo=0, ye=8),
    _d('depthwise', 'generic', 'bf16', 'f32', 24, 24, 7, 1, 24, 'none', (2, 9, 11)),
    _d('depthwise', 'generic', 'f32', 'bf16', 24, 24, 3, 2, 24, 'relu', (2, 9, 11), yl='nchw'),
    _d('depthwise', 'generic', 'bf16', 'bf16', 8, 8, 5, 1, 8, 'gelu', (2, 9, 11), bn='both'),
    _d('depthwise-map-1x1', 'generic', 'f32', 'f32', 8, 8, 7, 2, 8, 'silu', ONE),
    _d('cin_g3-cout_g5-block-spans-2-groups', 'generic', 'f32', 'f32', 6, 10, 3, 1, 2, 'silu', (2, 9, 11), xo=1, xe=1, yo=1, ye=1),
    _d('cout_g16-blocks-inside-a-group', 'generic', 'bf16', 'bf16', 6, 48, 3, 2, 3, 'silu', (2, 9, 11)),
    _d('cout_g20-blocks-across-two-groups', 'generic', 'f32', 'bf16', 9, 60, 3, 1, 3, 'silu', (2, 9, 11), yo=2, ye=2),
    _d('cin_g4-cout_g2-block-spans-4-groups', 'generic', 'bf16', 'f32', 16, 8, 5, 1, 4, 'none', (2, 9, 11), bn='bias'),
]


def _d_id(c):
    return (f'{c.route}-{c.xdt}-{c.ydt}-cin{c.cin}-cout{c.cout}-k{c.k}s{c.s}g{c.g}-{c.act}-{c.b}x{c.h}x{c.w}-x{c.xl}{c.xo}of{c.xo + c.cin + c.xe}'
            f'-y{c.yl}{c.yo}of{c.yo + c.cout + c.ye}-{c.bn}-{c.note}')


d_params = [pytest.param(c, id=_d_id(c)) for c in D_CASES]


def _d_out_hw(c):
    p = c.k // 2
    return (c.h + 2 * p - c.k) // c.s + 1, (c.w + 2 * p - c.k) // c.s + 1


@functools.lru_cache(maxsize=None)
def d_case(c):
    """Buffers, parameters and float64 reference of one conv2d_direct case: computed once, shared by the host-only and the GPU tests."""
    gen = _gen('direct', c)
    xbig = _buf(c.b, c.xo + c.cin + c.xe, c.h, c.w, c.xl, DT[c.xdt], gen)
    if c.xdt == 'u8':
        xv = xbig[:, c.xo:c.xo + c.cin]
        xv[0, 0, 0, 0], xv[-1, -1, -1, -1] = 255, 0
    cp = ConvP(gen, c.cout, c.cin // c.g, c.k, bn=c.bn in ('bn', 'both'), bias=c.bn in ('bias', 'both'), gain=2.0, dt=F32, wrep=F32)
    ho, wo = _d_out_hw(c)
    ybig0 = _buf(c.b, c.yo + c.cout + c.ye, ho, wo, c.yl, DT[c.ydt], gen)
    xv = _values(xbig[:, c.xo:c.xo + c.cin])
    return dict(xbig=xbig, ybig0=ybig0, cp=cp, xv=xv, ref=ref_direct(xv, cp, c.s, c.act, c.g))


def _d_views(c, device):
    d = d_case(c)
    ybig = _place(d['ybig0'], device)
    return _place(d['xbig'], device)[:, c.xo:c.xo + c.cin], ybig[:, c.yo:c.yo + c.cout], ybig


def _d_expected(c):
    ho, wo = _d_out_hw(c)
    return dict(family=c.route, gx=cdiv(c.b * ho * wo, 256), gy=c.cout // 16 if c.route == 'stem' else cdiv(c.cout, 16), status=OK)


def test_census_conv2d_direct():
    """Every conv2d_direct id against mgdt_conv2d_direct_route on views of the case's sizes, strides and offsets: kernel family and grid.  What the
    module is there for must be present: each instantiated dtype pair on each kernel, three pixel blocks, a partial cout block, NCHW output, a block
    of 16 output channels that spans two groups."""
    from mgdt_yolo_amd import ops
    seen = collections.Counter()
    for c in D_CASES:
        x, y, _ = _d_views(c, 'meta')
        r = ops.conv2d_direct_route(x, y, c.k, c.s, c.g)
        assert r == _d_expected(c), (_d_id(c), r)
        seen[(c.route, c.xdt, c.ydt)] += 1
        seen[('gx', r['gx'])] += 1
        seen[('partial-block', c.route, c.cout % 16 != 0)] += 1
        seen[('y', c.yl)] += 1
        seen[('k', c.k)] += 1
        seen[('s', c.s)] += 1
        if c.g > 1:
            cg = c.cout // c.g
            seen[('grouped', 'dw' if c.g == c.cin == c.cout else 'span' if any(b // cg != min(b + 15, c.cout - 1) // cg for b in range(0, c.cout, 16)) else 'inside')] += 1
    for pair in (('u8', 'bf16'), ('u8', 'f32'), ('bf16', 'bf16'), ('f32', 'bf16'), ('f32', 'f32')):
        assert seen[('stem',) + pair] > 0, pair
    for pair in (('bf16', 'bf16'), ('bf16', 'f32'), ('f32', 'bf16'), ('f32', 'f32')):
        assert seen[('generic',) + pair] > 0, pair
    for key in [('gx', 1), ('gx', 3), ('partial-block', 'generic', True), ('y', 'nchw'), ('grouped', 'dw'), ('grouped', 'span'), ('grouped', 'inside')] + \
            [('k', k) for k in (1, 3, 5, 7)] + [('s', s) for s in (1, 2, 3)]:
        assert seen[key] > 0, key
    assert len({_d_id(c) for c in D_CASES}) == len(D_CASES)


def test_stem_predicate_needs_16_byte_aligned_bf16_pixels():
    """The stem kernel stores bf16x8 (16 bytes) per half pixel.  A 16-channel slice at channel 8 of a 28-channel bf16 buffer has a 16-byte aligned
    pointer and a pixel stride of 56 bytes: the route must be the generic kernel; the same slice of a 32-channel buffer, and the fp32 view with strides
    that are multiples of 4 elements, keep the stem kernel."""
    from mgdt_yolo_amd import ops
    x = torch.empty(2, 3, 17, 19, dtype=F32, device='meta')
    route = lambda ctot, off, dt: ops.conv2d_direct_route(x, torch.empty(2, ctot, 17, 19, dtype=dt, device='meta', memory_format=torch.channels_last)[:, off:off + 16],
                                                          3, 1)['family']
    assert route(28, 8, BF16) == 'generic' and route(32, 8, BF16) == 'stem' and route(24, 8, BF16) == 'stem' and route(36, 8, BF16) == 'generic'
    assert route(28, 8, F32) == 'stem' and route(28, 4, F32) == 'stem' and route(30, 4, F32) == 'generic' and route(32, 4, BF16) == 'generic'


def _d_refusals(device):
    """(what, x, y, cin_g, k, groups, status) that mgdt_conv2d_direct_fwd refuses before any launch."""
    mk = lambda c, dt, layout='nhwc': _place(_buf(1, c, 5, 7, layout, dt, _gen('direct refusal', c, str(dt))), device)
    return [('uint8 input, cout 40', mk(3, U8, 'nchw'), mk(40, F32), 3, 3, 1, BAD_DTYPE),
            ('uint8 input, k 5', mk(3, U8, 'nchw'), mk(16, F32), 3, 5, 1, BAD_DTYPE),
            ('uint8 input, cin 5', mk(5, U8, 'nchw'), mk(16, F32), 5, 3, 1, BAD_DTYPE),
            ('even k', mk(8, F32), mk(16, F32), 8, 2, 1, BAD_SHAPE),
            ('even k', mk(8, F32), mk(16, F32), 8, 4, 1, BAD_SHAPE),
            ('k = 9', mk(8, F32), mk(16, F32), 8, 9, 1, BAD_SHAPE),
            ('cin % groups != 0', mk(5, F32), mk(16, F32), 2, 3, 2, BAD_SHAPE),
            ('cout % groups != 0', mk(6, F32), mk(16, F32), 2, 3, 3, BAD_SHAPE),
            ('wrong y shape', mk(8, F32), mk(16, F32)[:, :, :4], 8, 3, 1, BAD_SHAPE)]


def test_conv2d_direct_refusals_reported_by_the_route():
    from mgdt_yolo_amd import ops
    for what, x, y, _, k, g, status in _d_refusals('meta'):
        assert ops.conv2d_direct_route(x, y, k, 1, g) == dict(family='refused', gx=0, gy=0, status=status), what
    x, y = torch.empty(1, 3, 5, 7, device='meta'), torch.empty(1, 16, 5, 7, device='meta', memory_format=torch.channels_last)
    assert ops.conv2d_direct_route(x, y, 3, 1, dtype=5)['status'] == BAD_DTYPE and ops.conv2d_direct_route(x, y, 3, 1, x_dtype=5)['status'] == BAD_DTYPE


def _acts():
    from mgdt_yolo_amd import ops
    return {'none': ops.ACT_NONE, 'silu': ops.ACT_SILU, 'relu': ops.ACT_RELU, 'gelu': ops.ACT_GELU}


def _pack_direct(cp, groups=1):
    from mgdt_yolo_amd import ops
    w, cb, bn = cp.dev_args()
    return ops.PackedConv(w, cb, bn, cp.k, F32, direct=True, groups=groups)


@gpu
@pytest.mark.parametrize('c', d_params)
def test_conv2d_direct(c):
    from mgdt_yolo_amd import ops
    d = d_case(c)
    x, y, ybig = _d_views(c, DEV)
    r = ops.conv2d_direct_route(x, y, c.k, c.s, c.g)
    assert r == _d_expected(c), r
    ops.conv2d(x, _pack_direct(d['cp'], c.g), c.s, _acts()[c.act], out=y)
    torch.cuda.synchronize()
    _borders_untouched(ybig, d['ybig0'], c.yo, c.cout)
    _check(y, d['ref'], DT[c.ydt], 'direct ' + _d_id(c))


@gpu
def test_conv2d_direct_refuses_before_any_launch():
    from mgdt_yolo_amd import ops
    for what, x, y, cin_g, k, g, _ in _d_refusals(DEV):
        base = y._base if y._base is not None else y
        before = base.cpu()
        pk = _pack_direct(ConvP(_gen('direct refusal weights', what), y.shape[1], cin_g, k, dt=F32, wrep=F32), g)
        with pytest.raises(RuntimeError):
            ops._launch('conv2d_direct_fwd', 'mgdt_conv2d_direct_fwd', ops.vp(x), ops.U8 if x.dtype == U8 else ops.dtype_code(x.dtype), ops.ptr(pk.w),
                        ops.ptr(pk.bias), k, 1, g, ops.ACT_SILU, ops.vp(y), ops.dtype_code(y.dtype), ops.stream())
        torch.cuda.synchronize()
        assert torch.equal(base.cpu(), before), what


# ================================================================================================ conv_pack_direct
# (cout, cin_g, k): cout 300 with one weight per output channel - the weight part fills two blocks of which the second also holds the bias of
# channels 256..299
PACK_SHAPES = [(10, 3, 3), (17, 5, 5), (33, 2, 7), (300, 1, 1)]


@gpu
@pytest.mark.parametrize('fold', ['bn', 'bias', 'both', 'none'])
@pytest.mark.parametrize('shape', PACK_SHAPES, ids=lambda s: f'cout{s[0]}-cin_g{s[1]}-k{s[2]}')
def test_conv_pack_direct(shape, fold):
    """The panel [(tap * cin_g + ci) * cout + co] and the bias against the float64 fold, at the fp32 bound; the weights are all distinct, so an element
    in the wrong place cannot pass."""
    cout, cin_g, k = shape
    cp = ConvP(_gen('pack_direct', shape, fold), cout, cin_g, k, bn=fold in ('bn', 'both'), bias=fold in ('bias', 'both'), dt=F32, wrep=F32)
    n = cp.w.numel()                                  # a permutation of n distinct multiples of 2^-10: random draws of a few thousand fp32 values collide
    cp.w = ((torch.randperm(n, generator=_gen('pack_direct weights', shape, fold)).float() - n // 2 + 0.25) / 1024).view_as(cp.w)
    assert cp.w.unique().numel() == n
    panel, bias = ref_pack_direct(cp)
    assert panel.unique().numel() == panel.numel()
    pk = _pack_direct(cp)
    torch.cuda.synchronize()
    assert pk.w.numel() == panel.numel() and pk.bias.numel() == cout
    what = f'pack_direct cout{cout}-cin_g{cin_g}-k{k}-{fold}'
    _check(pk.w, panel, F32, what + ' panel')
    if fold == 'none':
        _exact(pk.bias, bias, what + ' bias')
    else:
        _check(pk.bias, bias, F32, what + ' bias')


# ================================================================================================ image_pad4
PAD_PAIRS = [('u8', 'bf16'), ('u8', 'f32'), ('f32', 'f32'), ('f32', 'bf16'), ('bf16', 'bf16')]


def _pad4_ref(x, ydt):
    """(b, 4, h, w) of dtype ydt: uint8 as np.float32(v) / np.float32(255), the cast otherwise, rounded to nearest even when ydt is bf16; channels at
    and above C exactly 0."""
    b, c, h, w = x.shape
    v = x.numpy().astype(np.float32) / np.float32(255) if x.dtype == U8 else x.float().numpy()
    out = torch.zeros(b, 4, h, w, dtype=F32)
    out[:, :c] = torch.from_numpy(np.ascontiguousarray(v))
    return out.to(ydt)


def _pad4_run(x_cpu, C, ydt, key):
    """x = the first C channels of the 3-channel buffer x_cpu; y = channels [4, 8) of an 8-channel NHWC buffer.  Returns y's values."""
    from mgdt_yolo_amd import ops
    b, _, h, w = x_cpu.shape
    ybig0 = _buf(b, 8, h, w, 'nhwc', ydt, _gen('pad4 out', key))
    ybig = _place(ybig0, DEV)
    y = ybig[:, 4:8]
    x = _place(x_cpu, DEV)[:, :C]
    ops._launch('image_pad4_fwd', 'mgdt_image_pad4_fwd', ops.vp(x), ops.U8 if x.dtype == U8 else ops.dtype_code(x.dtype), ops.vp(y), ops.dtype_code(ydt),
                ops.stream())
    torch.cuda.synchronize()
    got = ybig.cpu()
    assert torch.equal(got[:, :4], ybig0[:, :4]), 'channels 0..3 of the buffer written'
    return got[:, 4:8]


@gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('pair', PAD_PAIRS, ids=lambda p: f'{p[0]}-{p[1]}')
def test_image_pad4(pair, C, layout):
    """Bit-equal to the cast (uint8: all 256 values, the fp32 division by 255 and its round-to-nearest-even); the channels at and above C exactly 0,
    though the image is the first C channels of a 3-channel buffer of random values.  'nhwc' of a uint8 image is the HWC array of an image reader,
    permuted."""
    xdt, ydt = DT[pair[0]], DT[pair[1]]
    gen = _gen('pad4', pair, C, layout)
    if xdt == U8 and layout == 'nhwc':
        full = torch.randint(0, 256, (2, 13, 21, 3), generator=gen, dtype=U8).permute(0, 3, 1, 2)
    else:
        full = _buf(2, 3, 13, 21, layout, xdt, gen)
    if xdt == U8:
        flat = torch.arange(256, dtype=torch.int64).to(U8)
        full[0, 0, :12, :] = flat[:252].view(12, 21)
        full[0, 0, 12, :4] = flat[252:]
        assert full[0, 0].unique().numel() == 256
    got = _pad4_run(full, C, ydt, (pair, C, layout))
    ref = _pad4_ref(full[:, :C], ydt)
    assert got.dtype == ref.dtype
    _exact(got, ref, f'image_pad4 {pair} C{C} {layout}')
    assert (got[:, C:] == 0).all() and not torch.signbit(got[:, C:].float()).any()


@gpu
def test_image_pad4_grid_stride_beyond_16384_blocks():
    """1 x 3 x 2049 x 2048 uint8 -> bf16: 2048 pixels more than 16384 blocks of 256 hold, so the last ones are reached by the grid-stride loop only."""
    x = torch.randint(0, 256, (1, 3, 2049, 2048), generator=_gen('pad4 large'), dtype=U8)
    got = _pad4_run(x, 3, BF16, 'large')
    assert torch.equal(got, _pad4_ref(x, BF16))
