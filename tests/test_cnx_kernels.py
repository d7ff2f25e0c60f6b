"""The ConvNeXtV2 forward kernels against float64 restatements, per route and tile: mgdt_cnx_block_fwd (cnx_block.hip), mgdt_cnx_mlp_fwd
(mlp_chain.hip), mgdt_dwconv7_ln_fwd / _train_fwd and mgdt_grn_stats_fwd (pointwise.hip).  The GPU tests are marked `gpu`; the rest runs anywhere.

Routes.  Every GPU case names the route it is there for in its id; test_census_* asserts that name from the library's host-side queries
(mgdt_dwconv7_ln_route, mgdt_cnx_block_geometry), which are in turn held to Python restatements of the pickers over a grid of shapes.

Bounds.  dwconv7_ln has ONE rounding (the store) and grn_stats an fp32 output: plain kernel_ref._close of their dtype, the bf16 `u` of the training
form included.  The two fused kernels round to bf16 inside (t = LayerNorm output, h = GELU output, v = GRN output): a correct fp32 evaluation may
round an element that sits next to a rounding boundary to the other neighbour than the float64 reference, and one flipped t of magnitude 3 moves
a whole output pixel by about 1e-3 max|y|.  Their bound is _close's bf16 bound PLUS the flip allowance of kernel_ref.cnx_allowance, computed from the
float64 reference alone with the per-case delta_s of kernel_ref.cnx_deltas (4 x the fp32-vs-fp64 difference of the restatement at that stage, + 1e-6
at h for the polynomial GELU, itself held to 6e-7 of the erf GELU here).  test_allowance_caps holds every GPU case to: allowance above half the
plain bound on at most 2 % of the output elements, nowhere above 3 x the plain bound, and the fp32 evaluation of the restatement inside bound +
allowance - so the allowance cannot hide a wrong kernel (a wrong kernel moves far more than 2 % of the elements).

The closing conv is checked in two stages, as the Detect tail is: the launch without it against the restatement as above, then the launch with it
against a float64 evaluation of the closing conv on the bf16 map the first launch WROTE (plain _close).  Both instantiations perform the same
arithmetic up to bf16(acc2 + residual).

Two defects these cases exposed, fixed with them: the row kernel of dwconv7_ln computed the LayerNorm statistics of only the first
TS * C / 4 pixels of a tile when C < 4 * TS (c = 4: 8 of 64), and the closing conv inside cnx_block indexed its panel with C / 16 cout blocks per
chunk where mgdt_conv_pack lays out cdiv(C3, 16) (C = 64, C3 = 48 read the wrong weights and past the panel)."""
import functools
import os
import re

import pytest
import torch

from kernel_ref import (BF16, DEV, F32, ConvP, _bf16_bound, _borders_untouched, _check, _close_allow, _erf_gelu, _gen, _nhwc, _out_buf, _rand,
                        cnx_allowance, cnx_deltas, ref_cnx_block, ref_cnx_mlp, ref_cnx_tail, ref_dwconv7_ln, ref_grn_scale)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-6
MI355X_CUS = 256


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ restatements of the host pickers
def py_cnx_lds(c, th, tw):
    """cnx_lds of cnx_block.hip: total dynamic LDS bytes."""
    kc1, hd = c // 32, 4 * c
    segs = cdiv(tw, 5)
    rw, rh = segs * 5 + 6, th + 6
    npixa = cdiv(th * tw, 16) * 16
    al = lambda v: (v + 15) & ~15
    u = max(rh * rw * c * 2, kc1 * 8 * kc1 * 1024, 4 * kc1 * 2 * kc1 * 1024, th * tw * (c // 4) * 4)
    d = max(49 * c * 4, (3 * hd + 2 * kc1 * 16 + 16) * 4)
    t = max(npixa * (2 * c + 16), 16 * hd * 4)
    return al(u) + al(d) + al(t) + npixa * 4 + 64


def py_cnx_geometry(h, w, c):
    """cnx_pick_tile + the derived figures of mgdt_cnx_block_geometry, or None: fewest tiles, then least overhang, then the largest tile, then the
    smallest halo; at most 256 pixels (16 groups of 16), 1024 depth-wise threads, 6 halo pieces per thread, 160 KiB - 512 of LDS."""
    if c not in (32, 64, 96) or h < 1 or w < 1:
        return None
    q, best, pick = c // 4, None, None
    for th in range(2, 17):
        for tw in range(5, 41):
            if th * tw > 256:
                continue
            segs = cdiv(tw, 5)
            rw, rh = segs * 5 + 6, th + 6
            if q * th * segs > 1024 or rh * rw * (c // 8) > 6 * 1024 or py_cnx_lds(c, th, tw) > 160 * 1024 - 512:
                continue
            tiles = cdiv(h, th) * cdiv(w, tw)
            cost = tiles * 100000 + (tiles * th * tw - h * w) * 16 + (256 - th * tw) + rh * rw
            if best is None or cost < best:
                best, pick = cost, (th, tw)
    if pick is None:
        return None
    th, tw = pick
    return dict(TH=th, TW=tw, SEGS=cdiv(tw, 5), tiles_x=cdiv(w, tw), tiles=cdiv(w, tw) * cdiv(h, th), NWT=cdiv(th * tw, 16), lds_bytes=py_cnx_lds(c, th, tw))


def py_cnx_supported(n, h, w, c, dtype):
    g = py_cnx_geometry(h, w, c) if dtype == BF16 else None
    return bool(g and n >= 1 and g['tiles'] <= 256)


def _dw_lds(ts, c, sz):
    return (((ts + 6) * (ts + 6) * c * sz + 15) & ~15) + 49 * c * 4 + ts * ts * (c // 4) * 4 + ts * ts * 4


def _dw_cost(ts, n, h, w, c, sz):
    qt, l = c // 4, _dw_lds(ts, c, sz)
    if ts * qt > 256 or l + 256 > (64 if ts == 8 else 80) * 1024:
        return -1
    per_cu = max(1, min(160 * 1024 // (l + 256), 2048 // (ts * qt)))
    return cdiv(n * cdiv(h, ts) * cdiv(w, ts), 256 * per_cu) * ts * ts


def py_dw_route(n, h, w, c, dtype):
    """dwconv7_ln_plan of pointwise.hip (without the MGDT_DW_TS knob)."""
    sz, qt = (2 if dtype == BF16 else 4), c // 4
    c8, c10 = _dw_cost(8, n, h, w, c, sz), _dw_cost(10, n, h, w, c, sz)
    ts = 10 if c10 >= 0 and (c8 < 0 or c10 < c8) else 8
    if qt <= 32 and (c8 if ts == 8 else c10) >= 0:
        return dict(family=f'row{ts}', ts=ts, nwg=n * cdiv(h, ts) * cdiv(w, ts), lds_bytes=_dw_lds(ts, c, sz), threads=ts * qt)
    return dict(family='generic', ts=0, nwg=cdiv(n * h * w, 256 // qt), lds_bytes=0, threads=256)


def py_dw_retired_tiled_fits(c, dtype):
    """The test the retired 8x8 LDS-tiled kernel (several pixels per thread) applied to itself: C / 4 <= 64 and halo + weights + partials <= 64 KiB."""
    sz = 2 if dtype == BF16 else 4
    return c // 4 <= 64 and ((14 * 14 * c * sz + 15) & ~15) + 49 * c * 4 + 64 * (c // 4) * 4 <= 64 * 1024


# ------------------------------------------------------------------------------------------------ cases
# cnx_block: (what it pins, C, B, H, W, (TH, TW), tiles, pixel groups NWT, C3 of the closing conv, its activation)
BLOCK_CASES = [
    ('kc1-1-map-1x1-inside-the-window', 32, 2, 1, 1, (2, 5), 1, 1, 20, 'silu'),
    ('kc1-2-map-1x1-inside-the-window', 64, 2, 1, 1, (2, 5), 1, 1, 64, 'none'),
    ('kc1-3-map-1x1-inside-the-window', 96, 2, 1, 1, (2, 5), 1, 1, 96, 'silu'),
    ('kc1-1-map-5x3-tile-wider-than-map', 32, 2, 5, 3, (5, 5), 1, 2, 32, 'none'),
    ('kc1-2-map-5x3-tile-wider-than-map', 64, 2, 5, 3, (5, 5), 1, 2, 48, 'silu'),
    ('kc1-3-map-5x3-tile-wider-than-map', 96, 2, 5, 3, (5, 5), 1, 2, 96, 'none'),
    ('partial-last-group-147px-TW21', 32, 2, 7, 21, (7, 21), 1, 10, 20, 'none'),
    ('partial-last-group-117px-TW9', 64, 2, 13, 9, (13, 9), 1, 8, 48, 'none'),
    ('all-16-groups', 32, 2, 16, 16, (16, 16), 1, 16, 32, 'silu'),
    ('all-16-groups', 64, 2, 16, 16, (16, 16), 1, 16, 64, 'silu'),
    ('overhang-bottom-3-tiles', 96, 3, 23, 17, (8, 17), 3, 9, 96, 'silu'),
    ('overhang-bottom-2-tiles', 64, 2, 17, 16, (9, 16), 2, 9, 48, 'silu'),
    ('exactly-16-tiles-unrolled-sum', 32, 1, 61, 59, (16, 15), 16, 15, 20, 'silu'),
    ('18-tiles-loop-sum', 96, 2, 61, 59, (7, 30), 18, 14, 96, 'none'),
    ('20-tiles-loop-sum', 64, 1, 68, 68, (14, 17), 20, 15, 48, 'silu'),
    ('two-launches-last-holds-one-image', 32, MI355X_CUS // 2 + 1, 20, 20, (10, 20), 2, 13, 20, 'silu'),
]
# cnx_mlp: (what it pins, C, B, H, W, splits)
MLP_CASES = [
    ('B1-splits-eq-tiles-HW117', 32, 1, 13, 9, 8),
    ('B3-HW117-partial-last-tile', 64, 3, 13, 9, 8),
    ('HW1-one-pixel', 96, 3, 1, 1, 1),
    ('HW10-below-one-tile', 32, 3, 2, 5, 1),
    ('HW256-16-full-tiles', 64, 1, 16, 16, 16),
    ('HW512-32-tiles-2-workgroups', 96, 3, 32, 16, 32),
    ('B300-HW35-one-split', 96, 300, 7, 5, 1),
]
# dwconv7_ln: (C, B, H, W, route in fp32, route in bf16)
DW_CASES = [
    (4, 2, 13, 11, 'row8', 'row8'), (32, 2, 13, 11, 'row8', 'row8'), (96, 2, 13, 11, 'generic', 'row8'),
    (4, 1, 8, 8, 'row8', 'row8'), (32, 1, 8, 8, 'row8', 'row8'), (96, 1, 8, 8, 'generic', 'row8'),
    (32, 2, 1, 1, 'row8', 'row8'), (32, 2, 3, 5, 'row8', 'row8'), (32, 2, 7, 7, 'row8', 'row8'),
    (100, 2, 13, 11, 'generic', 'row10'), (96, 21, 40, 40, 'generic', 'row10'), (52, 21, 40, 40, 'row10', 'row8'),
    (104, 2, 9, 7, 'generic', 'generic'), (260, 2, 9, 7, 'generic', 'generic'), (1024, 2, 9, 7, 'generic', 'generic'),
    (64, 2, 13, 11, 'generic', 'row8'),
]
DW_PARAMS = [pytest.param(c, b, h, w, dt, rt, False, id=f'{"f32" if dt == F32 else "bf16"}-{rt}-c{c}-{b}x{h}x{w}')
             for (c, b, h, w, r32, r16) in DW_CASES for dt, rt in ((F32, r32), (BF16, r16))]
# the variance over the channels of the same order as eps (conv weights x 5e-4, no bias): the only inputs on which eps shows in the output
DW_PARAMS += [pytest.param(c, b, h, w, dt, rt, True, id=f'{"f32" if dt == F32 else "bf16"}-{rt}-c{c}-{b}x{h}x{w}-variance-near-eps')
              for (c, b, h, w, dt, rt) in ((32, 2, 7, 7, F32, 'row8'), (32, 2, 7, 7, BF16, 'row8'), (100, 2, 13, 11, BF16, 'row10'), (104, 2, 9, 7, F32, 'generic'))]
# grn_stats: (what it pins, C, B, H, W, sliced)
GRN_CASES = [
    ('c4-HW5-empty-bands', 4, 2, 1, 5, False),
    ('c64-HW117', 64, 2, 13, 9, True),
    ('c68-second-block-partial-quads-HW1600', 68, 2, 40, 40, False),
    ('c384-HW117', 384, 2, 13, 9, True),
    ('c8192-HW1', 8192, 2, 1, 1, False),
]
block_params = [pytest.param(*c, id=f'c{c[1]}-{c[2]}x{c[3]}x{c[4]}-tile{c[5][0]}x{c[5][1]}-{c[6]}tiles-{c[7]}grp-{c[0]}-tail{c[8]}{c[9]}') for c in BLOCK_CASES]
mlp_params = [pytest.param(*c, id=f'c{c[1]}-{c[2]}x{c[3]}x{c[4]}-{c[5]}splits-{c[0]}') for c in MLP_CASES]


def _uniform(gen, *shape, a=1.0):
    return ((torch.rand(*shape, generator=gen) * 2 - 1) * a)


def _mlp_weights(gen, C):
    """pwconv1 / pwconv2 weights uniform with unit fan-in variance and bf16-representable, fp32 biases, |gamma| <= 0.25: uniform draws keep the
    hidden map's tail - and with it the largest single-flip allowance - shorter than normal ones."""
    w1 = _uniform(gen, 4 * C, C, a=(3.0 / C) ** 0.5).to(BF16).float()
    w2 = _uniform(gen, C, 4 * C, a=(3.0 / (4 * C)) ** 0.5).to(BF16).float()
    b1, b2 = torch.randn(4 * C, generator=gen) * 0.1, torch.randn(C, generator=gen) * 0.1
    gamma, beta = _uniform(gen, 4 * C, a=0.25), torch.randn(4 * C, generator=gen) * 0.1
    return w1, b1, w2, b2, gamma, beta


def _ln_weights(gen, C):
    return (torch.randn(C, 1, 7, 7, generator=gen) * 0.2, torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5,
            torch.randn(C, generator=gen) * 0.1)


@functools.lru_cache(maxsize=None)
def block_case(C, B, H, W):
    """Inputs, float64 reference, delta_s and flip allowance of one cnx_block case: computed once, shared by the host-only and the GPU tests."""
    gen = _gen('cnx_block', C, B, H, W)
    x = _rand(gen, B, C, H, W, dt=BF16)
    ln = _ln_weights(gen, C)
    mlp = _mlp_weights(gen, C)
    y, st = ref_cnx_block(x, *ln, EPS, *mlp, stages=True)
    deltas = cnx_deltas(st, mlp[0], mlp[1], mlp[4], mlp[5], ln=(x, *ln, EPS))
    allow, count = cnx_allowance(st, deltas, mlp[0], mlp[1], mlp[2], mlp[5])
    return dict(x=x, ln=ln, mlp=mlp, y=y, deltas=deltas, allow=allow, count=count, gen=gen)


@functools.lru_cache(maxsize=None)
def mlp_case(C, B, H, W):
    gen = _gen('cnx_mlp', C, B, H, W)
    t, res = _rand(gen, B, C, H, W, dt=BF16), _rand(gen, B, C, H, W, dt=BF16)
    mlp = _mlp_weights(gen, C)
    y, st = ref_cnx_mlp(t, res, *mlp, stages=True)
    st['t'] = t
    deltas = cnx_deltas(st, mlp[0], mlp[1], mlp[4], mlp[5])
    allow, count = cnx_allowance(st, deltas, mlp[0], mlp[1], mlp[2], mlp[5])
    return dict(t=t, res=res, mlp=mlp, y=y, y_nores=y - res, deltas=deltas, allow=allow, count=count, gen=gen)


def _caps(y, allow, y32, what):
    bound = _bf16_bound(y)
    share = (allow > 0.5 * bound).double().mean().item()
    worst = (allow / bound).max().item()
    use = ((y32.double() - y).abs() / (bound + allow)).max().item()
    print(f'{what}: allowance above half the bound on {100 * share:.2f} % of the elements, at most {worst:.2f} x the bound; the fp32 evaluation uses '
          f'{use:.3f} of bound + allowance')
    assert share <= 0.02, (what, 'allowance above half the plain bound on more than 2 % of the elements', share)
    assert worst <= 3.0, (what, 'allowance above 3 x the plain bound', worst)
    assert use <= 1.0, (what, 'the fp32 evaluation of the restatement leaves bound + allowance', use)


# ------------------------------------------------------------------------------------------------ host-only: polynomial, census, caps
def test_gelu_polynomial_within_6e_7_of_erf_gelu():
    """The eight coefficients and the cap of gelu_fast / gelu_coef (mlp_common.h), evaluated in float64 on a dense grid of [-8, 8]:
    max(v, 0) - |v| * 2^p(min(|v|, cap)) within 6e-7 of 0.5 v (1 + erf(v / sqrt 2)), the figure the header states."""
    src = open(os.path.join(ROOT, 'mgdt_yolo_amd', 'csrc', 'mlp_common.h')).read()
    m = re.search(r'return GeluCoef\{\{([^}]*)\},\s*([0-9.e+-]+)f\}', src)
    coef = [float(v.strip().rstrip('f')) for v in m.group(1).split(',')]
    cap = float(m.group(2))
    assert len(coef) == 8 and cap == 6.5
    body = src[src.index('float gelu_fast(float v)'):src.index('typedef')]
    assert [float(v) for v in re.findall(r'(-?\d\.\d+e[+-]\d+)f', body)] == coef, 'gelu_fast and gelu_coef must hold the same coefficients'
    v = torch.linspace(-8, 8, 3_200_001, dtype=torch.float64)
    a = v.abs().clamp(max=cap)
    p = torch.full_like(a, coef[0])
    for k in coef[1:]:
        p = p * a + k
    err = (v.clamp(min=0) - v.abs() * torch.exp2(p) - _erf_gelu(v)).abs().max().item()
    print(f'polynomial GELU: max |error| {err:.3e} on [-8, 8]')
    assert err <= 6e-7, err


CENSUS_MAPS = [(1, 1, 1), (2, 3, 5), (1, 8, 8), (2, 13, 11), (2, 9, 7), (3, 23, 17), (21, 40, 40), (32, 40, 40), (64, 20, 20), (1, 80, 80), (1, 160, 160),
               (300, 7, 5), (7, 33, 65)]


def test_census_dwconv7_route_matches_the_restated_plan():
    """mgdt_dwconv7_ln_route == py_dw_route for every c in 4..1024 (step 4), both dtypes, thirteen maps; shapes the forward call refuses are refused."""
    from mgdt_yolo_amd import ops
    for dt in (F32, BF16):
        for c in range(4, 1025, 4):
            for n, h, w in CENSUS_MAPS:
                assert ops.dwconv7_ln_route(n, h, w, c, dt) == py_dw_route(n, h, w, c, dt), (dt, c, n, h, w)
    for bad in ((1, 8, 8, 6), (1, 8, 8, 1028), (0, 8, 8, 32), (1, 0, 8, 32), (1, 8, 8, 0)):
        with pytest.raises(RuntimeError):
            ops.dwconv7_ln_route(*bad, BF16)


def test_census_retired_tiled_kernel_was_unreachable():
    """Why dwconv7_ln_tiled_kernel is gone: for every c in 4..1024 (step 4) and both dtypes, wherever its own LDS test let it run, an 8x8 or 10x10
    row kernel fits as well - and the plan asks the row kernels first, whatever the map.  The row kernels' feasibility does not depend on the map."""
    for dt in (F32, BF16):
        sz = 2 if dt == BF16 else 4
        for c in range(4, 1025, 4):
            if py_dw_retired_tiled_fits(c, dt):
                assert c // 4 <= 32 and (_dw_cost(8, 1, 1, 1, c, sz) >= 0 or _dw_cost(10, 1, 1, 1, c, sz) >= 0), (dt, c)
                for n, h, w in CENSUS_MAPS:
                    assert py_dw_route(n, h, w, c, dt)['family'] != 'generic', (dt, c, n, h, w)
    # the last channel count of each dtype that has a row kernel, and the first without: the tiled kernel did not fit the latter either
    assert py_dw_route(1, 8, 8, 100, BF16)['family'] == 'row10' and py_dw_route(1, 8, 8, 104, BF16)['family'] == 'generic'
    assert py_dw_route(1, 8, 8, 60, F32)['family'] == 'row8' and py_dw_route(1, 8, 8, 64, F32)['family'] == 'generic'
    assert not py_dw_retired_tiled_fits(104, BF16) and not py_dw_retired_tiled_fits(64, F32)


def test_census_fp32_c64_and_above_is_generic_and_row10_only_where_stated():
    """fp32 c >= 64 always takes the generic kernel (the existing fp32 cases `bench`, `odd-96` and `c64` of test_dwconv7_layernorm_kernel_vs_torch do).
    row<10> is chosen only where 8x8 tiles need another round of workgroups over the chip than 10x10 tiles do (bf16 c = 96 at 21x40x40), or where
    8x8 does not fit at all (bf16 c = 100, any map)."""
    for n, h, w in CENSUS_MAPS:
        for c in range(64, 1025, 4):
            assert py_dw_route(n, h, w, c, F32)['family'] == 'generic'
        assert py_dw_route(n, h, w, 100, BF16)['family'] == 'row10'
    for dt in (F32, BF16):
        sz = 2 if dt == BF16 else 4
        for c in range(4, 129, 4):
            for n, h, w in CENSUS_MAPS:
                if py_dw_route(n, h, w, c, dt)['family'] == 'row10':
                    c8, c10 = _dw_cost(8, n, h, w, c, sz), _dw_cost(10, n, h, w, c, sz)
                    assert c8 < 0 or c10 < c8
                    if c8 >= 0:     # both fit: 10x10 needs fewer (rounds x pixels per round)
                        assert c10 // 100 < c8 // 64
    assert py_dw_route(21, 40, 40, 96, BF16)['family'] == 'row10' and py_dw_route(20, 40, 40, 96, BF16)['family'] == 'row8'
    assert py_dw_route(32, 40, 40, 96, BF16)['family'] == 'row10'      # the bench map
    assert py_dw_route(2, 12, 10, 160, BF16)['family'] == 'generic'    # the case once named `c160-tiled`


def test_census_cnx_block_geometry_matches_the_restated_picker():
    """mgdt_cnx_block_geometry / mgdt_cnx_block_supported == the Python restatement of cnx_pick_tile / cnx_lds over a grid of maps, refused ones
    included: more tiles than 256 (300x300), C = 128, fp32."""
    from mgdt_yolo_amd import _lib, ops
    sizes = [1, 2, 3, 5, 7, 9, 13, 16, 17, 20, 21, 23, 40, 59, 60, 61, 67, 68, 80, 160, 300]
    lib = _lib.lib()
    for c in (32, 64, 96):
        for h in sizes:
            for w in sizes:
                g = py_cnx_geometry(h, w, c)
                assert g is not None and ops.cnx_block_geometry(h, w, c) == g, (c, h, w)
                assert g['NWT'] <= 16 and g['lds_bytes'] <= 160 * 1024 - 512
                assert bool(lib.mgdt_cnx_block_supported(2, h, w, c, _lib.BF16)) == py_cnx_supported(2, h, w, c, BF16), (c, h, w)
                assert lib.mgdt_cnx_block_workspace_bytes(2, h, w, c) == 4096 + 2 * g['tiles'] * 4 * c * 4
    assert not lib.mgdt_cnx_block_supported(1, 300, 300, 96, _lib.BF16) and py_cnx_geometry(300, 300, 96)['tiles'] > 256
    assert lib.mgdt_cnx_block_supported(1, 160, 160, 96, _lib.BF16)
    assert not lib.mgdt_cnx_block_supported(1, 20, 20, 128, _lib.BF16) and not lib.mgdt_cnx_block_supported(1, 20, 20, 96, _lib.F32)
    assert not lib.mgdt_cnx_block_supported(0, 20, 20, 96, _lib.BF16)
    for bad in ((20, 20, 128), (20, 20, 48), (0, 20, 96)):
        with pytest.raises(RuntimeError):
            ops.cnx_block_geometry(*bad)
    # the loop form of the GRN partial-sum read (tiles > 16) needs maps of this size; the bench map (40x40) and 80x80 at C = 32 / 64 stay below
    assert py_cnx_geometry(61, 59, 96)['tiles'] == 18 and py_cnx_geometry(68, 68, 64)['tiles'] == 20 and py_cnx_geometry(68, 68, 32)['tiles'] == 20
    assert py_cnx_geometry(61, 59, 32)['tiles'] == 16 and py_cnx_geometry(40, 40, 96)['tiles'] <= 16 and py_cnx_geometry(64, 64, 64)['tiles'] <= 16


def test_census_every_gpu_case_runs_the_route_in_its_id():
    from mgdt_yolo_amd import _lib, ops
    for what, C, B, H, W, tile, tiles, nwt, c3, act in BLOCK_CASES:
        g = ops.cnx_block_geometry(H, W, C)
        assert (g['TH'], g['TW'], g['tiles'], g['NWT']) == (*tile, tiles, nwt), (what, C, g)
        assert _lib.lib().mgdt_cnx_block_supported(B, H, W, C, _lib.BF16)
        assert c3 <= C and c3 % 4 == 0
    by = {c[0] + str(c[1]): c for c in BLOCK_CASES}
    assert by['exactly-16-tiles-unrolled-sum32'][6] == 16 and min(by['18-tiles-loop-sum96'][6], by['20-tiles-loop-sum64'][6]) > 16
    assert any(c[7] == 16 for c in BLOCK_CASES) and any(c[5][0] * c[5][1] % 16 for c in BLOCK_CASES) and any(c[5][1] % 5 for c in BLOCK_CASES)
    assert {(c[1], c[8]) for c in BLOCK_CASES} >= {(96, 96), (64, 48), (32, 20), (64, 64), (32, 32)} and {c[9] for c in BLOCK_CASES} == {'silu', 'none'}
    # several launches: images per launch = CUs // tiles; CUs // 2 + 1 images of two tiles need a second launch, which holds one image
    last = BLOCK_CASES[-1]
    assert last[6] == 2 and last[2] == MI355X_CUS // last[6] + 1
    for c, b, h, w, r32, r16 in DW_CASES:
        assert ops.dwconv7_ln_route(b, h, w, c, F32)['family'] == r32 and ops.dwconv7_ln_route(b, h, w, c, BF16)['family'] == r16, (c, b, h, w)
    assert {r for c in DW_CASES for r in c[4:]} == {'row8', 'row10', 'generic'}
    assert any(256 % (c[0] // 4) for c in DW_CASES if c[0] > 100) and any(c[0] == 1024 for c in DW_CASES)      # idle threads; one pixel per block


def _mlp_splits(n, h, w, c):
    from mgdt_yolo_amd import _lib
    nbytes = _lib.lib().mgdt_cnx_mlp_workspace_bytes(n, h, w, c)
    assert nbytes % (n * 4 * c * 4) == 0
    return nbytes // (n * 4 * c * 4)


def test_census_cnx_mlp_one_wave_tile_per_wave():
    """splits (workgroups per image, derived from mgdt_cnx_mlp_workspace_bytes) = max(cdiv(tiles, 16), min(cdiv(256, n), tiles)) with tiles =
    cdiv(HW, 16); tiles <= 16 * splits always, so no wave of the 16 ever has a second wave tile: the `tile += tstep` loop of cnx_mlp_kernel never
    takes a second trip (its prefetch of the next tile is dead code today)."""
    for n in (1, 2, 3, 16, 17, 32, 255, 256, 300):
        for h, w in ((1, 1), (2, 5), (13, 9), (16, 16), (32, 16), (7, 5), (40, 40), (80, 80), (160, 160)):
            tiles = cdiv(h * w, 16)
            s = _mlp_splits(n, h, w, 96)
            assert s == max(cdiv(tiles, 16), min(cdiv(256, n), tiles)) and 1 <= s <= tiles <= 16 * s, (n, h, w, s)
    for what, C, B, H, W, splits in MLP_CASES:
        assert _mlp_splits(B, H, W, C) == splits, what
    assert _mlp_splits(1, 13, 9, 32) == cdiv(117, 16) and _mlp_splits(300, 7, 5, 96) == cdiv(cdiv(35, 16), 16)


@pytest.mark.parametrize('what,C,B,H,W,tile,tiles,nwt,c3,act', block_params)
def test_allowance_caps_cnx_block(what, C, B, H, W, tile, tiles, nwt, c3, act):
    """Conditions on the INPUTS of every cnx_block GPU case (see the module docstring), and the fp32 evaluation of the restatement inside
    bound + allowance."""
    k = block_case(C, B, H, W)
    print(f'delta_s: {k["deltas"]}, undecided elements: {k["count"]}')
    _caps(k['y'], k['allow'], ref_cnx_block(k['x'], *k['ln'], EPS, *k['mlp'], dt=F32), what)


@pytest.mark.parametrize('what,C,B,H,W,splits', mlp_params)
def test_allowance_caps_cnx_mlp(what, C, B, H, W, splits):
    k = mlp_case(C, B, H, W)
    print(f'delta_s: {k["deltas"]}, undecided elements: {k["count"]}')
    _caps(k['y'], k['allow'], ref_cnx_mlp(k['t'], k['res'], *k['mlp'], dt=F32), what)


# ------------------------------------------------------------------------------------------------ GPU: cnx_block
def _dw49(dw):
    return dw.reshape(dw.shape[0], 49).t().contiguous().to(DEV)


def _dev_mlp(mlp):
    from mgdt_yolo_amd import ops
    w1, b1, w2, b2, gamma, beta = (t.to(DEV) for t in mlp)
    return ops.PackedCnxMlp(w1, b1, w2, b2, BF16), gamma.contiguous(), beta.contiguous()


def _three_times(fn, out):
    """Replays: three calls into the same buffer must leave the same bits (the barrier words and partial sums persist across calls)."""
    bits = []
    for _ in range(3):
        fn()
        bits.append(out.clone())
    torch.cuda.synchronize()
    assert torch.equal(bits[0], bits[1]) and torch.equal(bits[0], bits[2]), 'replays differ'


@gpu
@pytest.mark.parametrize('what,C,B,H,W,tile,tiles,nwt,c3,act', block_params)
def test_cnx_block(what, C, B, H, W, tile, tiles, nwt, c3, act):
    """Stage 1: the launch without a closing conv against ref_cnx_block + flip allowance.  Stage 2: the launch with it against the float64 closing
    conv of the bf16 map stage 1 wrote (plain bf16 _close).  x and both outputs are channel slices at offset 8 of wider buffers full of random
    values (an unmasked halo or overhang read would pick those up; the neighbours of the outputs must come back bit-identical); every launch is
    made three times.  Always through ops.cnx_block, which owns the zeroed workspace."""
    from mgdt_yolo_amd import ops
    if what.startswith('two-launches'):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert B == cus // tiles + 1, f'this case is sized for {MI355X_CUS} compute units, the device has {cus}'
    k = block_case(C, B, H, W)
    gen = torch.Generator().manual_seed(B * H * W + C)
    xv, _ = _nhwc(k['x'], BF16, 8, 8, gen)
    assert ops.cnx_block_supported(xv, BF16)
    dwb, lnw, lnb = (t.to(DEV) for t in k['ln'][1:])
    pk, gamma, beta = _dev_mlp(k['mlp'])
    args = (xv, _dw49(k['ln'][0]), dwb, lnw, lnb, EPS, pk, gamma, beta)
    out, big, big0 = _out_buf(B, C, H, W, BF16, 8, 8, gen)
    _three_times(lambda: ops.cnx_block(*args, out=out), out)
    _borders_untouched(big, big0, 8, C)
    print(f'delta_s: {k["deltas"]}')
    _close_allow(out, k['y'], k['allow'], f'cnx_block {what} c{C}')
    # stage 2
    cp = ConvP(_gen('cnx_tail', C, c3), c3, C, 1, bn=True, bias=False)
    w, cb, bn = cp.dev_args(ops.acc_order_index(C, 'cpu'))
    pk3 = ops.PackedConv(w, cb, bn, 1, BF16)
    out3, big3, big30 = _out_buf(B, c3, H, W, BF16, 8, 8 + -c3 % 8, gen)      # pixel stride a multiple of 8 elements, as the kernel's 16-byte rule asks
    code = {'silu': ops.ACT_SILU, 'none': ops.ACT_NONE}[act]
    _three_times(lambda: ops.cnx_block(*args, out=out3, tail=pk3, tail_act=code), out3)
    _borders_untouched(big3, big30, 8, c3)
    _check(out3, ref_cnx_tail(out.double().cpu(), cp, act), BF16, f'cnx_block closing conv {C}->{c3} {act} {what}')


@gpu
def test_cnx_block_refuses_misaligned_views_before_any_launch():
    """Channel offset 4 (an 8-byte aligned pointer) and pixel strides that are no multiple of 8 elements: MGDT_BAD_SHAPE, outputs untouched."""
    from mgdt_yolo_amd import ops
    k = block_case(32, 2, 5, 3)
    gen = torch.Generator().manual_seed(1)
    dwb, lnw, lnb = (t.to(DEV) for t in k['ln'][1:])
    pk, gamma, beta = _dev_mlp(k['mlp'])
    rest = (_dw49(k['ln'][0]), dwb, lnw, lnb, EPS, pk, gamma, beta)
    good, _ = _nhwc(k['x'], BF16, 8, 8, gen)
    for xoff, xextra, ooff, oextra in ((4, 4, 8, 8), (8, 8, 4, 4), (0, 4, 8, 8), (8, 8, 0, 4)):
        xv, _ = _nhwc(k['x'], BF16, xoff, xextra, gen)
        out, big, big0 = _out_buf(2, 32, 5, 3, BF16, ooff, oextra, gen)
        with pytest.raises(RuntimeError, match='16-byte aligned'):
            ops.cnx_block(xv, *rest, out=out)
        torch.cuda.synchronize()
        assert torch.equal(big.cpu(), big0)
    out, _, _ = _out_buf(2, 32, 5, 3, BF16, 8, 8, gen)
    ops.cnx_block(good, *rest, out=out)


# ------------------------------------------------------------------------------------------------ GPU: cnx_mlp
@gpu
@pytest.mark.parametrize('what,C,B,H,W,splits', mlp_params)
def test_cnx_mlp(what, C, B, H, W, splits):
    """STATS + APPLY against ref_cnx_mlp + flip allowance over h and v; t is a slice at channel offset 8, res and y at offset 4."""
    from mgdt_yolo_amd import ops
    k = mlp_case(C, B, H, W)
    gen = torch.Generator().manual_seed(B * H * W + C)
    tv, _ = _nhwc(k['t'], BF16, 8, 8, gen)
    rv, _ = _nhwc(k['res'], BF16, 4, 4, gen)
    pk, gamma, beta = _dev_mlp(k['mlp'])
    out, big, big0 = _out_buf(B, C, H, W, BF16, 4, 4, gen)
    ops.cnx_mlp(tv, rv, pk, gamma, beta, out=out)
    first = out.clone()
    ops.cnx_mlp(tv, rv, pk, gamma, beta, out=out)
    assert torch.equal(first, out), 'two calls differ'
    _borders_untouched(big, big0, 4, C)
    print(f'delta_s: {k["deltas"]}')
    _close_allow(out, k['y'], k['allow'], f'cnx_mlp {what} c{C}')


@gpu
def test_cnx_mlp_without_residual():
    """res = NULL is part of the C entry point, not of ops.cnx_mlp's contract: reached with a direct launch."""
    from mgdt_yolo_amd import _lib, ops
    what, C, B, H, W, _ = MLP_CASES[1]
    k = mlp_case(C, B, H, W)
    gen = torch.Generator().manual_seed(9)
    tv, _ = _nhwc(k['t'], BF16, 8, 8, gen)
    pk, gamma, beta = _dev_mlp(k['mlp'])
    out, big, big0 = _out_buf(B, C, H, W, BF16, 4, 4, gen)
    ws = torch.empty(_lib.lib().mgdt_cnx_mlp_workspace_bytes(B, H, W, C), dtype=torch.uint8, device=DEV)
    ops._launch('cnx_mlp_fwd', 'mgdt_cnx_mlp_fwd', ops.vp(tv), None, ops.ptr(pk.blob), ops.ptr(gamma), ops.ptr(beta), ops.ptr(ws), ops.vp(out),
                ops.dtype_code(BF16), ops.stream())
    _borders_untouched(big, big0, 4, C)
    _close_allow(out, k['y_nores'], k['allow'], f'cnx_mlp no residual c{C}')


# ------------------------------------------------------------------------------------------------ GPU: dwconv7_ln
@gpu
@pytest.mark.parametrize('c,B,H,W,dt,route,tiny', DW_PARAMS)
def test_dwconv7_ln(c, B, H, W, dt, route, tiny):
    """y of the inference form and (y, u) of the training form against ref_dwconv7_ln in float64, plain _close of the dtype; input and both outputs
    are channel slices at offset 4.  Every pixel of every map is compared: edge rows and columns and the tiles that overhang the map included."""
    from mgdt_yolo_amd import ops
    assert ops.dwconv7_ln_route(B, H, W, c, dt)['family'] == route
    gen = _gen('dwconv7', c, B, H, W)
    x = _rand(gen, B, c, H, W, dt=BF16)
    dw, dwb, lnw, lnb = _ln_weights(gen, c)
    if tiny:
        dw, dwb = dw * 5e-4, torch.zeros(c)
    y_ref, u_ref = ref_dwconv7_ln(x, dw, dwb, lnw, lnb, EPS)
    if tiny:
        var = u_ref.var(1, unbiased=False)
        assert 0.05 * EPS < var.median().item() < 20 * EPS, var.median().item()
    xv, _ = _nhwc(x, dt, 4, 4, gen)
    args = (_dw49(dw), dwb.to(DEV), lnw.to(DEV), lnb.to(DEV), EPS)
    out, big, big0 = _out_buf(B, c, H, W, dt, 4, 4, gen)
    ops.dwconv7_ln(xv, *args, out=out)
    _borders_untouched(big, big0, 4, c)
    _check(out, y_ref, dt, f'dwconv7_ln y {route} c{c}')
    # training form: its own outputs are dense; a sliced pair goes through the C entry point
    y2, u = ops.dwconv7_ln_train(xv, *args)
    assert torch.equal(y2, out)
    _check(u, u_ref, dt, f'dwconv7_ln u {route} c{c}')
    yo, ybig, ybig0 = _out_buf(B, c, H, W, dt, 4, 4, gen)
    uo, ubig, ubig0 = _out_buf(B, c, H, W, dt, 8, 4, gen)
    ops._launch('dwconv7_ln_train_fwd', 'mgdt_dwconv7_ln_train_fwd', ops.vp(xv), *(ops.ptr(a) for a in args[:4]), EPS, ops.vp(yo), ops.vp(uo),
                ops.dtype_code(dt), ops.stream())
    _borders_untouched(ybig, ybig0, 4, c)
    _borders_untouched(ubig, ubig0, 8, c)
    assert torch.equal(yo, out) and torch.equal(uo, u)


# ------------------------------------------------------------------------------------------------ GPU: grn_stats
@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('what,C,B,H,W,sliced', [pytest.param(*c, id=c[0]) for c in GRN_CASES])
def test_grn_stats(what, C, B, H, W, sliced, dt):
    """scale = gamma * Gx / (mean_c Gx + 1e-6) + 1 against float64, _close F32 (the output is fp32 whatever the input dtype).  Channel 1 of image 0
    is all zero (Gx = 0: the scale is exactly 1 there); gamma = 0 gives exactly 1 everywhere."""
    from mgdt_yolo_amd import ops
    gen = _gen('grn', what)
    t = _rand(gen, B, C, H, W, dt=BF16)
    t[0, 1] = 0
    gamma = torch.randn(C, generator=gen) * 0.5
    tv, _ = _nhwc(t, dt, 4, 4, gen) if sliced else _nhwc(t, dt)
    sc = ops.grn_scale(tv, gamma.to(DEV))
    _check(sc, ref_grn_scale(t, gamma), F32, f'grn_stats {what}')
    assert sc[0, 1].item() == 1.0
    one = ops.grn_scale(tv, torch.zeros(C, device=DEV))
    assert (one == 1.0).all()
