"""The five fused forward kernels of bf16 inference - mgdt_csp_block_fwd, mgdt_pw_chain3_fwd, mgdt_conv1x1_inject_fwd,
mgdt_conv1x1_inject_conv_fwd, mgdt_detect_tail(_aug)_fwd - against float64 restatements on the CPU (kernel_ref.py), per route and tile, through the
ops.* entry points.  GPU cases need a real MI355X (-m gpu); the predicate and soundness tests run on the host.

Kernel and reference see the SAME values: inputs and weights are representable in bf16, a BN tuple is folded as the pack kernels fold it
(kernel_ref._fold).  The reference rounds to bf16 exactly where the kernel stores bf16 by design (stated in each restatement's docstring) and
nowhere else.  Bounds (kernel_ref._close, unchanged):
  bf16 outputs: every element within 2^-8 * |ref| + 1e-3 * max|ref|.
  fp32 outputs: relative L2 error <= 2e-5 and every element within 1e-4 * max|ref|.
fp32 outputs computed from a stored bf16 map (detect_tail's y and best keys, csp_block's pool sums) are checked in two stages: the bf16 map against
float64, then the fp32 output against a float64 evaluation of the map the kernel itself wrote.
test_restatement_soundness shows for each restatement that its fp32 evaluation stays within the bf16 bound of its fp64 one at the seeds used:
accumulation order and the rare one-ulp flip of an intermediate do not break the bound by themselves.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from kernel_ref import (BF16, DEV, F32, ConvP, _borders_untouched, _check, _gen, _nhwc, _out_buf, _rand, inj_bilinear, inj_lerp, ref_csp_block,
                        ref_detect_decode, ref_detect_map, ref_inject, ref_inject_conv, ref_pw_chain3)
from knobs import forced_tile as _forced_tile

gpu = pytest.mark.gpu
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ host predicates (mirror the C dispatch)
def chain_nbk(wd):
    """chain_nbk of mlp_chain.hip: 16-channel blocks of the chain, 3 runs as 4; 0 = refused (wd % 4, wd < 4, wd > 64)."""
    if wd < 4 or wd % 4 or wd > 64:
        return 0
    nbk = (wd + 15) // 16
    return 4 if nbk == 3 else nbk


def chain_second_round_pixels(wd):
    """pw_chain3's grid is capped at 2048 workgroups of 8 waves, a wave takes 16 * MT pixels (MT = 4 for nbk <= 2, else 2): a wave takes a second
    tile above this many pixels."""
    return 2048 * 8 * 16 * (4 if chain_nbk(wd) <= 2 else 2)


def csp_supported(mode, cin, cout, wd, n, h, w):
    """mgdt_csp_block_supported for bf16."""
    if wd not in (8, 16, 32, 64) or n < 1 or n > 2 or cout % 4:
        return False
    catc = (3 if mode == 0 else 2) * wd + n * wd
    if catc > 256 or catc % 8:
        return False
    if mode == 0:
        return cin == 4 * wd and h % 2 == 0 and w % 2 == 0 and h >= 4 and w >= 4
    return cin == 2 * wd and wd >= 16


def csp_lds(mode, wd, n, th, tw):
    """csp_geometry: P and T over the (th + 4n)(tw + 4n) region (+ the last pixel group's reach) at 2 wd bytes, the concat of the tile's pixels
    without the last bottleneck output, the staged chain (MSPA)."""
    rp = (th + 4 * n) * (tw + 4 * n)
    rpa, tpa = (rp + 30) // 16 * 16, (th * tw + 15) // 16 * 16
    catc = (3 if mode == 0 else 2) * wd + n * wd
    nbk = max(wd // 16, 1)
    extra = 3 * ((nbk + 1) // 2) * nbk * 1024 + 3 * nbk * 64 if mode == 0 else 0
    return 2 * rpa * wd * 2 + tpa * (catc - wd) * 2 + extra


def csp_pick(mode, B, wd, n, H, W, forced=None):
    """csp_pick_tile: (th, tw, lds) of the cheapest tile that divides the (half-)map and fits 156 KiB, or None."""
    qh, qw = (H // 2, W // 2) if mode == 0 else (H, W)
    best, best_cost = None, 1e30
    for th in range(2, min(qh, 32) + 1):
        if qh % th:
            continue
        for tw in range(2, min(qw, 32) + 1):
            if qw % tw or (forced and (th, tw) != tuple(forced)):
                continue
            lds = csp_lds(mode, wd, n, th, tw)
            if lds > 156 * 1024:
                continue
            wgs = float(B) * (W // tw) * (H // th)
            cost = (float((th + 4 * n) * (tw + 4 * n)) / (th * tw)) / (float(th * tw) / ((th * tw + 15) // 16 * 16))
            if wgs < 256:
                cost *= 256.0 / wgs
            if wd <= 32 and lds > 80 * 1024:
                cost *= 2.0
            if cost < best_cost:
                best, best_cost = (th, tw, lds), cost
    return best


def csp_pool_gst(cout):
    nbo = (cout + 15) // 16
    return 8 // nbo if (nbo < 8 and 8 % nbo == 0) else 1


def inj_patch(H, W, Hg, Wg, TH):
    """inj_patch / inj_patch_th: the largest source patch (rows, cols) a TH x 16 workgroup needs."""
    y0, y1, _ = inj_lerp(H, Hg)
    x0, x1, _ = inj_lerp(W, Wg)
    ph = max(int(y1[min(t + TH - 1, H - 1)] - y0[t]) + 1 for t in range(0, H, TH))
    pw = max(int(x1[min(t + 15, W - 1)] - x0[t]) + 1 for t in range(0, W, 16))
    return ph, pw


def inj_kc(cin):
    return (cin + 31) // 32


def inject_supported(cin, cout, H, W, Hg, Wg):
    """mgdt_conv1x1_inject_supported (bf16): LDS = panel + two source patches of cout + 8 channels, at most 80 KiB."""
    if cin % 8 or cin > 128 or cout not in (128, 256) or H < Hg or W < Wg or Hg < 1 or Wg < 1:
        return False
    ph, pw = inj_patch(H, W, Hg, Wg, 4)
    return inj_kc(cin) * (cout // 16) * 1024 + 2 * ph * pw * (cout + 8) * 2 <= 80 * 1024


def inject_conv_supported(cin, cmid, cout2, H, W, Hg, Wg):
    """mgdt_conv1x1_inject_conv_supported (bf16): source patch of an 8 x 16 workgroup within 64 pixels, LDS within 156 KiB."""
    if cin % 8 or cin > 128 or cmid != 256 or cout2 % 16 or cout2 < 16 or cout2 > 64 or H < Hg or W < Wg or Hg < 1 or Wg < 1:
        return False
    ph, pw = inj_patch(H, W, Hg, Wg, 8)
    nb, nb2 = cmid // 16, cout2 // 16
    lds = inj_kc(cin) * nb * 1024 + (nb // 2) * nb2 * 1024 + max(2 * ph * pw * (nb * 16 + 8) * 2, 2 * nb * 2 * 1024)
    return ph * pw <= 64 and lds <= 156 * 1024


def tail_supported(c2, c3, nc, reg_max=4):
    return reg_max == 4 and c2 % 8 == 0 and c2 <= 32 and c3 % 8 == 0 and c3 <= 128 and 4 <= nc <= 256 and nc % 4 == 0


def tail_lds(c3, nc):
    """detect_tail_launch: box panel, class panel (kch x nbc KiB), biases, four waves' staging tiles, the 3x3 box panel + its bias; above 64 KiB
    the launch raises the kernel's dynamic-LDS limit first."""
    kch, nbc = (c3 + 31) // 32, (nc + 15) // 16
    return 1024 + kch * nbc * 1024 + (16 + nbc * 16) * 4 + 4 * (2 * 16 + 4) * 20 * 4 + 5 * 1024 + 64


INJ_CAP, INJ2_CAP, TAIL_CAP_UNITS, CONV_CAP_ROWS = 512, 256, 1024 * 4, 256 * 256     # persistent grids: patches / patches / 32-anchor units / output rows


def _c_tiles(mode, B, cin, cout, wd, n, H, W, tile):
    from mgdt_yolo_amd import _lib
    g = (C.c_int * 8)()
    with _forced_tile(tile):
        slots = _lib.lib().mgdt_csp_block_tiles(mode, B, cin, cout, wd, n, H, W, g)
    return slots, list(g)


# ------------------------------------------------------------------------------------------------ pw_chain3
# (id, wd, B, H, W, x offset, out offset, bn)
CHAIN_CASES = [
    ('wd8-nbk1-M70', 8, 2, 5, 7, 0, 0, False), ('wd12-nbk1-slices', 12, 1, 9, 9, 4, 4, False), ('wd16-nbk1-1x1', 16, 3, 1, 1, 0, 0, False),
    ('wd24-nbk2', 24, 2, 6, 11, 0, 4, False), ('wd32-nbk2-bn', 32, 1, 7, 9, 0, 0, True), ('wd40-nbk3as4', 40, 1, 5, 13, 4, 0, False),
    ('wd64-nbk4-slices', 64, 2, 3, 11, 4, 4, False),
    (f'wd4-2nd-round-{1025 * 1025}px-over-{chain_second_round_pixels(4)}', 4, 1, 1025, 1025, 0, 0, False),
]


def _chain_inputs(cid, wd, B, H, W, bn):
    gen = _gen('chain', cid)
    return _rand(gen, B, 3 * wd, H, W, dt=BF16), [ConvP(gen, wd, wd, 1, bn=bn, gain=1.5) for _ in range(3)], gen


@gpu
@pytest.mark.parametrize('cid,wd,B,H,W,xoff,ooff,bn', [pytest.param(*c, id=c[0]) for c in CHAIN_CASES])
def test_pw_chain3(cid, wd, B, H, W, xoff, ooff, bn):
    """Each stored sp_i against ref_pw_chain3 (rounding points stated there); slice borders of the output buffer stay untouched."""
    from mgdt_yolo_amd import ops
    assert chain_nbk(wd) and ops.pw_chain_supported(wd, BF16)
    x, convs, gen = _chain_inputs(cid, wd, B, H, W, bn)
    pk = ops.PackedPwChain([c.dev_args() for c in convs], BF16)
    xv, _ = _nhwc(x, BF16, xoff, xoff, gen)
    out, big, big0 = _out_buf(B, 3 * wd, H, W, BF16, ooff, ooff, gen)
    ops.pw_chain3(xv, pk, ops.ACT_SILU, out)
    _check(out, ref_pw_chain3(x, convs), BF16, cid)
    _borders_untouched(big, big0, ooff, 3 * wd)


# ------------------------------------------------------------------------------------------------ csp_block
# (id, mode, wd, n, shortcut, want_pool, B, H, W, forced tile, cout, x offset, bn)
CSP_CASES = [
    ('mspa-wd8-n1-4x4-min-map', 0, 8, 1, True, True, 1, 4, 4, None, 32, 0, False),
    ('mspa-wd8-n2-8x12-tile2x3-cout20', 0, 8, 2, False, True, 3, 8, 12, (2, 3), 20, 0, False),
    ('mspa-wd16-n1-12x20-tile-half-map-6x10', 0, 16, 1, True, False, 1, 12, 20, (6, 10), 64, 0, False),
    ('mspa-wd16-n2-4x20-tile2x5-slice4-bn', 0, 16, 2, True, True, 3, 4, 20, (2, 5), 128, 4, True),
    ('mspa-wd32-n1-8x12-tile2x3', 0, 32, 1, False, True, 1, 8, 12, (2, 3), 128, 0, False),
    ('mspa-wd32-n2-20x40-tile10x20-lds-over-80k', 0, 32, 2, True, True, 1, 20, 40, (10, 20), 64, 0, False),
    ('mspa-wd64-n1-8x8-tile2x2-cout256', 0, 64, 1, True, True, 1, 8, 8, (2, 2), 256, 0, False),
    ('mspa-wd64-n1-12x12-cout48', 0, 64, 1, False, False, 3, 12, 12, None, 48, 4, False),
    ('c2f-wd16-n1-5x7-whole-map', 1, 16, 1, True, True, 1, 5, 7, None, 32, 0, False),
    ('c2f-wd16-n2-8x12-tile2x3-slice4', 1, 16, 2, False, False, 3, 8, 12, (2, 3), 64, 4, False),
    ('c2f-wd32-n1-8x12-tile2x2-cout20-bn', 1, 32, 1, False, True, 1, 8, 12, (2, 2), 20, 0, True),
    ('c2f-wd32-n2-16x24-tile8x24-lds-over-80k', 1, 32, 2, True, True, 1, 16, 24, (8, 24), 128, 0, False),
    ('c2f-wd64-n1-8x8-tile2x2', 1, 64, 1, True, False, 1, 8, 8, (2, 2), 128, 0, False),
    ('c2f-wd64-n2-6x10-cout256', 1, 64, 2, True, True, 3, 6, 10, None, 256, 0, False),
]


def _csp_inputs(cid, mode, wd, n, B, H, W, cout, bn):
    gen = _gen('csp', cid)
    cin = 4 * wd if mode == 0 else 2 * wd
    x = _rand(gen, B, cin, H, W, dt=BF16)
    front = [ConvP(gen, wd, wd, 1, bn=bn) for _ in range(3)] if mode == 0 else None
    mids = [ConvP(gen, wd, wd, 3, bn=bn) for _ in range(2 * n)]
    back = ConvP(gen, cout, (3 if mode == 0 else 2) * wd + n * wd, 1, bn=bn)
    return x, front, mids, back, gen


def _pool_ref(y, B, cout, H, W, th, tw, gst):
    """fp64 sums of the STORED y per (image, tile, slot, channel): tile pixel t = row * tw + col of tile (ty, tx) goes to slot (t // 16) % gst
    (the back phase: the waves that share a cout block take pixel groups gv, gv + gst, ...; pool[n][ty * tiles_x + tx][gv][c])."""
    ty, tx = H // th, W // tw
    yt = y.double().cpu().reshape(B, cout, ty, th, tx, tw).permute(0, 2, 4, 3, 5, 1).reshape(B, ty * tx, th * tw, cout)
    slot = (torch.arange(th * tw) // 16) % gst
    return torch.stack([yt[:, :, slot == s].sum(2) for s in range(gst)], 2)


@gpu
@pytest.mark.parametrize('cid,mode,wd,n,sc,pool,B,H,W,tile,cout,xoff,bn', [pytest.param(*c, id=c[0]) for c in CSP_CASES])
def test_csp_block(cid, mode, wd, n, sc, pool, B, H, W, tile, cout, xoff, bn):
    """y against ref_csp_block (rounding points stated there).  The pool output holds per-tile channel sums taken AFTER the bf16 rounding of y
    (psum adds the rounded accumulators), one slot per wave sharing a cout block: each slot is held to the fp64 sum of the kernel's own stored y
    under the fp32 bound; a slot no pixel group maps to must hold zeros.  Slot count and tile grid equal mgdt_csp_block_tiles."""
    from mgdt_yolo_amd import ops
    x, front, mids, back, gen = _csp_inputs(cid, mode, wd, n, B, H, W, cout, bn)
    th, tw, lds = csp_pick(mode, B, wd, n, H, W, tile)
    slots_c, g = _c_tiles(mode, B, x.shape[1], cout, wd, n, H, W, tile)
    assert (g[0], g[1], g[4]) == (th, tw, lds) and (tile is None or (th, tw) == tile)
    xv, _ = _nhwc(x, BF16, xoff, xoff, gen)
    chain = ops.PackedPwChain([c.dev_args() for c in front], BF16) if mode == 0 else None
    with _forced_tile(tile):
        assert ops.csp_block_supported(mode, xv, cout, wd, n, BF16)
        y, part, slots, tiles = ops.csp_block(mode, xv, chain.blob if chain else None, None, [m.pack() for m in mids], sc, back.pack(), wd,
                                              ops.ACT_SILU, cout, pool)
        torch.cuda.synchronize()
    _check(y, ref_csp_block(mode, x, front, mids, sc, back), BF16, cid)
    gst = csp_pool_gst(cout)
    assert slots == slots_c == (H // th) * (W // tw) * gst and tuple(tiles) == (W // tw, H // th) == (g[6], g[7])
    if not pool:
        assert part is None
        return
    _check(part.reshape(B, -1, gst, cout), _pool_ref(y, B, cout, H, W, th, tw, gst), F32, cid + ' pool')


@gpu
@pytest.mark.parametrize('what', ['odd-H', 'wd12', 'n3', 'fp32'])
def test_csp_block_refused(what):
    """Shapes outside mgdt_csp_block_supported raise: the C entry point checks them before it launches anything."""
    from mgdt_yolo_amd import ops
    wd, n, H, dt = {'odd-H': (8, 1, 5, BF16), 'wd12': (12, 1, 4, BF16), 'n3': (8, 3, 4, BF16), 'fp32': (8, 1, 4, F32)}[what]
    assert what == 'fp32' or not csp_supported(0, 4 * wd, 32, wd, n, H, 4)
    gen = _gen('csp-refused', what)
    x, _ = _nhwc(_rand(gen, 1, 4 * wd, H, 4, dt=dt), dt)
    # panels of a covered width: the call must be refused on its shapes alone, before anything reads them
    chain = ops.PackedPwChain([ConvP(gen, 8, 8, 1).dev_args() for _ in range(3)], BF16)
    mids = [ConvP(gen, 8, 8, 3).pack() for _ in range(2 * n)]
    back = ConvP(gen, 32, 40, 1).pack()
    assert not ops.csp_block_supported(0, x, 32, wd, n, dt)
    with pytest.raises(RuntimeError):
        ops.csp_block(0, x, chain.blob, None, mids, True, back, wd, ops.ACT_SILU, 32, False)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ conv1x1_inject(_conv)
# (id, cin, cout / cout2, B, H, W, Hg, Wg, bn, out offset)
INJ_CASES = [
    ('kc1-cout128-1to1', 8, 128, 2, 9, 20, 9, 20, False, 0), ('kc2-cin40-cout256-2to1', 40, 256, 1, 10, 36, 5, 18, False, 0),
    ('kc3-cout128-4to1', 72, 128, 1, 12, 40, 3, 10, False, 0), ('kc4-cout128-ragged-13x21-from-7x11', 128, 128, 2, 13, 21, 7, 11, False, 0),
    ('kc4-cout256-global-1x1', 128, 256, 3, 5, 7, 1, 1, False, 0), ('kc2-cout128-bn-out-slice', 64, 128, 1, 7, 33, 4, 9, True, 4),
    (f'kc1-2nd-round-{257 * 2}-patches-over-{INJ_CAP}', 8, 128, 1, 4 * 257, 17, 5, 3, False, 0),
]
# + gconv: the (gsrc, pkg) form
INJ2_CASES = [
    ('kc1-cout16-1to1-patch-limit-64', 8, 16, 2, 8, 8, 8, 8, False, 0, False), ('kc2-cin40-cout32-2to1', 40, 32, 1, 10, 36, 5, 18, False, 0, False),
    ('kc3-cout64-4to1', 72, 64, 1, 12, 40, 3, 10, False, 4, False), ('kc4-cout48-ragged-13x21-from-7x11', 128, 48, 2, 13, 21, 7, 11, False, 0, False),
    ('kc1-cout64-global-1x1', 16, 64, 3, 5, 7, 1, 1, True, 0, False), ('kc2-cout64-gconv-2to1-bn', 64, 64, 2, 12, 20, 6, 10, True, 0, True),
    ('kc1-cout32-gconv-ragged', 32, 32, 1, 13, 21, 7, 11, False, 4, True), ('kc1-cout16-gconv-global-1x1', 8, 16, 1, 9, 5, 1, 1, False, 0, True),
    (f'kc1-2nd-round-{129 * 2}-patches-over-{INJ2_CAP}', 8, 16, 1, 8 * 129, 17, 5, 3, False, 0, False),
]


def _inj_inputs(cid, cin, cmid, B, H, W, Hg, Wg, bn, gconv=False, cout2=0):
    """x, the local conv, the global maps as ONE (B, 2 cmid, Hg, Wg) buffer [ga | gf] (the gate spread over the saturating range of h_sigmoid),
    or the 32-channel source + merged panel of the GCONV form; the second conv when cout2."""
    gen = _gen('inj', cid)
    x = _rand(gen, B, cin, H, W, dt=BF16)
    pk = ConvP(gen, cmid, cin, 1, bn=bn)
    gaf = torch.cat([_rand(gen, B, cmid, Hg, Wg, dt=BF16, scale=3.0), _rand(gen, B, cmid, Hg, Wg, dt=BF16)], 1)
    gsrc, pkg = (_rand(gen, B, 32, Hg, Wg, dt=BF16), ConvP(gen, 2 * cmid, 32, 1, bn=bn, gain=2.0)) if gconv else (None, None)
    pk2 = ConvP(gen, cout2, cmid, 1, bn=bn, gain=2.0) if cout2 else None
    return x, pk, gaf, gsrc, pkg, pk2, gen


@gpu
@pytest.mark.parametrize('cid,cin,cout,B,H,W,Hg,Wg,bn,ooff', [pytest.param(*c, id=c[0]) for c in INJ_CASES])
def test_conv1x1_inject(cid, cin, cout, B, H, W, Hg, Wg, bn, ooff):
    """Against ref_inject: the local map is rounded to bf16 before the multiply (as the unfused pair stored it), nothing else; ga / gf are the
    two halves of one buffer, as the model passes them."""
    from mgdt_yolo_amd import ops
    x, pk, gaf, _, _, _, gen = _inj_inputs(cid, cin, cout, B, H, W, Hg, Wg, bn)
    gd, _ = _nhwc(gaf, BF16)
    ga, gf = gd[:, :cout], gd[:, cout:]
    xv, _ = _nhwc(x, BF16)
    assert inject_supported(cin, cout, H, W, Hg, Wg) and ops.conv1x1_inject_supported(xv, cout, ga, BF16)
    out, big, big0 = _out_buf(B, cout, H, W, BF16, ooff, ooff, gen)
    ops.conv1x1_inject(xv, pk.pack(), ga, gf, out=out)
    _check(out, ref_inject(x, pk, gaf[:, :cout], gaf[:, cout:]), BF16, cid)
    _borders_untouched(big, big0, ooff, cout)


@gpu
@pytest.mark.parametrize('cid,cin,cout2,B,H,W,Hg,Wg,bn,ooff,gconv', [pytest.param(*c, id=c[0]) for c in INJ2_CASES])
def test_conv1x1_inject_conv(cid, cin, cout2, B, H, W, Hg, Wg, bn, ooff, gconv):
    """Against ref_inject_conv: bf16(local map), bf16(injected map) feeding the second conv (its panel packed in acc_order_index order); the GCONV
    form in addition bf16(global maps), bf16(h_sigmoid(gate)) and bf16 tap weights (its interpolation is an MFMA)."""
    from mgdt_yolo_amd import ops
    x, pk, gaf, gsrc, pkg, pk2, gen = _inj_inputs(cid, cin, 256, B, H, W, Hg, Wg, bn, gconv, cout2)
    xv, _ = _nhwc(x, BF16)
    gd, _ = _nhwc(gaf, BF16)
    ga, gf = gd[:, :256], gd[:, 256:]
    assert inject_conv_supported(cin, 256, cout2, H, W, Hg, Wg) and ops.conv1x1_inject_conv_supported(xv, 256, cout2, ga, BF16)
    out, big, big0 = _out_buf(B, cout2, H, W, BF16, ooff, ooff, gen)
    p2 = pk2.pack(ops.acc_order_index(256, 'cpu'))
    if gconv:
        ops.conv1x1_inject_conv(xv, pk.pack(), None, None, p2, ops.ACT_SILU, out, gsrc=_nhwc(gsrc, BF16)[0], pkg=pkg.pack())
        ref = ref_inject_conv(x, pk, None, None, pk2, pkg=pkg, gsrc=gsrc)
    else:
        ops.conv1x1_inject_conv(xv, pk.pack(), ga, gf, p2, ops.ACT_SILU, out)
        ref = ref_inject_conv(x, pk, gaf[:, :256], gaf[:, 256:], pk2)
    _check(out, ref, BF16, cid)
    _borders_untouched(big, big0, ooff, cout2)


@gpu
def test_conv1x1_inject_conv_refused_beyond_the_patch_limit():
    """9 x 8 from 9 x 8: the first 8 x 16 workgroup's source patch is 9 x 8 = 72 > 64 pixels (8 x 8 from 8 x 8, exactly 64, is a case above)."""
    from mgdt_yolo_amd import ops
    assert inj_patch(8, 8, 8, 8, 8) == (8, 8) and inj_patch(9, 8, 9, 8, 8) == (9, 8) and not inject_conv_supported(8, 256, 16, 9, 8, 9, 8)
    x, pk, gaf, _, _, pk2, gen = _inj_inputs('refused', 8, 256, 1, 9, 8, 9, 8, False, False, 16)
    xv, gd = _nhwc(x, BF16)[0], _nhwc(gaf, BF16)[0]
    assert not ops.conv1x1_inject_conv_supported(xv, 256, 16, gd[:, :256], BF16)
    out = ops.new_act(1, 16, 9, 8, BF16, DEV)
    with pytest.raises(RuntimeError):
        ops.conv1x1_inject_conv(xv, pk.pack(), gd[:, :256], gd[:, 256:], pk2.pack(ops.acc_order_index(256, 'cpu')), ops.ACT_SILU, out)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ detect_tail
# (id, c2, c3, nc, B, H, W, a_off, a_extra, pk3, aug, best, feat offset)
TAIL_CASES = [
    ('c2-8-c3-8-nc4-5x7-scalar-flush-best', 8, 8, 4, 2, 5, 7, 3, 6, False, None, True, 0),
    ('c2-16-c3-40-nc20-aug-best', 16, 40, 20, 1, 6, 6, 0, 0, False, (0.83, False, 536.0), True, 0),
    ('c2-32-c3-128-nc80-aug-flip-feat-slice', 32, 128, 80, 2, 4, 9, 4, 4, False, (0.67, True, 640.0), False, 4),
    (f'c3-128-nc176-lds-{tail_lds(128, 176)}-below-64k', 16, 128, 176, 1, 3, 11, 0, 3, False, None, False, 0),
    (f'c3-128-nc192-lds-{tail_lds(128, 192)}-above-64k', 16, 128, 192, 1, 3, 11, 2, 0, False, None, False, 0),
    ('c2-8-c3-40-nc256', 8, 40, 256, 1, 2, 17, 0, 0, False, None, False, 0),
    ('pk3-bn-7x9-a-off-best', 16, 40, 20, 2, 7, 9, 5, 2, True, None, True, 0),
    ('pk3-aug-flip-8x4', 16, 8, 4, 1, 8, 4, 0, 0, True, (0.83, True, 536.0), False, 4),
    (f'2nd-round-{2 * 2064}-units-over-{TAIL_CAP_UNITS}', 8, 8, 4, 2, 256, 258, 0, 0, False, None, False, 0),
]


def _top2_gap_ok(cls):
    """Every anchor's two largest class logits differ by more than two bf16 ulps of the larger magnitude."""
    top = cls.topk(2, 1).values
    ulp = torch.exp2(torch.floor(torch.log2(top.abs().max(1).values.clamp_min(1e-30))) - 7)
    return bool(((top[:, 0] - top[:, 1]) > 2 * ulp).all())


def _tail_inputs(cid, c2, c3, nc, B, H, W, pk3, best):
    """Box logits x 3 (peaked and flat DFL sides both occur).  With best keys the class input is redrawn (salt 0, 1, ...) until _top2_gap_ok
    holds for the reference map: then no bf16 rounding of a logit can change an anchor's argmax."""
    gen = _gen('tail', cid)
    tb = _rand(gen, B, c2, H, W, dt=BF16)
    p3 = ConvP(gen, 16, 16, 3, bn=True, gain=2.0) if pk3 else None
    pkb, pkc = ConvP(gen, 16, c2, 1, gain=3.0), ConvP(gen, nc, c3, 1, gain=2.0)
    for salt in range(2000):
        tc = _rand(_gen('tail-tc', cid, salt), B, c3, H, W, dt=BF16)
        if not best or _top2_gap_ok(pkc(tc, F64)):
            return tb, tc, pkb, pkc, p3, gen
    raise AssertionError(('no class input with separated top-2 logits', cid))


def _pack_box_after_3x3(pkb):
    """The final 1x1 over the in-launch 3x3 conv's accumulators: 32 zero-padded input channels in acc_order_index order (head.py _box3_in_tail)."""
    from mgdt_yolo_amd import ops
    wp = torch.zeros(16, 32)
    wp[:, :16] = pkb.w.reshape(16, 16)
    return ops.PackedConv(wp[:, ops.acc_order_index(32, 'cpu')].reshape(16, 32, 1, 1).to(DEV), pkb.cb.to(DEV), None, 1, BF16)


@gpu
@pytest.mark.parametrize('cid,c2,c3,nc,B,H,W,a_off,extra,pk3,aug,best,foff', [pytest.param(*c, id=c[0]) for c in TAIL_CASES])
def test_detect_tail(cid, c2, c3, nc, B, H, W, a_off, extra, pk3, aug, best, foff):
    """Stage 1: the raw bf16 map against ref_detect_map (with pk3: bf16(silu(conv3x3)) in front of the box conv) under the bf16 bound.
    Stage 2: y (fp32) against the fp64 decode of the map the kernel wrote - the kernel decodes the ROUNDED logits - under the fp32 bound, boxes
    and scores separately; columns outside [a_off, a_off + HW) stay untouched.  Best keys: class = first maximal logit of the read-back map,
    score bits = the stored score, anchor = a_off + index; keys of other anchors stay untouched."""
    from mgdt_yolo_amd import ops
    tb, tc, pkb, pkc, p3, gen = _tail_inputs(cid, c2, c3, nc, B, H, W, pk3, best)
    tbv, tcv = _nhwc(tb, BF16)[0], _nhwc(tc, BF16)[0]
    assert tail_supported(c2, c3, nc) and ops.detect_tail_supported(tbv, tcv, nc, 4, BF16)
    A, stride = H * W, 8.0
    a_total = a_off + A + extra
    feat, fbig, fbig0 = _out_buf(B, 16 + nc, H, W, BF16, foff, foff, gen)
    y0 = torch.randn(B, 4 + nc, a_total, generator=gen)
    y = y0.to(DEV)
    k0 = torch.randint(0, 2 ** 62, (B, a_total), generator=gen, dtype=torch.int64)
    keys = k0.to(DEV)
    ops.detect_tail(tbv, tcv, _pack_box_after_3x3(pkb) if pk3 else pkb.pack(), pkc.pack(), nc, stride, a_off, feat, y, keys if best else None,
                    pk3=p3.pack() if pk3 else None, aug=aug)
    ref = ref_detect_map(tb, tc, pkb, pkc, p3)
    _check(feat[:, :16], ref[:, :16], BF16, cid + ' box logits')
    _check(feat[:, 16:], ref[:, 16:], BF16, cid + ' class logits')
    _borders_untouched(fbig, fbig0, foff, 16 + nc)
    fm = feat.float().cpu().double()
    got = y.cpu()
    yr = ref_detect_decode(fm, nc, stride, aug)
    _check(got[:, :4, a_off:a_off + A], yr[:, :4], F32, cid + ' boxes')
    _check(got[:, 4:, a_off:a_off + A], yr[:, 4:], F32, cid + ' scores')
    assert torch.equal(got[:, :, :a_off], y0[:, :, :a_off]) and torch.equal(got[:, :, a_off + A:], y0[:, :, a_off + A:]), 'other anchors written'
    kk = keys.cpu()
    if not best:
        assert torch.equal(kk, k0)
        return
    cls = fm[:, 16:].reshape(B, nc, A).numpy().argmax(1)
    sc = np.take_along_axis(got[:, 4:, a_off:a_off + A].numpy(), cls[:, None], 1)[:, 0]
    anchor = np.arange(a_off, a_off + A, dtype=np.uint64)[None]
    key = ((np.uint64(0xFFFFFFFF) - sc.view(np.uint32).astype(np.uint64)) << np.uint64(32)) | (anchor * np.uint64(nc) + cls.astype(np.uint64))
    assert np.array_equal(kk[:, a_off:a_off + A].numpy().view(np.uint64), key), 'best-class keys'
    assert torch.equal(kk[:, :a_off], k0[:, :a_off]) and torch.equal(kk[:, a_off + A:], k0[:, a_off + A:]), 'other keys written'


@gpu
def test_detect_tail_refused_nc6():
    from mgdt_yolo_amd import ops
    gen = _gen('tail-refused')
    tb, tc = _nhwc(_rand(gen, 1, 8, 3, 3, dt=BF16), BF16)[0], _nhwc(_rand(gen, 1, 8, 3, 3, dt=BF16), BF16)[0]
    assert not tail_supported(8, 8, 6) and not ops.detect_tail_supported(tb, tc, 6, 4, BF16)
    feat, y = ops.new_act(1, 22, 3, 3, BF16, DEV), torch.zeros(1, 10, 9, device=DEV)
    with pytest.raises(RuntimeError):
        ops.detect_tail(tb, tc, ConvP(gen, 16, 8, 1).pack(), ConvP(gen, 8, 8, 1).pack(), 6, 8.0, 0, feat, y)
    torch.cuda.synchronize()
    assert y.abs().max().item() == 0


# ------------------------------------------------------------------------------------------------ conv2d beyond its grid cap
@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('k', [1, 3], ids=lambda k: f'k{k}-2nd-round-{260 * 260}-rows-over-{CONV_CAP_ROWS}')
def test_conv2d_second_round(k, dt):
    """mgdt_conv2d_fwd caps its grid at 256 workgroups of 256 output rows: at 1 x 260 x 260 a workgroup takes a second row block."""
    import torch.nn.functional as F
    from mgdt_yolo_amd import ops
    assert 260 * 260 > CONV_CAP_ROWS
    gen = _gen('conv-2nd', k, str(dt))
    x = _rand(gen, 1, 8, 260, 260, dt=dt)
    p = ConvP(gen, 8, 8, k)
    w, cb, _ = p.dev_args()
    y = ops.conv2d(_nhwc(x, dt)[0], ops.PackedConv(w, cb, None, k, dt), 1, ops.ACT_SILU)
    _check(y, F.silu(F.conv2d(x, p.w.double(), p.cb.double(), 1, k // 2)), dt, f'k{k}')


# ------------------------------------------------------------------------------------------------ host only
def test_route_predicates():
    """Host only.  The Python predicates above against the C ones for every case (and the refused shapes), and each case's route facts: the
    forced tiles' properties, LDS thresholds, the second-round thresholds derived from the launch caps."""
    from mgdt_yolo_amd import _lib
    lib = _lib.lib()
    # pw_chain
    for wd in range(0, 72, 4):
        assert (lib.mgdt_pw_chain_packed_bytes(wd, _lib.BF16) > 0) == bool(chain_nbk(wd)), wd
    assert lib.mgdt_pw_chain_packed_bytes(10, _lib.BF16) == 0 and lib.mgdt_pw_chain_packed_bytes(16, _lib.F32) == 0
    assert sorted({chain_nbk(c[1]) for c in CHAIN_CASES}) == [1, 2, 4] and any(c[1] % 16 for c in CHAIN_CASES)
    assert [c for c in CHAIN_CASES if c[2] * c[3] * c[4] > chain_second_round_pixels(c[1])] == [CHAIN_CASES[-1]]
    assert any((c[2] * c[3] * c[4]) % 64 for c in CHAIN_CASES)
    # csp_block
    seen = set()
    for cid, mode, wd, n, sc, pool, B, H, W, tile, cout, xoff, bn in CSP_CASES:
        cin = 4 * wd if mode == 0 else 2 * wd
        assert csp_supported(mode, cin, cout, wd, n, H, W) and lib.mgdt_csp_block_supported(mode, cin, cout, wd, n, H, W, _lib.BF16), cid
        th, tw, lds = csp_pick(mode, B, wd, n, H, W, tile)
        slots, g = _c_tiles(mode, B, cin, cout, wd, n, H, W, tile)
        assert (g[0], g[1], g[4]) == (th, tw, lds) and slots == (H // th) * (W // tw) * csp_pool_gst(cout), (cid, g)
        assert (lds > 80 * 1024) == ('lds-over-80k' in cid), (cid, lds)
        seen.add((mode, wd))
        seen.update([('n', n), ('sc', sc), ('pool', pool), ('B', B), ('xoff', xoff), ('gst>1', csp_pool_gst(cout) > 1), ('cout%16', cout % 16 != 0),
                     ('partial', th * tw % 16 != 0), ('whole', (th, tw) == ((H // 2, W // 2) if mode == 0 else (H, W))),
                     ('halo>=tile', 2 * n >= max(th, tw))])
    for mode, wds in ((0, (8, 16, 32, 64)), (1, (16, 32, 64))):
        assert all((mode, wd) in seen for wd in wds)
    for fact in [('n', 1), ('n', 2), ('sc', True), ('sc', False), ('pool', True), ('pool', False), ('B', 1), ('B', 3), ('xoff', 4), ('gst>1', True),
                 ('gst>1', False), ('cout%16', True), ('partial', True), ('whole', True), ('halo>=tile', True)]:
        assert fact in seen, fact
    for mode, cin, cout, wd, n, H, W in [(0, 32, 32, 8, 1, 5, 4), (0, 48, 32, 12, 1, 4, 4), (0, 32, 32, 8, 3, 4, 4), (0, 32, 30, 8, 1, 4, 4),
                                         (0, 256, 64, 64, 2, 8, 8), (1, 16, 32, 8, 1, 8, 8), (0, 32, 32, 8, 1, 2, 4), (1, 64, 32, 32, 1, 37, 37)]:
        ok = csp_supported(mode, cin, cout, wd, n, H, W)
        assert ok == bool(lib.mgdt_csp_block_supported(mode, cin, cout, wd, n, H, W, _lib.BF16)), (mode, wd, n, H, W)
        assert (ok and csp_pick(mode, 1, wd, n, H, W) is not None) == (lib.mgdt_csp_block_tiles(mode, 1, cin, cout, wd, n, H, W, None) > 0)
    assert not lib.mgdt_csp_block_supported(0, 32, 32, 8, 1, 4, 4, _lib.F32)
    # inject / inject_conv
    for cid, cin, cout, B, H, W, Hg, Wg, bn, ooff in INJ_CASES:
        assert inject_supported(cin, cout, H, W, Hg, Wg) and lib.mgdt_conv1x1_inject_supported(cin, cout, H, W, Hg, Wg, _lib.BF16), cid
    assert sorted({inj_kc(c[1]) for c in INJ_CASES}) == [1, 2, 3, 4] and {c[2] for c in INJ_CASES} == {128, 256} and any(c[1] % 32 for c in INJ_CASES)
    assert [c for c in INJ_CASES if c[3] * -(-c[4] // 4) * -(-c[5] // 16) > INJ_CAP] == [INJ_CASES[-1]]
    for cid, cin, cout2, B, H, W, Hg, Wg, bn, ooff, gconv in INJ2_CASES:
        assert inject_conv_supported(cin, 256, cout2, H, W, Hg, Wg) and lib.mgdt_conv1x1_inject_conv_supported(cin, 256, cout2, H, W, Hg, Wg, _lib.BF16), cid
    assert sorted({inj_kc(c[1]) for c in INJ2_CASES}) == [1, 2, 3, 4] and {c[2] for c in INJ2_CASES} == {16, 32, 48, 64}
    assert [c for c in INJ2_CASES if c[3] * -(-c[4] // 8) * -(-c[5] // 16) > INJ2_CAP] == [INJ2_CASES[-1]]
    ph, pw = inj_patch(8, 8, 8, 8, 8)
    assert ph * pw == 64
    for args in [(8, 128, 9, 20, 9, 20), (8, 256, 9, 20, 9, 20), (8, 64, 9, 20, 9, 20), (12, 128, 8, 8, 4, 4), (8, 128, 4, 4, 8, 8), (136, 128, 8, 8, 4, 4),
                 (128, 256, 64, 64, 64, 64)]:
        assert inject_supported(*args) == bool(lib.mgdt_conv1x1_inject_supported(*args, _lib.BF16)), args
    for args in [(8, 256, 16, 9, 8, 9, 8), (8, 256, 16, 8, 8, 8, 8), (8, 128, 16, 8, 8, 4, 4), (8, 256, 80, 8, 8, 4, 4), (8, 256, 24, 8, 8, 4, 4),
                 (8, 256, 64, 40, 40, 20, 20), (8, 256, 64, 40, 40, 40, 40), (128, 256, 64, 80, 80, 20, 20)]:
        assert inject_conv_supported(*args) == bool(lib.mgdt_conv1x1_inject_conv_supported(*args, _lib.BF16)), args
    # detect_tail
    for cid, c2, c3, nc, *_ in TAIL_CASES:
        assert tail_supported(c2, c3, nc) and lib.mgdt_detect_tail_supported(c2, c3, nc, 4, _lib.BF16), cid
    for args in [(8, 8, 6, 4), (8, 8, 4, 16), (12, 8, 4, 4), (40, 8, 4, 4), (8, 136, 4, 4), (8, 8, 260, 4), (8, 8, 0, 4)]:
        assert tail_supported(*args) == bool(lib.mgdt_detect_tail_supported(*args, _lib.BF16)), args
    assert {c[1] for c in TAIL_CASES} == {8, 16, 32} and {(c[2] + 31) // 32 for c in TAIL_CASES} == {1, 2, 4}
    assert {4, 20, 80, 256} <= {c[3] for c in TAIL_CASES} and {1, 2, 5, 16} <= {(c[3] + 15) // 16 for c in TAIL_CASES}
    assert tail_lds(128, 176) < 64 * 1024 < tail_lds(128, 192) and tail_lds(128, 256) <= 150 * 1024
    assert [c for c in TAIL_CASES if c[4] * -(-c[5] * c[6] // 32) > TAIL_CAP_UNITS] == [TAIL_CASES[-1]]
    assert any((c[5] * c[6]) % 32 for c in TAIL_CASES)


def _sound(f32, f64, what):
    _check(f32, f64, BF16, what + ' fp32 restatement')


@pytest.mark.parametrize('cid,wd,B,H,W,xoff,ooff,bn', [pytest.param(*c, id=c[0]) for c in CHAIN_CASES[:-1]])
def test_restatement_soundness_pw_chain3(cid, wd, B, H, W, xoff, ooff, bn):
    """Host only: ref_pw_chain3 in fp32 within the bf16 bound of its fp64 evaluation."""
    x, convs, _ = _chain_inputs(cid, wd, B, H, W, bn)
    _sound(ref_pw_chain3(x, convs, F32), ref_pw_chain3(x, convs), cid)


@pytest.mark.parametrize('cid,mode,wd,n,sc,pool,B,H,W,tile,cout,xoff,bn', [pytest.param(*c, id=c[0]) for c in CSP_CASES])
def test_restatement_soundness_csp_block(cid, mode, wd, n, sc, pool, B, H, W, tile, cout, xoff, bn):
    """Host only: ref_csp_block in fp32 within the bf16 bound of its fp64 evaluation."""
    x, front, mids, back, _ = _csp_inputs(cid, mode, wd, n, B, H, W, cout, bn)
    _sound(ref_csp_block(mode, x, front, mids, sc, back, F32), ref_csp_block(mode, x, front, mids, sc, back), cid)


@pytest.mark.parametrize('cid,cin,cout2,B,H,W,Hg,Wg,bn,ooff,gconv', [pytest.param(*c, id=c[0]) for c in INJ2_CASES[:-1]])
def test_restatement_soundness_inject(cid, cin, cout2, B, H, W, Hg, Wg, bn, ooff, gconv):
    """Host only: ref_inject and ref_inject_conv (both forms) in fp32 within the bf16 bound of their fp64 evaluation; the stated four-tap
    association equals F.interpolate(bilinear, align_corners=False) in fp64 up to the fp32 tap weights."""
    import torch.nn.functional as F
    x, pk, gaf, gsrc, pkg, pk2, _ = _inj_inputs(cid, cin, 256, B, H, W, Hg, Wg, bn, gconv, cout2)
    ga, gf = (None, None) if gconv else (gaf[:, :256], gaf[:, 256:])
    _sound(ref_inject(x, pk, ga, gf, F32, pkg, gsrc), ref_inject(x, pk, ga, gf, F64, pkg, gsrc), cid + ' inject')
    _sound(ref_inject_conv(x, pk, ga, gf, pk2, F32, pkg, gsrc), ref_inject_conv(x, pk, ga, gf, pk2, F64, pkg, gsrc), cid + ' inject_conv')
    want = F.interpolate(gaf, size=(H, W), mode='bilinear', align_corners=False)
    assert (inj_bilinear(gaf, H, W) - want).abs().max().item() <= 4e-6 * gaf.abs().max().item()


@pytest.mark.parametrize('cid,c2,c3,nc,B,H,W,a_off,extra,pk3,aug,best,foff', [pytest.param(*c, id=c[0]) for c in TAIL_CASES[:-1]])
def test_restatement_soundness_detect_tail(cid, c2, c3, nc, B, H, W, a_off, extra, pk3, aug, best, foff):
    """Host only: ref_detect_map in fp32 within the bf16 bound of its fp64 evaluation; with best keys the reference's two largest class logits
    differ by more than two bf16 ulps at every anchor, so no anchor has to be excluded from the key comparison."""
    tb, tc, pkb, pkc, p3, _ = _tail_inputs(cid, c2, c3, nc, B, H, W, pk3, best)
    ref = ref_detect_map(tb, tc, pkb, pkc, p3)
    _sound(ref_detect_map(tb, tc, pkb, pkc, p3, F32), ref, cid)
    if best:
        assert _top2_gap_ok(ref[:, 16:])
