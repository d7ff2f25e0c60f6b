"""csp_block_kernel<8, MSPA> runs one epilogue for two pixel groups: with wd = 8 a 16-row MFMA block carries 8 real output channels, so the
accumulators of two groups are merged (v_permlane32_swap) and SiLU, rounding and the LDS stores run once with every lane live (GPU, -m gpu).
The unpaired form stays reachable (MGDT_CSP_PAIR=0, read per call, so one process compares the two): both forms run the same MFMAs and round at
the same points, so y and the pool sums are compared bit for bit, and the paired form is held to ref_csp_block under the bf16 bound of
kernel_ref._close.
"""
import pytest
import torch

from kernel_ref import BF16, ConvP, _check, _gen, _nhwc, _rand, ref_csp_block
from knobs import knobs as _env

gpu = pytest.mark.gpu


def _bits(t):
    """Bit pattern of a device tensor on the CPU: NaN compares equal to the same NaN, -0 differs from +0."""
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def _csp_inputs(cid, mode, wd, n, B, H, W, cout):
    gen = _gen('csp-lean', cid)
    cin = 4 * wd if mode == 0 else 2 * wd
    x = _rand(gen, B, cin, H, W, dt=BF16)
    front = [ConvP(gen, wd, wd, 1) for _ in range(3)] if mode == 0 else None
    mids = [ConvP(gen, wd, wd, 3) for _ in range(2 * n)]
    back = ConvP(gen, cout, (3 if mode == 0 else 2) * wd + n * wd, 1)
    return x, front, mids, back, gen


def _run_csp(mode, xv, front, mids, sc, back, wd, cout, tile, **env):
    """One launch under the given knobs -> (bits of y, bits of the pool sums or None, y)."""
    from mgdt_yolo_amd import ops
    chain = ops.PackedPwChain([c.dev_args() for c in front], BF16) if mode == 0 else None
    knobs = dict(MGDT_CSP_PAIR=None, MGDT_CSP_TILE=f'{tile[0]},{tile[1]}' if tile else None)
    knobs.update(env)
    with _env(**knobs):
        assert ops.csp_block_supported(mode, xv, cout, wd, len(mids) // 2, BF16)
        y, part, _, tiles = ops.csp_block(mode, xv, chain.blob if chain else None, None, [m.pack() for m in mids], sc, back.pack(), wd, ops.ACT_SILU,
                                          cout, mode == 0)
        torch.cuda.synchronize()
    if tile:
        assert tuple(tiles) == (xv.shape[3] // tile[1], xv.shape[2] // tile[0])
    return _bits(y), None if part is None else _bits(part), y


# (id, n, shortcut, B, H, W, forced tile, cout, x offset).  Groups per phase (16 pixels each, 8 waves):
#   32x32 tile 16x16 n 1: region 20x20 = 25 groups (wave 0: two pairs, waves 1-7: a pair and a single); conv0 23 groups (waves 0-6: a pair, then
#                         a single without a second group; wave 7: one pair)
#   48x48 tile 8x8 n 2  : interior and border tiles, tocat stores from merged lanes, cout 20 (ragged last cout block)
#   4x4 whole map n 1   : tile 2x2, region 6x6 = 3 groups: fewer groups than waves
PAIR_CASES = [
    ('32x32-tile16x16-n1-B2', 1, False, 2, 32, 32, (16, 16), 32, 0),
    ('48x48-tile8x8-n2-shortcut-cout20', 2, True, 1, 48, 48, (8, 8), 20, 0),
    ('4x4-min-map-n1', 1, True, 1, 4, 4, None, 32, 0),
    ('8x12-tile2x3-n2-slice4-B3', 2, True, 3, 8, 12, (2, 3), 32, 4),
]


@gpu
@pytest.mark.parametrize('cid,n,sc,B,H,W,tile,cout,xoff', [pytest.param(*c, id=c[0]) for c in PAIR_CASES])
def test_paired_equals_unpaired(cid, n, sc, B, H, W, tile, cout, xoff):
    x, front, mids, back, gen = _csp_inputs(cid, 0, 8, n, B, H, W, cout)
    xv, _ = _nhwc(x, BF16, xoff, xoff, gen)
    yb1, pb1, y1 = _run_csp(0, xv, front, mids, sc, back, 8, cout, tile)
    yb0, pb0, _ = _run_csp(0, xv, front, mids, sc, back, 8, cout, tile, MGDT_CSP_PAIR='0')
    assert torch.equal(yb1, yb0), (cid, 'y differs in', int((yb1 != yb0).sum()), 'elements')
    assert torch.equal(pb1, pb0), (cid, 'pool sums differ in', int((pb1 != pb0).sum()), 'elements')
    _check(y1, ref_csp_block(0, x, front, mids, sc, back), BF16, cid)


@gpu
def test_paired_inf_pixel_stays_where_the_unpaired_form_has_it():
    """One Inf in one pixel of image 1: the paired front holds the neighbouring group (the pixel 16 region positions away) in the other half of the
    same registers.  Its B operands keep real zeros there, so the non-finite outputs are exactly those of the unpaired form, and every other
    element keeps its bits."""
    cid, n, sc, B, H, W, tile, cout, _ = PAIR_CASES[0]
    x, front, mids, back, gen = _csp_inputs(cid + '-inf', 0, 8, n, B, H, W, cout)
    x[1, 5, 9, 11] = float('inf')
    xv, _ = _nhwc(x, BF16)
    yb1, pb1, y1 = _run_csp(0, xv, front, mids, sc, back, 8, cout, tile)
    yb0, pb0, y0 = _run_csp(0, xv, front, mids, sc, back, 8, cout, tile, MGDT_CSP_PAIR='0')
    bad1, bad0 = ~torch.isfinite(y1.float().cpu()), ~torch.isfinite(y0.float().cpu())
    print('non-finite outputs: paired', int(bad1.sum()), 'unpaired', int(bad0.sum()))
    assert bad0.any() and not bad0[0].any(), 'the Inf must reach image 1 and only image 1'
    assert torch.equal(bad1, bad0), ('non-finite sets differ in', int((bad1 != bad0).sum()), 'elements')
    ok = ~bad0
    assert torch.equal(yb1[ok], yb0[ok])
    assert torch.equal(pb1.reshape(B, -1)[0], pb0.reshape(B, -1)[0])
