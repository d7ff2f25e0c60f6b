"""csp_block_kernel's 3x3 convs walk only the pixels of their output rectangle: the 16-pixel groups are formed over the rectangle's pixels in
row-major order instead of over the linear region range that also covers the wrap-around columns (GPU, -m gpu).  The linear walk stays reachable
(MGDT_CSP_COMPACT=0, read per call, so one process compares the two).  Every needed pixel goes through the same MFMAs in the same order and is
rounded at the same points, so y and the pool sums are compared bit for bit, and the compact form is held to ref_csp_block under the bf16 bound
of kernel_ref._close.  The cases also run the fragment requests that the wide convs (wd 32 / 64) now issue in front of the barrier that ends a
conv, and the last conv's copy of the conv code; those have no knob of their own and change no arithmetic.

Shapes: the smallest at which the walk can go wrong, with forced tiles.  Rectangle widths that are no multiple of 16 (groups straddle rows, the
last group is partial), fewer groups than waves, interior and border tiles, a halo wider than the tile, the swizzled maps of wd 32 ((pix >> 1) & 3)
and wd 64 (pix & 7) whose XOR term is re-formed per group, one workgroup per CU (wd 64), C2f without shortcut, and an x view inside a wider buffer.
"""
import pytest
import torch

from kernel_ref import BF16, ConvP, _check, _gen, _nhwc, _rand, ref_csp_block
from test_csp_block_lean import _run_csp

gpu = pytest.mark.gpu


def _inputs(cid, mode, wd, n, B, H, W, cout):
    gen = _gen('csp-compact', cid)
    x = _rand(gen, B, 4 * wd if mode == 0 else 2 * wd, H, W, dt=BF16)
    front = [ConvP(gen, wd, wd, 1) for _ in range(3)] if mode == 0 else None
    mids = [ConvP(gen, wd, wd, 3) for _ in range(2 * n)]
    back = ConvP(gen, cout, (3 if mode == 0 else 2) * wd + n * wd, 1)
    return x, front, mids, back, gen


# (id, mode, wd, n, shortcut, B, H, W, forced tile, cout, x offset).  Output rectangles of the 3x3 convs (conv j: (RH - 2j - 2) x (RW - 2j - 2)):
#   wd 8  32x32 tile 16x16 n 1 : 18x18 = 324 px (20.25 groups) and 16x16; rows of 18 straddle the groups of 16
#   wd 8  4x4 whole map        : tile 2x2, 4x4 = 16 px and 2x2 = 4 px: one group, seven waves idle, 12 clamped lanes
#   wd 16 48x48 tile 8x8 n 2   : 14x14, 12x12, 10x10, 8x8; 36 tiles, interior and border; tocat stores; cout 20 = a ragged last cout block
#   wd 32 12x12 tile 2x3 n 2   : region 10x11, halo 4 > tile, every tile on the border
#   wd 32 40x40 tile 10x10 n 2 : the bench tile (region 18x18)
#   wd 64 20x20 tile 5x10, 5x5 : region 9x14 / 9x9, one workgroup per CU
#   C2f wd 32 24x24 tile 8x12  : no shortcut, no pool; once as channels [4, 68) of a 72-channel buffer
CASES = [
    ('wd8-32x32-tile16x16-n1-B2', 0, 8, 1, True, 2, 32, 32, (16, 16), 32, 0),
    ('wd8-4x4-min-map-n1', 0, 8, 1, True, 1, 4, 4, None, 32, 0),
    ('wd16-48x48-tile8x8-n2-shortcut-cout20', 0, 16, 2, True, 1, 48, 48, (8, 8), 20, 0),
    ('wd32-12x12-tile2x3-n2-B2', 0, 32, 2, True, 2, 12, 12, (2, 3), 128, 0),
    ('wd32-40x40-tile10x10-n2-B1', 0, 32, 2, True, 1, 40, 40, (10, 10), 128, 0),
    ('wd64-20x20-tile5x10-n1-B2', 0, 64, 1, True, 2, 20, 20, (5, 10), 256, 0),
    ('wd64-20x20-tile5x5-n1-B1', 0, 64, 1, True, 1, 20, 20, (5, 5), 256, 0),
    ('c2f-wd32-24x24-tile8x12-n1-B2', 1, 32, 1, False, 2, 24, 24, (8, 12), 64, 0),
    ('c2f-wd32-24x24-tile8x12-n1-slice4', 1, 32, 1, False, 1, 24, 24, (8, 12), 64, 4),
]


@gpu
@pytest.mark.parametrize('cid,mode,wd,n,sc,B,H,W,tile,cout,xoff', [pytest.param(*c, id=c[0]) for c in CASES])
def test_compact_walk_equals_linear_walk(cid, mode, wd, n, sc, B, H, W, tile, cout, xoff):
    x, front, mids, back, gen = _inputs(cid, mode, wd, n, B, H, W, cout)
    xv, _ = _nhwc(x, BF16, xoff, xoff, gen)
    yb1, pb1, y1 = _run_csp(mode, xv, front, mids, sc, back, wd, cout, tile, MGDT_CSP_COMPACT=None)
    yb0, pb0, _ = _run_csp(mode, xv, front, mids, sc, back, wd, cout, tile, MGDT_CSP_COMPACT='0')
    assert torch.equal(yb1, yb0), (cid, 'y differs in', int((yb1 != yb0).sum()), 'elements')
    if mode == 0:
        assert torch.equal(pb1, pb0), (cid, 'pool sums differ in', int((pb1 != pb0).sum()), 'elements')
    else:
        assert pb1 is None and pb0 is None
    _check(y1, ref_csp_block(mode, x, front, mids, sc, back), BF16, cid)


# one Inf in one pixel of image 1: a pixel group of the compact walk holds other pixels than the linear walk's group does, but an MFMA column is
# one pixel, so the set of non-finite outputs and every other bit must be the linear walk's.  wd 8 = the paired epilogue, wd 32 = a swizzled map.
INF_CASES = [(CASES[0], (1, 5, 9, 11)), (CASES[3], (1, 40, 5, 7))]


@gpu
@pytest.mark.parametrize('case,at', [pytest.param(c, at, id=c[0]) for c, at in INF_CASES])
def test_compact_inf_pixel_stays_where_the_linear_walk_has_it(case, at):
    cid, mode, wd, n, sc, B, H, W, tile, cout, _ = case
    x, front, mids, back, gen = _inputs(cid + '-inf', mode, wd, n, B, H, W, cout)
    x[at] = float('inf')
    xv, _ = _nhwc(x, BF16)
    yb1, pb1, y1 = _run_csp(mode, xv, front, mids, sc, back, wd, cout, tile, MGDT_CSP_COMPACT=None)
    yb0, pb0, y0 = _run_csp(mode, xv, front, mids, sc, back, wd, cout, tile, MGDT_CSP_COMPACT='0')
    bad1, bad0 = ~torch.isfinite(y1.float().cpu()), ~torch.isfinite(y0.float().cpu())
    print('non-finite outputs: compact', int(bad1.sum()), 'linear', int(bad0.sum()))
    assert bad0.any() and not bad0[0].any(), 'the Inf must reach image 1 and only image 1'
    assert torch.equal(bad1, bad0), ('non-finite sets differ in', int((bad1 != bad0).sum()), 'elements')
    ok = ~bad0
    assert torch.equal(yb1[ok], yb0[ok])
    assert torch.equal(pb1.reshape(B, -1)[0], pb0.reshape(B, -1)[0])
