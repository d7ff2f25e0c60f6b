"""Tile geometry of the whole-block CSP kernel (mgdt_csp_block_fwd): LDS per workgroup at the bench shapes (host only), and the
single launch against the per-conv launch chain at the bench shapes and at forced tiles of both residencies (GPU)."""
import ctypes as C

import pytest
import torch

from knobs import forced_tile
from mgdt_yolo_amd import _lib
from mgdt_yolo_amd.seeding import seed_state_dict_

DEV = 'cuda:0'
LDS_2WG = 80 * 1024          # two workgroups per CU (160 KiB of LDS)

# the five blocks of the bench model (n scale, 640x640): (mode, block width c, bottlenecks, map size); mode 0 = MSPA_C2f, 1 = C2f (c2 = 64)
BENCH = [(0, 32, 1, 160), (0, 64, 2, 80), (0, 128, 2, 40), (0, 256, 1, 20), (1, 64, 1, 80)]


def _tiles(mode, n, c, nbtl, hw, tile=None):
    """(slots, geom8) of mgdt_csp_block_tiles for a block of width c (wd = c/4 for MSPA, c/2 for C2f)."""
    wd = c // 4 if mode == 0 else c // 2
    cin = 4 * wd if mode == 0 else 2 * wd
    g = (C.c_int * 8)()
    with forced_tile(tile):
        slots = _lib.lib().mgdt_csp_block_tiles(mode, n, cin, c, wd, nbtl, hw, hw, g)
    return slots, list(g)


@pytest.mark.parametrize('mode,c,nbtl,hw', BENCH)
def test_bench_blocks_fit_two_workgroups_per_cu(mode, c, nbtl, hw):
    """Host only.  At B = 32 the picked tile of every block whose registers allow two workgroups per CU (wd <= 32) needs at most
    80 KiB of LDS; wd = 64 (more than 128 VGPRs, one workgroup per CU) keeps its 5x10 tile."""
    slots, g = _tiles(mode, 32, c, nbtl, hw)
    wd = c // 4 if mode == 0 else c // 2
    assert slots > 0
    th, tw, lds = g[0], g[1], g[4]
    assert (hw // 2 if mode == 0 else hw) % th == 0 and (hw // 2 if mode == 0 else hw) % tw == 0
    assert g[5] == 32 * g[6] * g[7] and g[6] * tw == hw and g[7] * th == hw
    if wd <= 32:
        assert lds <= LDS_2WG, (th, tw, lds)
    else:
        assert (th, tw) == (5, 10) and lds < 96 * 1024, (th, tw, lds)


def test_lds_footprint_formula():
    """Host only.  P and T hold (th + 4n)(tw + 4n) pixels (+ the reach of the last pixel group) at 2 wd bytes, the concat buffer the
    tile's pixels at (catC - wd) * 2 bytes: no padding, no tables."""
    # MSPA wd = 16, n = 2, tile 10x20: region 18x28 = 504 -> 528 pixels; tile 200 -> 208; concat 64 channels; chain blob 3 KiB + bias
    slots, g = _tiles(0, 32, 64, 2, 80, (10, 20))
    assert g[:4] == [10, 20, 18, 28]
    assert g[4] == 2 * 528 * 32 + 208 * 128 + 3 * 1024 + 3 * 16 * 4
    # C2f wd = 32, n = 1, tile 8x16: region 12x20 = 240 -> 256; concat 64 channels
    slots, g = _tiles(1, 32, 64, 1, 80, (8, 16))
    assert g[4] == 2 * 256 * 64 + 128 * 128


def _mspa(c, n, sc, hw, B, tile):
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.nn.modules import MSPA_C2f
    m = seed_state_dict_(MSPA_C2f(c, c, n, sc), 7).eval().to(DEV)
    for sub in m.modules():
        if isinstance(sub, torch.nn.BatchNorm2d):
            sub.eps = 1e-3
    x = torch.randn(B, c, *hw, generator=torch.Generator().manual_seed(11)).to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return ops, m, x, lambda: ops.csp_block_supported(ops.CSP_MSPA, x, c, c // 4, n, torch.bfloat16)


def _c2f(c1, c2, n, sc, hw, B, tile):
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.nn.modules import C2f
    m = seed_state_dict_(C2f(c1, c2, n, sc), 5).eval().to(DEV)
    for sub in m.modules():
        if isinstance(sub, torch.nn.BatchNorm2d):
            sub.eps = 1e-3
    x = torch.randn(B, c1, *hw, generator=torch.Generator().manual_seed(3)).to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y01 = torch.empty(B, c2, *hw, device=DEV, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return ops, m, x, lambda: ops.csp_block_supported(ops.CSP_C2F, y01, c2, c2 // 2, n, torch.bfloat16)


def _fused_vs_chain(ops, m, x, supported, tile, what):
    with forced_tile(tile):
        assert supported()
        with torch.no_grad():
            y_fused = m(x).float()
            torch.cuda.synchronize()
    with torch.no_grad():
        ops.FUSED_CSP_BLOCK = False
        try:
            y_chain = m(x).float()
        finally:
            ops.FUSED_CSP_BLOCK = True
        y32 = m(x.float()).float()
    scale = y32.abs().max().item()
    d = (y_fused - y_chain).abs()
    print(f'{what} tile {tile}: fused vs chain max {d.max().item() / scale:.2e} mean {d.mean().item() / scale:.2e}')
    assert torch.isfinite(y_fused).all()
    assert d.max().item() < 1.5e-2 * scale and d.mean().item() < 1e-3 * scale
    assert (y_fused - y32).abs().max().item() < 3e-2 * scale


# (mode, c, n, shortcut, map, tile): tile None = the picker's at B = 2; forced: the tile the picker takes at B = 32 and one of the other
# residency (more than 80 KiB: one workgroup per CU; wd = 8 cannot reach that with tiles <= 32, a 3-per-CU tile instead); (2, 2) / (2, 3):
# the halo is wider than the tile, every tile touches the image border, also where the back conv reads the last bottleneck from P
CASES = [(0, 32, 1, True, 160, None), (0, 64, 2, True, 80, None), (0, 128, 2, True, 40, None), (0, 256, 1, True, 20, None), (1, 64, 1, False, 80, None),
         (0, 32, 1, True, 160, (20, 20)), (0, 32, 1, True, 160, (8, 10)),
         (0, 64, 2, True, 80, (10, 20)), (0, 64, 2, False, 80, (20, 20)),
         (0, 128, 2, True, 40, (10, 10)), (0, 128, 2, True, 40, (10, 20)),
         (0, 256, 1, True, 20, (5, 10)), (0, 256, 1, False, 20, (5, 5)),
         (1, 64, 1, False, 80, (10, 20)), (1, 64, 1, False, 80, (16, 16)),
         (0, 64, 2, True, 12, (2, 2)), (0, 128, 2, False, 12, (2, 3)), (1, 128, 2, True, 12, (2, 2))]


@pytest.mark.gpu
@pytest.mark.parametrize('mode,c,n,sc,hw,tile', CASES)
def test_csp_block_geometry_matches_launch_chain(mode, c, n, sc, hw, tile):
    B = 2
    if tile:
        slots, g = _tiles(mode, B, c, n, hw, tile)
        assert slots > 0 and (g[0], g[1]) == tile, (tile, g)
    if mode == 0:
        ops, m, x, sup = _mspa(c, n, sc, (hw, hw), B, tile)
    else:
        ops, m, x, sup = _c2f(256, c, n, sc, (hw, hw), B, tile)
    _fused_vs_chain(ops, m, x, sup, tile, f'mode {mode} c={c} n={n} sc={sc} {hw}x{hw}')
