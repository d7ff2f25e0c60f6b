"""mgdt_stem2_fwd as a persistent kernel: a workgroup walks several 8 x 16 output tiles, keeps everything tile-independent in registers and requests the
next tile's image patch while it computes the current one.  Which workgroup gets which tiles must not matter, and the values are those of the
one-tile-per-workgroup kernel: the K mapping, the MFMA order and both bf16 rounding points are unchanged.

The kernel is called through the C ABI (ops._launch) rather than ops.stem2 because the output here is a channel- and row-strided view inside a
larger buffer, which ops.stem2 (it allocates its own output) cannot express.

Bounds: 2e-2 of the fp64 reference's largest magnitude, for the fused kernel, for the two-launch chain and for their difference - the bounds of
test_hip_parity.py::test_fused_stem_matches_two_conv_launches, not new ones.  Everything else is torch.equal."""
import ctypes as C

import pytest
import torch

from kernel_ref import DEV, _gen
from mgdt_yolo_amd.models import get_config
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images

CASES = [(2, 64, 96), (2, 37, 45), (2, 30, 18), (2, 320, 352), (2, 640, 640), (5, 160, 160)]
DTYPES = ['bf16', 'f32', 'u8']
WGS = ['1', '3', '7', None]           # MGDT_STEM_WGS: one workgroup walks every tile of every image; uneven counts and empty XCD ranges; the default grid
OFF, EXTRA, ROW0, ROWX = 8, 24, 1, 2  # the output view: channels [8, 40) of 64, rows [1, 1 + H1) of H1 + 3


@pytest.fixture(scope='module')
def stem():
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    m = seed_state_dict_(DetectionModel(get_config('mspa_c2f_gd_yolov8', 'n', 80), verbose=False), 0).eval().to(DEV).set_compute_dtype(torch.bfloat16)
    m0, m1 = m.model[0], m.model[1]
    with torch.no_grad():
        pk0 = ops.PackedStem2(m0.conv.weight, (m0.bn.weight, m0.bn.bias, m0.bn.running_mean, m0.bn.running_var, m0.bn.eps))
        pk1 = m1.packed(torch.bfloat16, direct=False)
    return m, pk0, pk1


def _image(in_dtype, b, h, w):
    """(device image of the kernel's input dtype, the same values as CPU fp32)"""
    img = seeded_images(b, h, w, seed=4)
    if in_dtype == 'u8':
        x = (img * 255).round().clamp_(0, 255).to(torch.uint8).to(DEV)
        return x, x.float().cpu() / 255
    if in_dtype == 'bf16':
        x = img.to(DEV).to(torch.bfloat16)
        return x, x.float().cpu()
    return img.to(DEV), img


def _out_hw(h, w):
    h0, w0 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return (h0 - 1) // 2 + 1, (w0 - 1) // 2 + 1


def _run(x, pk0, pk1, wgs, monkeypatch, key):
    """One launch into a strided view of a buffer of random values; returns (the view's values, True when nothing outside the view was written)."""
    from mgdt_yolo_amd import ops
    b, _, h, w = x.shape
    h1, w1 = _out_hw(h, w)
    big0 = torch.randn(b, 32 + OFF + EXTRA, h1 + ROW0 + ROWX, w1, generator=_gen('stem2 out', key)).to(torch.bfloat16)
    big = torch.empty(big0.shape, dtype=torch.bfloat16, device=DEV, memory_format=torch.channels_last)
    big.copy_(big0)
    y = big[:, OFF:OFF + 32, ROW0:ROW0 + h1]
    if wgs is None:
        monkeypatch.delenv('MGDT_STEM_WGS', raising=False)
    else:
        monkeypatch.setenv('MGDT_STEM_WGS', wgs)
    code = ops.U8 if x.dtype == torch.uint8 else ops.dtype_code(x.dtype)
    ops._launch('stem2_fwd', 'mgdt_stem2_fwd', ops.vp(x), code, ops.ptr(pk0.blob), ops.ptr(pk0.bias), ops.ptr(pk1.w), ops.ptr(pk1.bias), ops.vp(y), ops.stream())
    torch.cuda.synchronize()
    got = big.cpu()
    mask = torch.ones(big0.shape, dtype=torch.bool)
    mask[:, OFF:OFF + 32, ROW0:ROW0 + h1] = False
    untouched = torch.equal(got[mask], big0[mask])
    return got[:, OFF:OFF + 32, ROW0:ROW0 + h1].clone(), untouched


@pytest.mark.gpu
@pytest.mark.parametrize('in_dtype', DTYPES)
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_tile_to_workgroup_assignment_does_not_matter(stem, in_dtype, case, monkeypatch):
    """MGDT_STEM_WGS = 1, 3, 7 and unset: the same bits, and nothing outside the output view is written.  Catches a prefetched patch that reaches the
    LDS patch buffer too early, a stale per-workgroup table entry, a wrong tile origin, a lost last tile."""
    _, pk0, pk1 = stem
    x, _ = _image(in_dtype, *case)
    outs = []
    for wgs in WGS:
        y, untouched = _run(x, pk0, pk1, wgs, monkeypatch, (in_dtype, case))
        assert untouched, f'MGDT_STEM_WGS={wgs}: wrote outside the output view'
        assert torch.isfinite(y.float()).all()
        outs.append(y)
    for wgs, y in zip(WGS[1:], outs[1:]):
        assert torch.equal(y, outs[0]), f'MGDT_STEM_WGS={wgs} differs from MGDT_STEM_WGS=1 in {(y != outs[0]).sum().item()} elements'


@pytest.mark.gpu
@pytest.mark.parametrize('in_dtype', DTYPES)
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_same_values_as_the_reference_and_the_two_launch_chain(stem, in_dtype, case, monkeypatch):
    """Against the fp64 two-layer reference (BN folded) on the values the kernel sees, and against the stem kernel + implicit-GEMM conv chain."""
    from oracle import layers as OL
    m, pk0, pk1 = stem
    x, xf = _image(in_dtype, *case)
    assert m._stem_fusable(x)
    y_fused, untouched = _run(x, pk0, pk1, None, monkeypatch, (in_dtype, case))
    assert untouched
    with torch.no_grad():
        y_two = m.model[1](m.model[0](x)).float().cpu()
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    ref = OL.conv(OL.conv(xf.double(), sd, 'model.0', s=2, fused=True), sd, 'model.1', s=2, fused=True)
    scale = ref.abs().max().item()
    y_fused = y_fused.float()
    assert y_fused.shape == y_two.shape == ref.shape
    e_f, e_t = (y_fused.double() - ref).abs().max().item() / scale, (y_two.double() - ref).abs().max().item() / scale
    e_d = (y_fused - y_two).abs().max().item() / scale
    print(f'stem2 {in_dtype} {case}: fused vs fp64 {e_f:.2e}, two launches vs fp64 {e_t:.2e}, fused vs two launches {e_d:.2e}')
    assert e_f < 2e-2 and e_t < 2e-2
    assert e_d < 2e-2


@pytest.mark.gpu
@pytest.mark.parametrize('hw', [(64, 96), (320, 352)])
@pytest.mark.parametrize('wgs', ['1', '7', None])
def test_strided_image_takes_the_generic_loader_and_agrees_with_the_fast_path(stem, hw, wgs, monkeypatch):
    """A crop of a larger bf16 tensor at an odd column offset has rows that are neither contiguous with each other nor 16-byte aligned, so the
    wrapper cannot choose the 16-byte loader; the contiguous copy of the same values can.  Both must give the same bits."""
    _, pk0, pk1 = stem
    h, w = hw
    big = seeded_images(2, h + 5, w + 16, seed=9).to(DEV).to(torch.bfloat16)
    crop = big[:, :, 2:2 + h, 3:3 + w]
    dense = crop.contiguous()
    assert crop.data_ptr() % 16 != 0 and dense.data_ptr() % 16 == 0 and w % 8 == 0
    y_g, ok_g = _run(crop, pk0, pk1, wgs, monkeypatch, ('crop', hw))
    y_f, ok_f = _run(dense, pk0, pk1, wgs, monkeypatch, ('crop', hw))
    assert ok_g and ok_f
    assert torch.equal(y_g, y_f), f'{(y_g != y_f).sum().item()} elements differ'


def test_grid_fits_the_chip_at_the_bench_shape(monkeypatch):
    """Host only (no launch): at bench.py's shape (32 x 3 x 640 x 640) on a 256-CU device the persistent grid is no larger than the tile count or than
    three workgroups per compute unit, three workgroups' LDS fit the 160 KB of a compute unit, and MGDT_STEM_WGS caps the grid."""
    from mgdt_yolo_amd import _lib
    lib = _lib.lib()
    out = (C.c_int * 5)()
    monkeypatch.delenv('MGDT_STEM_WGS', raising=False)
    for cus in (256, 304, 8):
        _lib.check(lib.mgdt_stem2_geometry(32, 640, 640, cus, out), 'stem2_geometry')
        tiles, grid, lds, per_cu, ncu = list(out)
        assert tiles == 32 * 20 * 10 and ncu == cus and per_cu == 3
        assert 1 <= grid <= tiles and grid <= 3 * cus and grid == min(tiles, 3 * cus)
        assert lds * 3 <= 160 * 1024
    _lib.check(lib.mgdt_stem2_geometry(2, 30, 18, 256, out), 'stem2_geometry')
    assert out[0] == 2 and out[1] == 2            # fewer tiles than the chip holds: one workgroup per tile
    monkeypatch.setenv('MGDT_STEM_WGS', '7')
    _lib.check(lib.mgdt_stem2_geometry(32, 640, 640, 256, out), 'stem2_geometry')
    assert out[1] == 7
    assert lib.mgdt_stem2_geometry(0, 640, 640, 256, out) != 0
