"""The forward convolution kernels - mgdt_conv2d_fwd / mgdt_conv2d_fp8_fwd on conv_igemm_kernel and on the LDS-staged conv3x3_lds_kernel - against a
float64 F.conv2d on the CPU, per route, tile and epilogue, through ops.conv2d / ops.conv2d_fp8.  GPU cases need a real MI355X (-m gpu); the route
census and the soundness tests run on the host.

Which kernel instantiation a shape reaches is decided on the host (igemm_plan in conv_igemm.hip, mgdt_conv3x3_lds_plan in conv3x3_lds.hip) and
reported by ops.conv2d_route, which calls those same functions.  Every case states the route it is there for; its id is built from that statement
and test_route_census holds the query to it, so a change of the dispatch that moves a case onto another kernel fails here instead of silently
shrinking the coverage (the older sweep in test_hip_parity.py only ever reaches NT in {1, 3, 5}: asserted below).

Kernel and reference see the SAME values: inputs, residuals and weights are representable in the kernel's dtype (the master weights of an fp8 panel
are plain fp32: see kernel_ref.ref_conv2d_fp8), a BN tuple is folded as the pack kernels fold it (kernel_ref._fold), the input is a channel slice of
a wider buffer and the output a channel slice of a buffer pre-filled with random values whose other channels must come back untouched.  The reference (kernel_ref.ref_conv2d) rounds to bf16 only where the kernel stores bf16 by
design: after the x + x2 add and after the input affine.  Bounds (kernel_ref._close, unchanged):
  bf16 outputs: every element within 2^-8 * |ref| + 1e-3 * max|ref|.
  fp32 outputs: relative L2 error <= 2e-5 and every element within 1e-4 * max|ref|.
  fp8: the e4m3 emulation and the bound of test_conv_fp8_matches_e4m3_emulation (kernel_ref.ref_conv2d_fp8, 8e-3 of max(1, max|ref|)).
"""
import functools

import pytest
import torch

from kernel_ref import (BF16, F32, ConvP, _borders_untouched, _check, _check_fp8, _gen, _nhwc, _out_buf, _rand, ref_conv2d, ref_conv2d_fp8)

gpu = pytest.mark.gpu
F64 = torch.float64
XQ = 16.0                       # fp8 cases: activation multiplier (inputs are N(0, 1): |x| * XQ stays far below 448)
_DT = {'f32': F32, 'bf16': BF16, 'fp8': BF16}


class Case:
    """One launch.  dt 'f32' | 'bf16' | 'fp8'; extras: letters of the fused operands - x = x2, s = in_scale (per image and channel), t = in_shift,
    1 = r1, 2 = r2; yoff / xoff = first channel of the output / input slice in its buffer (xoff defaults to one 16-byte piece); env = experiment
    knobs of the launch; route = the fields of ops.conv2d_route this case is there for."""

    def __init__(self, dt, route, B, cin, cout, k, s, H, W, act='silu', extras='', yoff=4, xoff=None, bn=False, env=None, note=''):
        self.dt, self.route, self.B, self.cin, self.cout, self.k, self.s, self.H, self.W = dt, route, B, cin, cout, k, s, H, W
        self.act, self.extras, self.yoff, self.bn, self.env, self.note = act, extras, yoff, bn, env or {}, note
        self.xoff = (4 if dt == 'f32' else 8) if xoff is None else xoff
        self.Ho, self.Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        r = '-'.join(f'{n}{v}' for n, v in route.items() if n != 'family')
        self.id = '-'.join(str(p) for p in (dt, route.get('family', 'igemm'), r, f'{B}x{H}x{W}', f'c{cin}to{cout}', f'k{k}s{s}', act, extras or 'plain', f'y{yoff}', note) if p != '')

    @property
    def flags(self):
        e = self.extras
        return dict(x2='x' in e, in_scale='s' in e, in_shift='t' in e, r1='1' in e, r2='2' in e, fp8=self.dt == 'fp8')


def _views(c, device='meta'):
    """x and y views of the case with the strides the GPU test uses (slices of buffers 2 * off channels wider), without memory."""
    dt = _DT[c.dt]
    x = torch.empty(c.B, c.cin + 2 * c.xoff, c.H, c.W, dtype=dt, device=device, memory_format=torch.channels_last)[:, c.xoff:c.xoff + c.cin]
    y = torch.empty(c.B, c.cout + 2 * c.yoff, c.Ho, c.Wo, dtype=dt, device=device, memory_format=torch.channels_last)[:, c.yoff:c.yoff + c.cout]
    return x, y


def _route(c, monkeypatch=None):
    from mgdt_yolo_amd import ops
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    x, y = _views(c)
    return ops.conv2d_route(x, y, c.k, c.s, act={'none': ops.ACT_NONE, 'silu': ops.ACT_SILU, 'relu': ops.ACT_RELU, 'gelu': ops.ACT_GELU}[c.act], **c.flags)


# ------------------------------------------------------------------------------------------------ igemm cases
# NT through the default dispatch with one K chunk (cin = 8, k = 1): NT = the largest of {8, 6, 5, 4, 3, 2, 1} dividing the cout blocks, halved while
# the grid has fewer than 128 workgroups and NT is even.  Every map has M % 256 != 0: the last tile has dead pixel rows.
NT_SHAPES = {8: (2, 512, 63, 63), 6: (1, 288, 104, 104), 4: (1, 448, 68, 68), 2: (1, 352, 53, 54), 3: (2, 48, 9, 11), 5: (2, 80, 9, 11), 1: (2, 112, 9, 11)}
ALL5 = 'xst12'


def _nt_cases():
    out = []
    for nt, (B, cout, H, W) in NT_SHAPES.items():
        for dt in ('f32', 'bf16', 'fp8'):
            out.append(Case(dt, dict(NT=nt, D=2, extra=0), B, 8, cout, 1, 1, H, W, 'silu'))
        for dt in ('f32', 'bf16'):
            out.append(Case(dt, dict(NT=nt, D=2, extra=1), B, 8, cout, 1, 1, H, W, 'relu', ALL5, bn=True))
    return out


def _wide_cases():
    """The WIDE epilogue (bf16 / fp8, NT >= 4: ds_bpermute transpose, two 16-byte stores per pixel and group of four cout blocks) and its ragged
    fallback: with cout % 16 != 0 the workgroup that owns the last cout block stores 8 bytes at a time and the others keep the transpose (NT = 5:
    one workgroup, fallback only).  yoff 4 = a slice start that is 8 but not 16 bytes aligned; the residual views are slices of the same kind."""
    out = []
    for nt in (4, 5, 6, 8):
        B, cout, H, W = NT_SHAPES[nt]
        for dt in ('bf16', 'fp8'):
            out.append(Case(dt, dict(NT=nt, ragged=0), B, 8, cout, 1, 1, H, W, 'silu', '12', yoff=8))
            out.append(Case(dt, dict(NT=nt, ragged=1), B, 8, cout - 12, 1, 1, H, W, 'silu', '12', yoff=4, note='cout%16=4'))
            out.append(Case(dt, dict(NT=nt, ragged=1), B, 8, cout - 4, 1, 1, H, W, 'relu', '', yoff=8, note='cout%16=12'))
            out.append(Case(dt, dict(NT=nt, ragged=0), B, 8, cout, 1, 1, H, W, 'none', '1', yoff=4))
    return out


# K chunks (4 pieces of 16 bytes each): 1 and 2 run the depth-2 pipeline, 3 makes the look-ahead equal to the chunk count, 4 fills the depth-4 groups,
# 5 pads the last group with three dead chunks.  k = 3: 9 * CP pieces (3 chunks at CP = 1 with three dead pieces in the last, 5 at CP = 2).
CHUNK_CASES = [
    Case('bf16', dict(NT=3, D=2, nchunks=2), 2, 64, 48, 1, 1, 7, 9), Case('bf16', dict(NT=3, D=4, nchunks=3), 2, 96, 48, 1, 1, 7, 9, 'relu', ALL5),
    Case('bf16', dict(NT=3, D=4, nchunks=4), 2, 128, 48, 1, 1, 7, 9), Case('bf16', dict(NT=5, D=4, nchunks=5), 2, 160, 80, 1, 1, 7, 9, 'relu', ALL5),
    Case('f32', dict(NT=3, D=2, nchunks=2), 2, 32, 48, 1, 1, 7, 9, 'relu', ALL5), Case('f32', dict(NT=3, D=4, nchunks=3), 2, 48, 48, 1, 1, 7, 9),
    Case('f32', dict(NT=5, D=4, nchunks=4), 2, 64, 80, 1, 1, 7, 9, 'relu', ALL5), Case('f32', dict(NT=3, D=4, nchunks=5), 2, 80, 48, 1, 1, 7, 9),
    Case('fp8', dict(NT=3, D=4, nchunks=3), 2, 96, 48, 1, 1, 7, 9, 'relu', 'x1'), Case('fp8', dict(NT=5, D=4, nchunks=5), 2, 160, 80, 1, 1, 7, 9),
    # k = 3, stride 1 and 2, odd maps at stride 2
    Case('bf16', dict(NT=3, D=4, nchunks=3), 2, 8, 48, 3, 2, 13, 17), Case('bf16', dict(NT=1, D=4, nchunks=5), 2, 16, 112, 3, 1, 9, 11, 'relu', ALL5),
    Case('bf16', dict(NT=5, D=4, nchunks=5), 2, 16, 80, 3, 2, 15, 11, 'relu', ALL5, bn=True),
    Case('f32', dict(NT=3, D=4, nchunks=3), 2, 4, 48, 3, 2, 15, 11, 'relu', ALL5), Case('f32', dict(NT=5, D=4, nchunks=5), 2, 8, 80, 3, 1, 9, 11),
    Case('f32', dict(NT=1, D=4, nchunks=5), 2, 8, 16, 3, 2, 13, 17, bn=True), Case('fp8', dict(NT=1, D=4, nchunks=5), 2, 16, 112, 3, 2, 13, 17),
    Case('bf16', dict(NT=4, D=4, nchunks=5), 1, 16, 448, 3, 2, 135, 137, 'relu', ALL5, note='wide-k3s2'),
]

# Pixel decomposition: at Wo >= 16 the first pixel of a 16-pixel block is decomposed on the scalar unit and the lanes wrap (one row, then one image:
# `bump`); below 16 every lane divides for itself.  in_scale is per image, so a block that spans two images reads two rows of it.
PIXEL_CASES = [
    Case('bf16', dict(NT=3), 2, 8, 48, 1, 1, 5, 15, 'relu', ALL5, note='Wo15'), Case('bf16', dict(NT=3), 2, 8, 48, 1, 1, 5, 16, 'relu', ALL5, note='Wo16'),
    Case('bf16', dict(NT=3), 2, 8, 48, 1, 1, 5, 17, 'relu', ALL5, note='Wo17'), Case('f32', dict(NT=3), 2, 8, 48, 3, 1, 5, 15, 'relu', ALL5, note='Wo15'),
    Case('f32', dict(NT=3), 2, 8, 48, 3, 1, 5, 16, 'relu', ALL5, note='Wo16'), Case('f32', dict(NT=3), 2, 8, 48, 3, 1, 5, 17, 'relu', ALL5, note='Wo17'),
    Case('bf16', dict(NT=5), 3, 8, 80, 3, 1, 1, 20, 'relu', ALL5, note='Ho1-block-spans-images'), Case('f32', dict(NT=3), 3, 8, 48, 1, 1, 1, 20, 'relu', ALL5, note='Ho1-block-spans-images'),
    Case('fp8', dict(NT=3), 3, 8, 48, 3, 1, 1, 20, 'silu', 'x1', note='Ho1-block-spans-images'),
    Case('bf16', dict(NT=3), 3, 8, 48, 3, 1, 5, 7, 'relu', ALL5, note='HoWo35'), Case('f32', dict(NT=5), 2, 8, 80, 3, 1, 3, 17, 'relu', ALL5, note='HoWo51'),
    Case('bf16', dict(NT=5), 2, 8, 80, 3, 2, 5, 33, 'relu', ALL5, note='HoWo51'),
    Case('bf16', dict(NT=3), 1, 8, 48, 3, 1, 1, 1, note='1x1'), Case('f32', dict(NT=1), 3, 8, 16, 3, 1, 1, 1, 'relu', ALL5, note='1x1'),
    Case('fp8', dict(NT=5), 1, 8, 80, 1, 1, 1, 1, note='1x1'),
]

# Segmented panels: one cout block whose K panel exceeds 144 KiB is staged in 64-chunk segments (NT = 1, MULTI); 147 chunks = 64 + 64 + 19.
SEG_CASES = [
    Case('f32', dict(NT=1, D=4, extra=0, nseg=3, seg_chunks=64, nchunks=147), 2, 260, 16, 3, 1, 6, 7),
    Case('f32', dict(NT=1, D=4, extra=1, nseg=3, seg_chunks=64, nchunks=147), 2, 260, 32, 3, 2, 9, 7, 'relu', ALL5),
    Case('bf16', dict(NT=1, D=4, extra=0, nseg=3, seg_chunks=64, nchunks=147), 2, 520, 32, 3, 1, 6, 7),
    Case('bf16', dict(NT=1, D=4, extra=1, nseg=3, seg_chunks=64, nchunks=147), 2, 520, 16, 3, 2, 9, 7, 'relu', ALL5),
    Case('fp8', dict(NT=1, D=4, nseg=5, seg_chunks=64, nchunks=293), 1, 1040, 16, 3, 1, 6, 7, note='293=4x64+37'),
]

# The persistent tile loop (a workgroup's second tile: nxt -> cur hand-over, segment 0 staged again) needs more than 65 536 pixels by default;
# MGDT_CONV_GCAP (read on every call) caps the grid instead.
GCAP = {'MGDT_CONV_GCAP': '8'}
PERSIST_CASES = [
    Case('bf16', dict(NT=8, extra=1, gx=8, numTiles=32), 2, 8, 512, 1, 1, 63, 63, 'relu', ALL5, env=GCAP),
    Case('f32', dict(NT=6, extra=1, gx=8, numTiles=43), 1, 8, 288, 1, 1, 104, 104, 'relu', ALL5, env=GCAP),
    Case('bf16', dict(NT=1, extra=1, nseg=3, gx=8, numTiles=10), 2, 520, 16, 3, 1, 33, 35, 'relu', ALL5, env=GCAP),
    Case('f32', dict(NT=1, extra=0, nseg=3, gx=8, numTiles=10), 2, 260, 16, 3, 1, 33, 35, env=GCAP),
    Case('fp8', dict(NT=4, gx=8, numTiles=19), 1, 8, 448, 1, 1, 68, 68, 'silu', 'x12', env=GCAP),
    Case('bf16', dict(NT=5, D=4, gx=8, numTiles=19, nchunks=5), 1, 16, 80, 3, 2, 135, 137, env=GCAP),
]

MT4 = {'MGDT_CONV_MT1': '4'}
MT4_CASES = [
    Case('f32', dict(NT=1, MT=4, numTiles=2), 3, 8, 16, 3, 1, 13, 17, 'relu', ALL5, env=MT4),
    Case('bf16', dict(NT=1, MT=4, numTiles=2, ragged=1), 3, 16, 12, 3, 1, 13, 17, env=MT4),
    Case('bf16', dict(NT=1, MT=4, numTiles=1), 2, 8, 16, 1, 1, 5, 16, 'relu', ALL5, env=MT4),
]

ACT_CASES = [Case(dt, dict(NT=nt), 2, 8, 16 * nt, 1, 1, 9, 11, act, ex)
             for dt, ex in (('f32', '1'), ('bf16', '1'), ('fp8', '')) for act, nt in (('gelu', 3), ('none', 5))]

IGEMM_CASES = _nt_cases() + _wide_cases() + CHUNK_CASES + PIXEL_CASES + SEG_CASES + PERSIST_CASES + MT4_CASES + ACT_CASES

# ------------------------------------------------------------------------------------------------ lds3x3 cases
# The predicate's floor is 16 384 INPUT pixels with h, w >= 16; no map is a multiple of the 16-column tiles or of the tile rows; sliced views.
LDS_CASES = [
    Case('bf16', dict(family='lds3x3', NBW=2, tile_rows=16, ncg=1, waves=4), 1, 32, 32, 3, 1, 113, 147),
    Case('bf16', dict(family='lds3x3', NBW=3, tile_rows=16, ncg=1, waves=4), 1, 48, 48, 3, 1, 147, 113, 'relu'),
    Case('bf16', dict(family='lds3x3', NBW=4, tile_rows=16, ncg=1, waves=8), 4, 64, 64, 3, 1, 65, 67, 'none', bn=True),
    Case('bf16', dict(family='lds3x3', NBW=6, tile_rows=16, ncg=1, waves=8), 1, 64, 96, 3, 1, 113, 147),
    Case('bf16', dict(family='lds3x3', NBW=5, tile_rows=12, ncg=1, waves=8, nchunks=23), 1, 80, 80, 3, 1, 113, 147),
    Case('bf16', dict(family='lds3x3', NBW=6, tile_rows=16, ncg=1, nchunks=9), 2, 32, 84, 3, 1, 91, 93, note='cout%16=4'),
    Case('bf16', dict(family='lds3x3', NBW=4, tile_rows=8, ncg=1, nchunks=9, waves=8), 1, 32, 64, 3, 2, 129, 131),
    Case('bf16', dict(family='lds3x3', NBW=4, tile_rows=8, ncg=2, nchunks=18, waves=8), 1, 64, 128, 3, 2, 131, 129, 'relu'),
    Case('bf16', dict(family='lds3x3', NBW=4, tile_rows=8, ncg=3, nchunks=9, waves=8), 2, 32, 192, 3, 2, 91, 93, 'none'),
    Case('fp8', dict(family='lds3x3', NBW=2, tile_rows=16, waves=4), 1, 32, 32, 3, 1, 113, 147),
    Case('fp8', dict(family='lds3x3', NBW=4, tile_rows=16, waves=4), 4, 64, 64, 3, 1, 65, 67, 'relu', bn=True),
    Case('fp8', dict(family='lds3x3', NBW=6, tile_rows=16, waves=4, nchunks=23), 1, 80, 96, 3, 1, 147, 113, 'none'),
]

# just under each threshold of the predicate: the igemm kernel takes these
NOT_LDS = [
    Case('bf16', dict(family='igemm'), 1, 32, 32, 3, 1, 127, 129, note='16383px'), Case('bf16', dict(family='igemm'), 1, 32, 32, 3, 1, 15, 1100, note='h15'),
    Case('bf16', dict(family='igemm'), 1, 32, 32, 3, 1, 1100, 15, note='w15'), Case('bf16', dict(family='igemm'), 1, 24, 32, 3, 1, 113, 147, note='cin24'),
    Case('bf16', dict(family='igemm'), 1, 88, 32, 3, 1, 113, 147, note='cin88'), Case('bf16', dict(family='igemm'), 1, 32, 28, 3, 1, 113, 147, note='cout28'),
    Case('bf16', dict(family='igemm'), 1, 32, 112, 3, 1, 113, 147, note='7blocks'), Case('bf16', dict(family='igemm'), 1, 32, 32, 3, 1, 113, 147, 'gelu', note='gelu'),
    Case('bf16', dict(family='igemm'), 1, 32, 32, 3, 1, 113, 147, 'silu', '1', note='residual'), Case('bf16', dict(family='igemm'), 1, 32, 32, 3, 1, 113, 147, 'silu', 'x', note='x2'),
    Case('bf16', dict(family='igemm'), 1, 32, 32, 3, 1, 113, 147, 'silu', 's', note='in_scale'), Case('bf16', dict(family='igemm'), 1, 32, 32, 1, 1, 113, 147, note='k1'),
    Case('f32', dict(family='igemm'), 1, 32, 32, 3, 1, 113, 147, note='f32'), Case('bf16', dict(family='igemm'), 1, 32, 96, 3, 2, 129, 131, note='s2-6blocks'),
    Case('bf16', dict(family='igemm'), 1, 80, 64, 3, 2, 129, 131, note='s2-cin80'), Case('fp8', dict(family='igemm'), 1, 32, 64, 3, 2, 129, 131, note='s2-fp8'),
    Case('bf16', dict(family='igemm'), 1, 48, 64, 3, 2, 129, 131, note='s2-14chunks'),
    # five cout blocks: 16-row tiles are not instantiated, so only the 80-channel panel (which forces 12-row tiles) is taken
    Case('bf16', dict(family='igemm'), 1, 32, 80, 3, 1, 113, 147, note='5blocks-16rows'), Case('bf16', dict(family='igemm'), 1, 72, 80, 3, 1, 113, 147, note='5blocks-16rows'),
]

ALL_CASES = IGEMM_CASES + LDS_CASES
_ids = lambda cs: [c.id for c in cs]


# ------------------------------------------------------------------------------------------------ host-only tests
def test_case_ids_are_unique():
    ids = _ids(ALL_CASES + NOT_LDS)
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)


@pytest.mark.parametrize('c', ALL_CASES + NOT_LDS, ids=_ids(ALL_CASES + NOT_LDS))
def test_route_census(c, monkeypatch):
    """ops.conv2d_route (the launch's own planning functions) sends the case to exactly the route it states."""
    r = _route(c, monkeypatch)
    want = dict(c.route)
    want.setdefault('family', 'igemm')
    assert {k: r.get(k) for k in want} == want, r
    if c.route.get('gx'):
        assert r['numTiles'] > r['gx']                              # a workgroup takes at least two tiles
    assert r['lds_bytes'] <= 160 * 1024


def test_route_census_covers_every_route(monkeypatch):
    """The union of the igemm cases: every NT in every dtype, both pipeline depths, plain and extra, one and several panel segments, a workgroup
    with two tiles, ragged and full last blocks at NT >= 4, both pixel decompositions, MT = 4; the LDS cases: every NBW, tile height and cout-group
    count the kernel is instantiated for."""
    seen = []
    for c in IGEMM_CASES:
        with monkeypatch.context() as m:
            seen.append((c, _route(c, m)))
    assert all(r['family'] == 'igemm' for _, r in seen)
    for dt in ('f32', 'bf16', 'fp8'):
        mine = [(c, r) for c, r in seen if c.dt == dt]
        assert {r['NT'] for _, r in mine} == {1, 2, 3, 4, 5, 6, 8}, dt
        assert {r['NT'] for c, r in mine if c.act == 'silu' and not c.extras} == {1, 2, 3, 4, 5, 6, 8}, dt
        if dt != 'fp8':
            assert {r['NT'] for c, r in mine if c.extras == ALL5 and c.act == 'relu'} == {1, 2, 3, 4, 5, 6, 8}, dt
            assert {r['MT'] for _, r in mine} == {2, 4}, dt
        assert {r['D'] for _, r in mine} == {2, 4} and {r['extra'] for _, r in mine} == {0, 1}, dt
        assert {r['nchunks'] for _, r in mine} >= {1, 2, 3, 4, 5} if dt != 'fp8' else {1, 3, 5}, dt
        assert any(r['nseg'] >= 3 and r['nchunks'] % r['seg_chunks'] for _, r in mine), dt
        assert any(r['numTiles'] > r['gx'] for _, r in mine), dt
        assert {c.act for c, _ in mine} == {'silu', 'relu', 'gelu', 'none'}, dt
        assert {c.Wo >= 16 for c, _ in mine} == {True, False}, dt
    for dt in ('bf16', 'fp8'):
        for nt in (4, 5, 6, 8):
            wide = [(c, r) for c, r in seen if c.dt == dt and r['NT'] == nt]
            assert {(r['ragged'], c.cout % 16) for c, r in wide} >= {(0, 0), (1, 4), (1, 12)}, (dt, nt)
            assert {c.yoff for c, _ in wide} >= {4, 8} and {bool(set(c.extras) & set('12')) for c, _ in wide} == {True, False}, (dt, nt)
    for dt in ('f32', 'bf16'):                                      # segmented panels, plain and extra; a second tile at NT = 8 fused / NT = 1 segmented
        assert {r['extra'] for c, r in seen if c.dt == dt and r['nseg'] >= 3} == {0, 1}, dt
    two = [(c, r) for c, r in seen if r['numTiles'] > r['gx']]
    assert any(c.dt == 'bf16' and r['NT'] == 8 and r['extra'] for c, r in two) and any(r['NT'] == 1 and r['nseg'] > 1 for c, r in two)
    assert any(c.dt == 'fp8' for c, _ in two)
    lds = [(c, _route(c)) for c in LDS_CASES]
    assert all(r['family'] == 'lds3x3' for _, r in lds)
    bf = [(c, r) for c, r in lds if c.dt == 'bf16']
    assert {r['NBW'] for c, r in bf if c.s == 1} == {2, 3, 4, 5, 6} and {r['tile_rows'] for _, r in bf} == {8, 12, 16}
    assert {r['nchunks'] for c, r in bf if c.s == 2} == {9, 18} and {r['ncg'] > 1 for c, r in bf if c.s == 2} == {True, False}
    assert {r['NBW'] for c, r in lds if c.dt == 'fp8'} == {2, 4, 6}
    for c, _ in lds:
        assert c.B * c.H * c.W >= 16384 and (c.Wo % 16 or c.Ho % 16) and c.xoff and c.yoff


def test_old_sweep_reaches_only_odd_nt():
    """The blind spot this module closes: every shape of the older sweep (CONV_CASES / FP8_CONV_CASES of test_hip_parity.py, B = 3 / as listed)
    has so few pixels that an even NT is halved down to 1 or 3."""
    import test_hip_parity as T
    from mgdt_yolo_amd import ops

    def nt(B, cin, cout, k, s, h, w, dt, fp8):
        x = torch.empty(B, cin + 16, h, w, dtype=dt, device='meta', memory_format=torch.channels_last)[:, 8:8 + cin]
        ho, wo = ops.conv_out_hw(h, w, k, s)
        y = torch.empty(B, cout + 8, ho, wo, dtype=dt, device='meta', memory_format=torch.channels_last)[:, 4:4 + cout]
        return {ops.conv2d_route(x, y, k, s, fp8=fp8, x2=fused, r1=fused).get('NT', 'lds') for fused in (False, True)}
    seen = set()
    for cin, cout, k, s, h, w in T.CONV_CASES:
        for dt in (F32, BF16):
            seen |= nt(3, cin, cout, k, s, h, w, dt, False)
    assert seen == {1, 3, 5}, seen
    seen8 = set()
    for B, cin, h, w, cout, k, s, _ in T.FP8_CONV_CASES:
        seen8 |= nt(B, cin, cout, k, s, h, w, BF16, True)
    assert seen8 - {'lds'} <= {1, 3, 5}, seen8


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    """Seeded CPU operands of a case (fp64 holding values of the kernel's dtype) and its float64 reference, computed once per session."""
    c = {k.id: k for k in ALL_CASES}[cid]
    dt, gen = _DT[c.dt], _gen('conv', cid)
    x = _rand(gen, c.B, c.cin, c.H, c.W, dt=dt)
    cp = ConvP(gen, c.cout, c.cin, c.k, bn=c.bn, dt=dt, gain=1.5, wrep=F32 if c.dt == 'fp8' else BF16)   # fp8: see ref_conv2d_fp8
    f = c.flags
    ops_ = dict(x2=_rand(gen, c.B, c.cin, c.H, c.W, dt=dt) if f['x2'] else None,
                in_scale=(torch.rand(c.B, c.cin, generator=gen) + 0.5).float().double() if f['in_scale'] else None,
                in_shift=(torch.randn(c.cin, generator=gen) * 0.1).float().double() if f['in_shift'] else None,
                r1=_rand(gen, c.B, c.cout, c.Ho, c.Wo, dt=dt) if f['r1'] else None, r2=_rand(gen, c.B, c.cout, c.Ho, c.Wo, dt=dt) if f['r2'] else None)
    if c.dt == 'fp8':
        ref = ref_conv2d_fp8(x, cp, c.s, c.act, XQ, ops_['x2'], ops_['r1'], ops_['r2'])
    else:
        ref = ref_conv2d(x, cp, c.s, c.act, dt, **ops_)
    return x, cp, ops_, ref


SOUND = [c for c in ALL_CASES if c.dt == 'bf16' and set(c.extras) & set('xst')]


@pytest.mark.parametrize('c', SOUND, ids=_ids(SOUND))
def test_restatement_soundness(c):
    """Host only: the reference of each fused bf16 case, evaluated in fp32 with the same rounding points, stays inside the bf16 bound of its float64
    evaluation at the seed used: accumulation precision and the rare one-ulp flip of a rounded intermediate do not break the bound by themselves."""
    x, cp, o, ref = _inputs(c.id)
    _check(ref_conv2d(x, cp, c.s, c.act, BF16, dt=F32, **o), ref, BF16, c.id + ' fp32 restatement')


# ------------------------------------------------------------------------------------------------ GPU tests
def _run(c, monkeypatch):
    from mgdt_yolo_amd import ops
    from kernel_ref import DEV
    r = _route(c, monkeypatch)                                       # sets the case's knobs for the launch too
    assert {k: r.get(k) for k in c.route} == c.route, r
    dt = _DT[c.dt]
    x, cp, o, ref = _inputs(c.id)
    gen = _gen('conv-buffers', c.id)
    xv, _ = _nhwc(x, dt, c.xoff, c.xoff, gen)
    sl = lambda t, off: None if t is None else _nhwc(t, dt, off, off, gen)[0]
    x2, r1, r2 = sl(o['x2'], c.xoff), sl(o['r1'], 4), sl(o['r2'], 8)
    dev = lambda t: None if t is None else t.float().to(DEV)
    out, big, big0 = _out_buf(c.B, c.cout, c.Ho, c.Wo, dt, c.yoff, c.yoff, gen)
    assert xv.stride() == _views(c)[0].stride() and out.stride() == _views(c)[1].stride()
    act = {'none': ops.ACT_NONE, 'silu': ops.ACT_SILU, 'relu': ops.ACT_RELU, 'gelu': ops.ACT_GELU}[c.act]
    if c.dt == 'fp8':
        ops.conv2d_fp8(xv, cp.pack_fp8(XQ), c.s, act, out=out, x2=x2, r1=r1, r2=r2)
        _check_fp8(out, ref, c.id)
    else:
        ops.conv2d(xv, cp.pack(), c.s, act, out=out, x2=x2, r1=r1, r2=r2, in_scale=dev(o['in_scale']), in_shift=dev(o['in_shift']))
        _check(out, ref, dt, c.id)
    _borders_untouched(big, big0, c.yoff, c.cout)


@gpu
@pytest.mark.parametrize('c', IGEMM_CASES, ids=_ids(IGEMM_CASES))
def test_conv_igemm(c, monkeypatch):
    """One launch on the route the case states, against the float64 reference (fp8: the e4m3 emulation); the output buffer's other channels stay as
    they were."""
    _run(c, monkeypatch)


@gpu
@pytest.mark.parametrize('c', LDS_CASES, ids=_ids(LDS_CASES))
def test_conv3x3_lds(c, monkeypatch):
    """The LDS-staged kernel (the route query proves it takes the case) against the float64 reference under the bf16 bound; ragged maps, sliced views."""
    _run(c, monkeypatch)
