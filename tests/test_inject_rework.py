"""mgdt_conv1x1_inject_conv_fwd / mgdt_conv1x1_inject_fwd where the carried patch geometry, the division-free index arithmetic and the 8-byte
fragment stores of the GCONV build can go wrong: more patches than persistent workgroups with n, ty and tx wrapping together, ragged edges with a
non-integer ratio, source patches of exactly 16, 17..32 and 49..64 pixels (the 16-pixel groups of the build), a 1 x 1 global map, and run-to-run
determinism.  Against kernel_ref.ref_inject_conv / ref_inject in float64 with the bound of test_block_kernels (kernel_ref._check: every bf16
element within 2^-8 |ref| + 1e-3 max|ref|).  The host test restates the kernel's index arithmetic (FastDiv of common.h, inj_pw_magic and
inj_geom of inject_fused.hip) and compares it with // and %.
"""
import functools

import numpy as np
import pytest
import torch

from kernel_ref import BF16, _borders_untouched, _check, _nhwc, _out_buf, inj_lerp, ref_inject, ref_inject_conv
from test_block_kernels import INJ2_CAP, INJ_CAP, _inj_inputs, inject_conv_supported, inject_supported

gpu = pytest.mark.gpu

# (id, cin, cout2, B, H, W, Hg, Wg, out offset, gconv)
WRAP = ('wrap-270-patches', 64, 64, 5, 72, 88, 36, 44, 0)
CASES = [
    WRAP + (True,), WRAP + (False,),
    ('ragged-37x53-from-13x19', 24, 48, 2, 37, 53, 13, 19, 0, True), ('ragged-37x53-from-13x19', 24, 48, 2, 37, 53, 13, 19, 0, False),
    ('patch-16px-8x16-from-2x8', 32, 32, 2, 8, 16, 2, 8, 0, True), ('patch-32px-8x16-from-4x8', 32, 32, 2, 8, 16, 4, 8, 0, True),
    ('patch-64px-8x8-from-8x8', 32, 32, 2, 8, 8, 8, 8, 0, True),
    ('global-1x1-out-slice', 16, 16, 3, 9, 21, 1, 1, 4, True),
]
# the shapes of CASES, the plain kernel's case below, and the workload's (80 x 80 from 40 x 40 at B = 32): (B, H, W, Hg, Wg)
GEOMETRIES = sorted({c[3:8] for c in CASES} | {(32, 80, 80, 40, 40)})


def _patch_pixels(H, W, Hg, Wg, TH=8):
    """Source-patch sizes (ph * pw) over the TH x 16 tiles of a map."""
    y0, y1, _ = inj_lerp(H, Hg)
    x0, x1, _ = inj_lerp(W, Wg)
    return {(int(y1[min(t + TH - 1, H - 1)] - y0[t]) + 1) * (int(x1[min(u + 15, W - 1)] - x0[u]) + 1) for t in range(0, H, TH) for u in range(0, W, 16)}


@functools.lru_cache(maxsize=None)
def _case(cid, cin, cout2, B, H, W, Hg, Wg, gconv):
    """Inputs and the float64 reference of one case, computed once and shared (never modified)."""
    x, pk, gaf, gsrc, pkg, pk2, gen = _inj_inputs(cid, cin, 256, B, H, W, Hg, Wg, False, gconv, cout2)
    if gconv:
        ref = ref_inject_conv(x, pk, None, None, pk2, pkg=pkg, gsrc=gsrc)
    else:
        ref = ref_inject_conv(x, pk, gaf[:, :256], gaf[:, 256:], pk2)
    return x, pk, gaf, gsrc, pkg, pk2, gen, ref


def _run(case, ooff=0):
    from mgdt_yolo_amd import ops
    cid, cin, cout2, B, H, W, Hg, Wg, gconv = case
    x, pk, gaf, gsrc, pkg, pk2, gen, ref = _case(*case)
    xv, gd = _nhwc(x, BF16)[0], _nhwc(gaf, BF16)[0]
    assert inject_conv_supported(cin, 256, cout2, H, W, Hg, Wg) and ops.conv1x1_inject_conv_supported(xv, 256, cout2, gd[:, :256], BF16)
    out, big, big0 = _out_buf(B, cout2, H, W, BF16, ooff, ooff, gen)
    p2 = pk2.pack(ops.acc_order_index(256, 'cpu'))
    if gconv:
        ops.conv1x1_inject_conv(xv, pk.pack(), None, None, p2, ops.ACT_SILU, out, gsrc=_nhwc(gsrc, BF16)[0], pkg=pkg.pack())
    else:
        ops.conv1x1_inject_conv(xv, pk.pack(), gd[:, :256], gd[:, 256:], p2, ops.ACT_SILU, out)
    return out, big, big0, ref


def test_cases_are_what_they_claim():
    """The wrap case has more patches than persistent workgroups and no axis a multiple of the grid; the three group cases hold exactly 16, 17..32
    and 49..64 source pixels; the ragged case has partial tiles on both axes and a K chunk that is partly padding."""
    _, _, _, B, H, W, Hg, Wg, _ = WRAP
    tx, ty = -(-W // 16), -(-H // 8)
    assert B * ty * tx == 270 > INJ2_CAP and INJ2_CAP % tx and INJ2_CAP % (tx * ty)
    assert _patch_pixels(8, 16, 2, 8) == {16} and _patch_pixels(8, 16, 4, 8) == {32} and _patch_pixels(8, 8, 8, 8) == {64}
    assert 37 % 8 and 53 % 16 and 24 % 32 and 37 % 13 and 53 % 19
    assert all(max(_patch_pixels(*g[1:])) <= 64 for g in GEOMETRIES)


@gpu
@pytest.mark.parametrize('cid,cin,cout2,B,H,W,Hg,Wg,ooff,gconv', [pytest.param(*c, id=f'{c[0]}-{"gconv" if c[9] else "maps"}') for c in CASES])
def test_inject_conv_rework(cid, cin, cout2, B, H, W, Hg, Wg, ooff, gconv):
    out, big, big0, ref = _run((cid, cin, cout2, B, H, W, Hg, Wg, gconv), ooff)
    _check(out, ref, BF16, cid)
    _borders_untouched(big, big0, ooff, cout2)


@gpu
def test_inject_plain_kernel_wraps():
    """mgdt_conv1x1_inject_fwd (4 x 16 tiles, 512 persistent workgroups) on the wrap shape: 5 * 18 * 6 = 540 patches."""
    from mgdt_yolo_amd import ops
    cid, cin, _, B, H, W, Hg, Wg, _ = WRAP
    assert B * -(-H // 4) * -(-W // 16) == 540 > INJ_CAP and inject_supported(cin, 128, H, W, Hg, Wg)
    x, pk, gaf, _, _, _, gen = _inj_inputs(cid + '-plain', cin, 128, B, H, W, Hg, Wg, False)
    gd, xv = _nhwc(gaf, BF16)[0], _nhwc(x, BF16)[0]
    assert ops.conv1x1_inject_supported(xv, 128, gd[:, :128], BF16)
    out, big, big0 = _out_buf(B, 128, H, W, BF16, 4, 4, gen)
    ops.conv1x1_inject(xv, pk.pack(), gd[:, :128], gd[:, 128:], out=out)
    _check(out, ref_inject(x, pk, gaf[:, :128], gaf[:, 128:]), BF16, cid)
    _borders_untouched(big, big0, 4, 128)


@gpu
def test_inject_conv_is_deterministic():
    """The wrap case twice, then once more after a launch of another shape on the same stream (another geometry, other stale LDS slots)."""
    case = WRAP[:8] + (True,)
    a = _run(case)[0].clone()
    b = _run(case)[0].clone()
    _run(('patch-32px-8x16-from-4x8', 32, 32, 2, 8, 16, 4, 8, True))
    c = _run(case)[0]
    assert torch.equal(a, b) and torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ host: the index arithmetic
def make_fastdiv(d):
    """make_fastdiv of common.h: (mul, sh) with n // d == (n * mul >> 32) >> sh for n < 2^31; d == 1 is the identity."""
    if d == 1:
        return None
    l = 0
    while (1 << l) < d:
        l += 1
    return ((1 << (32 + l - 1)) // d + 1) & 0xffffffff, l - 1


def fdiv(n, f):
    return n if f is None else ((n * f[0]) >> 32) >> f[1]


def pw_magic(pw, first_guess_error):
    """inj_pw_magic: the hardware reciprocal gives 65536 / pw give or take one; two corrections make it the exact quotient, + 1 rounds up."""
    m = 65536 // pw + first_guess_error
    m -= m * pw > 65536
    m += (m + 1) * pw <= 65536
    return m + 1


def test_index_arithmetic_equals_division():
    for B, H, W, Hg, Wg in GEOMETRIES:
        for TH in (8, 4):
            tiles_x, tiles_y = -(-W // 16), -(-H // TH)
            fx, fy = make_fastdiv(tiles_x), make_fastdiv(tiles_y)
            # every patch index, and the one past the end
            patch = np.arange(B * tiles_x * tiles_y + 1).astype(object)
            for p in patch:
                row = fdiv(p, fx)
                n = fdiv(row, fy)
                assert (row, p - row * tiles_x, n, row - n * tiles_y) == (p // tiles_x, p % tiles_x, p // tiles_x // tiles_y, p // tiles_x % tiles_y)
            x0, x1, _ = inj_lerp(W, Wg)
            y0, y1, _ = inj_lerp(H, Hg)
            phs = {int(y1[min(t + TH - 1, H - 1)] - y0[t]) + 1 for t in range(0, H, TH)}
            for pw in {int(x1[min(u + 15, W - 1)] - x0[u]) + 1 for u in range(0, W, 16)}:
                for e in (-1, 0, 1):
                    m = pw_magic(pw, e)
                    assert m == 65536 // pw + 1
                    for p in range(max(64, max(phs) * pw)):      # the GCONV request divides all 64 slots, the copy loop ph * pw pixels
                        sy = (p * m) >> 16
                        assert (sy, p - sy * pw) == (p // pw, p % pw), (p, pw)
