"""The MGDT_*_DBG phase-stamp buffers (StampBuf in csrc/common.h) are sized by the launch that writes them (GPU, -m gpu).  A debug knob only adds
timestamps: with it set the outputs must equal, bit for bit, the outputs of the same calls without it - also when a later call has a larger grid
than the first one, or a grid larger than the fixed capacity the buffer once had.  The knobs are read per call, so one process runs both."""
import pytest
import torch

from kernel_ref import BF16, DEV, _gen, _nhwc, _rand
from knobs import knobs

gpu = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


@gpu
def test_dwconv7_ln_stamps_grow_with_the_grid():
    """dwconv7_ln's row kernel, 1x8x8x16 and then 2x16x16x16 bf16: the second call stamps more workgroups than the first one allocated for."""
    from mgdt_yolo_amd import ops
    shapes = [(1, 16, 8, 8), (2, 16, 16, 16)]
    routes = [ops.dwconv7_ln_route(b, h, w, c, BF16) for b, c, h, w in shapes]
    assert all(r['family'] != 'generic' for r in routes) and routes[0]['nwg'] < routes[1]['nwg'], routes
    gen = _gen('stamps-dw')
    c = 16
    args = ((torch.randn(c, 1, 7, 7, generator=gen) * 0.2).reshape(c, 49).t().contiguous().to(DEV), (torch.randn(c, generator=gen) * 0.1).to(DEV),
            (torch.rand(c, generator=gen) + 0.5).to(DEV), (torch.randn(c, generator=gen) * 0.1).to(DEV), 1e-6)
    xs = [_nhwc(_rand(gen, *s, dt=BF16), BF16)[0] for s in shapes]
    with knobs(MGDT_DW_DBG=None):
        plain = [_bits(ops.dwconv7_ln(x, *args)) for x in xs]
    with knobs(MGDT_DW_DBG='1'):
        stamped = [_bits(ops.dwconv7_ln(x, *args)) for x in xs]
    torch.cuda.synchronize()
    for s, a, b in zip(shapes, plain, stamped):
        assert torch.equal(a, b), s


@gpu
def test_spr_attention_scale_stamps_beyond_4096_workgroups():
    """spr_attention_scale launches (K, images) workgroups, K <= 12; its stamp buffer used to hold 4096 of them whatever the launch.  4097 images of
    8x8x16 (K = 1: 128 vectors per image against 2048 per workgroup) are the smallest launch past that: 4097 workgroups, 8 MB of activations."""
    from mgdt_yolo_amd import ops
    B, groups, cw, H, W = 4097, 1, 16, 8, 8
    gen = _gen('stamps-spr')
    x = _nhwc(_rand(gen, B, groups * cw, H, W, dt=BF16, shift=0.2), BF16)[0]
    hid = cw // 4
    w = [t.to(DEV).contiguous() for t in (torch.randn(hid, 5 * cw, 1, 1, generator=gen) * 0.4, torch.randn(hid, generator=gen) * 0.2,
                                           torch.randn(cw, hid, 1, 1, generator=gen) * 0.5, torch.randn(cw, generator=gen) * 0.2)]
    with knobs(MGDT_SPR_DBG=None):
        plain = _bits(ops.spr_attention_scale(x, *w, groups))
    with knobs(MGDT_SPR_DBG='1'):
        stamped = _bits(ops.spr_attention_scale(x, *w, groups))
    torch.cuda.synchronize()
    assert torch.equal(plain, stamped)
