"""mgdt_laf_fuse_fwd: SimFusion_3in's cv1, bilinear up-sampling and cv_fuse in one launch (ops.FUSED_LAF).

Every comparison is torch.equal against the three-launch route of the same build (ops.FUSED_LAF = False: conv2d into concat slot 0, bilinear into
slot 2, conv2d over the buffer).  The fused kernel keeps that route's MFMA order, operand roles and both bf16 rounding points and shares its
interpolation arithmetic (csrc/resample.h), so there is no tolerance to choose."""
import pytest
import torch

from kernel_ref import DEV, _gen
from mgdt_yolo_amd.models import get_config
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# (n, h, w, h2, w2, c0, oc, act1, act2)
KERNEL_CASES = [
    (1, 2, 2, 1, 1, 32, 64, 'relu', 'relu'),          # every tap clamped, 4 of the group's 16 pixels valid
    (2, 37, 53, 13, 19, 32, 64, 'relu', 'relu'),      # odd sizes, a ratio that is not 2, a ragged last group
    (3, 24, 40, 12, 20, 32, 64, 'relu', 'relu'),      # the model's 2x ratio
    (4, 160, 160, 80, 80, 32, 64, 'relu', 'relu'),    # 1600 workgroup tiles: more than the persistent grid holds, the loop wraps
    (2, 9, 11, 4, 5, 8, 32, 'relu', 'relu'),          # cv1's K chunk zero-padded from 8 channels, one chunk per concat slot
    (2, 9, 11, 4, 5, 16, 32, 'silu', 'none'),         # ... from 16; the other activations
    (1, 9, 11, 12, 7, 40, 64, 'none', 'silu'),        # two cv1 chunks, the second one padded; x2 larger than the output in one direction
    (1, 5, 7, 5, 7, 64, 32, 'relu', 'relu'),          # two full cv1 chunks; ratio 1
]


def _nhwc(t):
    out = torch.empty(t.shape, dtype=BF16, device=DEV, memory_format=torch.channels_last)
    out.copy_(t)
    return out


def _act(name):
    from mgdt_yolo_amd import ops
    return {'relu': ops.ACT_RELU, 'silu': ops.ACT_SILU, 'none': ops.ACT_NONE}[name]


@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 'n%d_%dx%d_from_%dx%d_c%d_oc%d_%s_%s' % c)
def test_kernel_equals_three_launches(case):
    """Random bf16 inputs, random panels with a non-zero bias.  x1 is slot 1 of a 3 * oc channel buffer, the output a channel slice of a wider buffer
    of random values: nothing outside the slice may change, and the fused launch leaves slots 0 and 2 of the concat buffer alone."""
    from mgdt_yolo_amd import ops
    n, h, w, h2, w2, c0, oc, a1, a2 = case
    g = _gen('laf', case)
    p0 = _nhwc(torch.randn(n, c0, h, w, generator=g))
    x2 = _nhwc(torch.randn(n, oc, h2, w2, generator=g))
    cat0 = torch.randn(n, 3 * oc, h, w, generator=g).to(BF16)
    big0 = torch.randn(n, oc + 24, h, w, generator=g).to(BF16)
    w1, b1 = torch.randn(oc, c0, 1, 1, generator=g) * c0 ** -0.5, torch.randn(oc, generator=g)
    w2_, b2 = torch.randn(oc, 3 * oc, 1, 1, generator=g) * (3 * oc) ** -0.5, torch.randn(oc, generator=g)
    pk1 = ops.PackedConv(w1.to(DEV), b1.to(DEV), None, 1, BF16)
    pk2 = ops.PackedConv(w2_.to(DEV), b2.to(DEV), None, 1, BF16)
    assert ops.FUSED_LAF
    res = {}
    for fused in (False, True):
        cat, big = _nhwc(cat0), _nhwc(big0)
        x1, out = cat[:, oc:2 * oc], big[:, 8:8 + oc]
        if fused:
            assert ops.laf_fuse_supported(p0, x1, x2, oc, _act(a1), _act(a2), BF16)
            ops.laf_fuse(p0, x1, x2, pk1, _act(a1), pk2, _act(a2), out=out)
        else:
            ops.conv2d(p0, pk1, 1, _act(a1), out=cat[:, :oc])
            ops.bilinear(x2, cat[:, 2 * oc:])
            ops.conv2d(cat, pk2, 1, _act(a2), out=out)
        torch.cuda.synchronize()
        res[fused] = (big.cpu(), cat.cpu())
    (bigf, catf), (bigr, _) = res[True], res[False]
    assert torch.isfinite(bigr.float()).all()
    assert torch.equal(bigf[:, 8:8 + oc], bigr[:, 8:8 + oc])
    mask = torch.ones(big0.shape, dtype=torch.bool)
    mask[:, 8:8 + oc] = False
    assert torch.equal(bigf[mask], big0[mask]) and torch.equal(bigr[mask], big0[mask]), 'written outside the output view'
    assert torch.equal(catf, cat0), 'the fused launch must not write the concat buffer'


def test_unsupported_shapes_are_refused_and_fall_back():
    """What the kernel does not take is refused by laf_fuse_supported (no launch) and by the entry point itself."""
    from mgdt_yolo_amd import ops
    mk = lambda c, h, w: torch.zeros(1, c, h, w, dtype=BF16, device=DEV).contiguous(memory_format=torch.channels_last)
    relu = ops.ACT_RELU
    assert ops.laf_fuse_supported(mk(32, 4, 4), mk(64, 4, 4), mk(64, 2, 2), 64, relu, relu, BF16)
    assert not ops.laf_fuse_supported(mk(32, 4, 4), mk(48, 4, 4), mk(48, 2, 2), 48, relu, relu, BF16)          # oc not 32 / 64
    assert not ops.laf_fuse_supported(mk(96, 4, 4), mk(64, 4, 4), mk(64, 2, 2), 64, relu, relu, BF16)          # c0 > 64
    assert not ops.laf_fuse_supported(mk(32, 4, 4), mk(64, 4, 4), mk(64, 2, 2), 32, relu, relu, BF16)          # cv_fuse not 3 oc -> oc
    assert not ops.laf_fuse_supported(mk(32, 4, 4), mk(64, 4, 4), mk(64, 2, 2), 64, ops.ACT_GELU, relu, BF16)  # an activation it does not know
    assert not ops.laf_fuse_supported(mk(32, 4, 4).float(), mk(64, 4, 4).float(), mk(64, 2, 2).float(), 64, relu, relu, torch.float32)
    pk1 = ops.PackedConv(torch.zeros(48, 32, 1, 1, device=DEV), None, None, 1, BF16)
    pk2 = ops.PackedConv(torch.zeros(48, 144, 1, 1, device=DEV), None, None, 1, BF16)
    with pytest.raises(RuntimeError):
        ops.laf_fuse(mk(32, 4, 4), mk(48, 4, 4), mk(48, 2, 2), pk1, relu, pk2, relu)


def _names_of(fn):
    from mgdt_yolo_amd import ops
    names, orig = [], ops._launch
    ops._launch = lambda name, *a, **k: (names.append(name), orig(name, *a, **k))[1]
    try:
        out = fn()
    finally:
        ops._launch = orig
    return out, names


def _off(fn):
    from mgdt_yolo_amd import ops
    ops.FUSED_LAF = False
    try:
        return fn()
    finally:
        ops.FUSED_LAF = True


@pytest.mark.parametrize('hw', [(24, 40), (13, 9)])
def test_module_route(hw):
    """SimFusion_3in([32, 64, 64], 64), eval, bf16: one laf_fuse_fwd launch in place of cv1's conv2d_fwd, bilinear_fwd and cv_fuse's conv2d_fwd, the
    same values; a forward hook on cv1 or an fp8 site on it sends the module back to the separate launches.  x[2] is resampled to x[1]'s size
    whatever its own (13 x 9 from 6 x 4 is no 2x ratio); x[0] is avg-pooled first."""
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.nn.modules import SimFusion_3in
    h, w = hw
    m = seed_state_dict_(SimFusion_3in([32, 64, 64], 64), 3).eval().to(DEV)
    g = _gen('laf module', hw)
    x = [_nhwc(torch.randn(2, 32, 2 * h, 2 * w, generator=g)), _nhwc(torch.randn(2, 64, h, w, generator=g)), _nhwc(torch.randn(2, 64, h // 2, w // 2, generator=g))]
    with torch.no_grad():
        m(x)                                                  # panels are packed on first use
        ref, n0 = _off(lambda: _names_of(lambda: m(x).clone()))
        got, n1 = _names_of(lambda: m(x).clone())
        assert n0.count('bilinear_fwd') == 1 and n0.count('conv2d_fwd') == 2 and 'laf_fuse_fwd' not in n0, n0
        assert n1.count('laf_fuse_fwd') == 1 and 'bilinear_fwd' not in n1 and 'conv2d_fwd' not in n1, n1
        assert len(n0) - len(n1) == 2 and n1.count('copy_fwd') == n0.count('copy_fwd') == 1, (n0, n1)
        assert torch.equal(got, ref)
        hook = m.cv1.register_forward_hook(lambda *a: None)
        try:
            got, n2 = _names_of(lambda: m(x).clone())
        finally:
            hook.remove()
        assert n2 == n0 and torch.equal(got, ref)
        m.cv1.__dict__['_q8'] = {'elsewhere': 1.0}            # an fp8 site table on the conv (no entry for the conv itself: it still runs in bf16)
        try:
            got, n3 = _names_of(lambda: m(x).clone())
        finally:
            del m.cv1.__dict__['_q8']
        assert n3 == n0 and torch.equal(got, ref)
        got, n4 = _names_of(lambda: m(x).clone())
        assert n4 == n1 and torch.equal(got, ref)


def _flat(o):
    if torch.is_tensor(o):
        return [o]
    return [t for e in o for t in _flat(e)]


@pytest.fixture(scope='module')
def model():
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(get_config('mspa_c2f_gd_yolov8', 'n', 80), verbose=False)
    seed_state_dict_(m, 0)
    return m.eval().to(DEV).set_compute_dtype(BF16)


@pytest.mark.parametrize('shape', [(2, 320, 256), (1, 224, 352)])
def test_model_equal_with_and_without(model, shape):
    """mspa_c2f_gd_yolov8 in bf16: y and every raw map equal with the flag on and off, eagerly and from one captured graph (which keeps the side
    stream's parallel branch) replayed on a second input."""
    from mgdt_yolo_amd import ops
    m = model
    xs = [seeded_images(shape[0], shape[1], shape[2], seed=s).to(DEV).to(BF16) for s in (11, 12)]
    with torch.no_grad():
        m(xs[0])
        ref, names0 = _off(lambda: _names_of(lambda: [[t.clone() for t in _flat(m(x))] for x in xs]))
        got, names = _names_of(lambda: [t.clone() for t in _flat(m(xs[0]))])
        assert names.count('laf_fuse_fwd') == 1 and 'laf_fuse_fwd' not in names0, names
        assert 2 * len(names) == len(names0) - 4 and 2 * names.count('bilinear_fwd') == names0.count('bilinear_fwd') - 2, (names0, names)
        assert len(got) == len(ref[0]) and all(torch.equal(a, b) for a, b in zip(got, ref[0]))
        assert m._side_branch() == (12, 13, 6)
        xin = xs[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(xin)
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = _flat(m(xin))
        for x, r in zip(xs[::-1], ref[::-1]):
            xin.copy_(x)
            gr.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(out, r))
