"""mgdt_sppf_fuse_fwd: SPPF's cv1, three max-pools and cv2 in one launch (ops.FUSED_SPPF).

Every comparison is torch.equal against the three-launch route of the same build (ops.FUSED_SPPF = False: conv2d into concat slot 0, sppf_pools into
slots 1..3, conv2d over the buffer).  The fused kernel keeps that route's MFMA order, operand roles and both bf16 rounding points, and a maximum is
exact, so there is no tolerance to choose."""
import pytest
import torch

from kernel_ref import DEV, _gen
from mgdt_yolo_amd.models import get_config
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# (n, c1, c2, h, w, act1, act2, bias1)
KERNEL_CASES = [
    (1, 64, 64, 1, 1, 'silu', 'silu', None),          # the map is smaller than every window
    (2, 64, 64, 3, 2, 'silu', 'silu', None),          # ... still
    (2, 64, 96, 13, 11, 'silu', 'silu', None),        # odd sizes, c2 != c1, two ragged tiles per direction
    (3, 256, 256, 20, 20, 'silu', 'silu', None),      # the bench channels: four 10 x 10 tiles per image, 16 x 16 regions
    (2, 256, 256, 27, 23, 'silu', 'silu', None),      # 6 x 6 tiles (what fits LDS at c_ = 128), ragged in both directions; interior tiles with the whole 18 x 18 region
    (2, 64, 64, 40, 40, 'silu', 'silu', None),        # the map of a 1280 x 1280 input: 16 tiles of 10 x 10, interior ones with the whole 22 x 22 region
    (70, 64, 64, 20, 20, 'silu', 'silu', None),       # 280 workgroups: more than the 256 compute units
    (2, 64, 64, 13, 11, 'silu', 'silu', -4.0),        # every cv1 output negative: a zero instead of -inf outside the map changes the maxima
    (2, 64, 96, 13, 11, 'relu', 'none', None),        # the other activations
    (1, 64, 64, 9, 12, 'none', 'relu', None),
]


def _nhwc(t):
    out = torch.empty(t.shape, dtype=BF16, device=DEV, memory_format=torch.channels_last)
    out.copy_(t)
    return out


def _act(name):
    from mgdt_yolo_amd import ops
    return {'relu': ops.ACT_RELU, 'silu': ops.ACT_SILU, 'none': ops.ACT_NONE}[name]


def _unfused(ops, x, pk1, a1, pk2, a2, out):
    n, _, h, w = x.shape
    cm = pk1.cout
    cat = torch.empty(n, 4 * cm, h, w, dtype=BF16, device=DEV, memory_format=torch.channels_last)
    ops.conv2d(x, pk1, 1, a1, out=cat[:, :cm])
    ops.sppf_pools(cat[:, :cm], cat[:, cm:2 * cm], cat[:, 2 * cm:3 * cm], cat[:, 3 * cm:])
    ops.conv2d(cat, pk2, 1, a2, out=out)
    return cat


@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 'n%d_c%d_c%d_%dx%d_%s_%s_b%s' % c)
def test_kernel_equals_three_launches(case):
    """Random bf16 input, random panels with a non-zero bias.  The input is a channel slice of a wider NHWC buffer, the output a channel slice of a
    wider buffer of random values: nothing outside the slice may change."""
    from mgdt_yolo_amd import ops
    n, c1, c2, h, w, a1, a2, bias1 = case
    cm = c1 // 2
    g = _gen('sppf', case)
    xbig = _nhwc(torch.randn(n, c1 + 16, h, w, generator=g))
    x = xbig[:, 8:8 + c1]
    big0 = torch.randn(n, c2 + 24, h, w, generator=g).to(BF16)
    w1 = torch.randn(cm, c1, 1, 1, generator=g) * c1 ** -0.5 * (1.0 if bias1 is None else 0.5)      # bias -4: the pre-activations are -4 +- 0.5
    b1 = torch.randn(cm, generator=g) if bias1 is None else torch.full((cm,), bias1)
    w2, b2 = torch.randn(c2, 4 * cm, 1, 1, generator=g) * (4 * cm) ** -0.5, torch.randn(c2, generator=g)
    pk1 = ops.PackedConv(w1.to(DEV), b1.to(DEV), None, 1, BF16)
    pk2 = ops.PackedConv(w2.to(DEV), b2.to(DEV), None, 1, BF16)
    assert ops.FUSED_SPPF
    res = {}
    for fused in (False, True):
        big = _nhwc(big0)
        out = big[:, 8:8 + c2]
        if fused:
            assert ops.sppf_fuse_supported(x, cm, c2, _act(a1), _act(a2), BF16)
            ops.sppf_fuse(x, pk1, _act(a1), pk2, _act(a2), out=out)
        else:
            cat = _unfused(ops, x, pk1, _act(a1), pk2, _act(a2), out)
            if bias1 is not None:
                assert (cat[:, :cm].float() < 0).all()
        torch.cuda.synchronize()
        res[fused] = big.cpu()
    bigf, bigr = res[True], res[False]
    assert torch.isfinite(bigr.float()).all()
    assert torch.equal(bigf[:, 8:8 + c2], bigr[:, 8:8 + c2])
    mask = torch.ones(big0.shape, dtype=torch.bool)
    mask[:, 8:8 + c2] = False
    assert torch.equal(bigf[mask], big0[mask]) and torch.equal(bigr[mask], big0[mask]), 'written outside the output view'


def test_unsupported_shapes_are_refused():
    """What the kernel does not take is refused by sppf_fuse_supported (no launch) and by the entry point itself."""
    from mgdt_yolo_amd import ops
    mk = lambda c, h, w: torch.zeros(1, c, h, w, dtype=BF16, device=DEV).contiguous(memory_format=torch.channels_last)
    silu = ops.ACT_SILU
    assert ops.sppf_fuse_supported(mk(64, 4, 4), 32, 64, silu, silu, BF16)
    assert ops.sppf_fuse_supported(mk(256, 4, 4), 128, 256, silu, silu, BF16)
    assert not ops.sppf_fuse_supported(mk(128, 4, 4), 64, 128, silu, silu, BF16)                         # channel counts without an instantiation
    assert not ops.sppf_fuse_supported(mk(64, 4, 4), 32, 80, silu, silu, BF16)
    assert not ops.sppf_fuse_supported(mk(64, 4, 4), 16, 64, silu, silu, BF16)                           # cv1 is not c1 -> c1 / 2
    assert not ops.sppf_fuse_supported(mk(64, 4, 4), 32, 64, ops.ACT_GELU, silu, BF16)                   # an activation it does not know
    assert not ops.sppf_fuse_supported(mk(64, 4, 4).float(), 32, 64, silu, silu, torch.float32)          # fp32
    assert not ops.sppf_fuse_supported(torch.zeros(1, 64, 4, 4, dtype=BF16, device=DEV), 32, 64, silu, silu, BF16)   # NCHW
    pk1 = ops.PackedConv(torch.zeros(64, 128, 1, 1, device=DEV), None, None, 1, BF16)
    pk2 = ops.PackedConv(torch.zeros(128, 256, 1, 1, device=DEV), None, None, 1, BF16)
    with pytest.raises(RuntimeError):
        ops.sppf_fuse(mk(128, 4, 4), pk1, silu, pk2, silu)
    pk1 = ops.PackedConv(torch.zeros(32, 64, 1, 1, device=DEV), None, None, 1, BF16)
    pk2 = ops.PackedConv(torch.zeros(64, 128, 1, 1, device=DEV), None, None, 1, BF16)
    with pytest.raises(RuntimeError):                                                                     # a view that is not NHWC
        ops.sppf_fuse(torch.zeros(1, 64, 4, 4, dtype=BF16, device=DEV), pk1, silu, pk2, silu, out=mk(64, 4, 4))
    pk1f = ops.PackedConv(torch.zeros(32, 64, 1, 1, device=DEV), None, None, 1, torch.float32)
    pk2f = ops.PackedConv(torch.zeros(64, 128, 1, 1, device=DEV), None, None, 1, torch.float32)
    with pytest.raises(RuntimeError):                                                                     # fp32
        ops.sppf_fuse(mk(64, 4, 4).float(), pk1f, silu, pk2f, silu)


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
    ops.FUSED_SPPF = False
    try:
        return fn()
    finally:
        ops.FUSED_SPPF = True


@pytest.mark.parametrize('kind', ['SPPF', 'SPP'])
def test_module_route(kind):
    """SPPF(64, 96) / SPP(64, 96), eval, bf16: one sppf_fuse_fwd launch in place of conv2d_fwd, sppf_pool_fwd and conv2d_fwd, the same values; a
    forward hook on cv1, an fp8 site table on it, fp32 input or channel counts the kernel has no instantiation for send the module back to the
    separate launches."""
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.nn import modules
    m = seed_state_dict_(getattr(modules, kind)(64, 96), 3).eval().to(DEV)
    g = _gen('sppf module', kind)
    x = _nhwc(torch.randn(2, 64, 13, 9, generator=g))
    with torch.no_grad():
        m(x)                                                  # panels are packed on first use
        ref, n0 = _off(lambda: _names_of(lambda: m(x).clone()))
        got, n1 = _names_of(lambda: m(x).clone())
        assert n0 == ['conv2d_fwd', 'sppf_pool_fwd', 'conv2d_fwd'], n0
        assert n1 == ['sppf_fuse_fwd'], n1
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
        _, n5 = _names_of(lambda: m(x.float()))               # fp32 keeps the three launches
        assert 'sppf_fuse_fwd' not in n5 and n5.count('sppf_pool_fwd') == 1, n5
        m2 = seed_state_dict_(getattr(modules, kind)(128, 128), 4).eval().to(DEV)     # no instantiation: refused, the unfused result
        x2 = _nhwc(torch.randn(1, 128, 6, 7, generator=g))
        got2, n6 = _names_of(lambda: m2(x2).clone())
        ref2 = _off(lambda: m2(x2).clone())
        assert 'sppf_fuse_fwd' not in n6 and torch.equal(got2, ref2), n6


def _flat(o):
    if o is None:                                             # augment=True returns (y, None)
        return []
    if torch.is_tensor(o):
        return [o]
    return [t for e in o for t in _flat(e)]


@pytest.fixture(scope='module', params=['mspa_c2f_gd_yolov8', 'yolov8', 'yolov3-spp'])
def model(request):
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(get_config(request.param, 'n', 80), verbose=False)
    seed_state_dict_(m, 0)
    return request.param, m.eval().to(DEV).set_compute_dtype(BF16)


@pytest.mark.parametrize('shape', [(2, 160, 160), (1, 320, 320)])
def test_model_equal_with_and_without(model, shape):
    """The seeded models in bf16 (P5 maps of 5 x 5 and 10 x 10): y and every raw map equal with the flag on and off - eagerly, inside
    torch.inference_mode(), with augment=True, and from one captured graph replayed on a second input."""
    name, m = model
    xs = [seeded_images(shape[0], shape[1], shape[2], seed=s).to(DEV).to(BF16) for s in (11, 12)]
    eq = lambda a, b: len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    with torch.no_grad():
        m(xs[0])
        ref, names0 = _off(lambda: _names_of(lambda: [[t.clone() for t in _flat(m(x))] for x in xs]))
        got, names = _names_of(lambda: [t.clone() for t in _flat(m(xs[0]))])
        if name != 'yolov3-spp':                              # the n-scale SPPF is 256 -> 128 -> 256; YOLOv3-SPP's 512 -> 256 -> 512 has no instantiation
            assert names.count('sppf_fuse_fwd') == 1 and 'sppf_pool_fwd' not in names and 'sppf_fuse_fwd' not in names0, names
            assert 2 * len(names) == len(names0) - 4, (names0, names)
        assert eq(got, ref[0])
        ref_aug = _off(lambda: [t.clone() for t in _flat(m(xs[0], augment=True))])
        assert eq([t.clone() for t in _flat(m(xs[0], augment=True))], ref_aug)
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
            assert eq(out, r)
    with torch.inference_mode():
        assert eq(_flat(m(xs[1].clone())), ref[1])
