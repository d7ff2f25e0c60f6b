"""YOLOv5 graphs (models/v5/yolov5.yaml): the C3 block, the 6x6 / stride 2 / padding 2 stem as space-to-depth + 3x3, inference and training, against the
reference-generated fixtures tests/golden/yolov5_NN.npz, yolov5_yaml.json and train_yolov5_n.npz (tests/golden/gen_yolov5.py) and against float64 torch on
the CPU.  Host-side checks run without a GPU; everything that launches a kernel is marked gpu.

Bounds.  Kernels against float64: kernel_ref._check (fp32 outputs: relative L2 <= 2e-5 and every element within 1e-4 max|ref|; bf16 outputs: 2^-8 |ref| +
1e-3 max|ref|), with the reference rounding where the kernel rounds by design (stated at the test); copies are compared exactly.  Modules against the
fixtures: 1e-4 (the project's module tolerance).  The model in fp32: boxes 1e-3 px, confidences 1e-4, head maps atol 1e-3 / rtol 1e-4 (the contract of
the other graphs).  bf16 model: 3 x the bf16 emulation error the generator recorded for the reference itself (the project's precedent for the Pose
head).  The composed C3 in bf16 against float64 autograd (the reference rounds every stored map of the forward; the reverse pass's bf16 stores are the
difference): relative L2 <= 2e-2, i.e. 2.3 - 3 x the 6.6e-3 - 8.5e-3 measured on the MI355X - a dropped or doubled shortcut gradient of one bottleneck changes
dx by tens of per cent.
"""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inputs as GI
import yolov5_ref as YR
from mgdt_yolo_amd import _lib, ops
from mgdt_yolo_amd.models import get_config
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
_FIX = []


def fixture():
    if not _FIX:
        _FIX.append(YR.load_fixture())
    return _FIX[0]


def build_model(dtype=F32, nc=80, scale='n', device=DEV, seed=0):
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    m = seed_state_dict_(DetectionModel(get_config('yolov5', scale, nc), verbose=False), seed).eval().set_compute_dtype(dtype)
    return m.to(device) if device else m


def to_nchw(t):
    return t.detach().float().contiguous().cpu().numpy()


def make_module(ctor, args, device=DEV):
    import mgdt_yolo_amd.nn.modules as M
    m = getattr(M, ctor)(*args)
    for sub in m.modules():
        if isinstance(sub, torch.nn.BatchNorm2d):
            sub.eps = 1e-3
    m = seed_state_dict_(m, YR.MODULE_SEED).eval()
    return m.to(device) if device else m


# ================================================================================================ host side (no GPU)
def test_config_equals_the_reference_yaml():
    ref = json.load(open(os.path.join(YR.GOLDEN, 'yolov5_yaml.json')))
    cfg = get_config('yolov5', 'n')
    for k in ('nc', 'scales', 'backbone', 'head'):
        assert cfg[k] == ref[k], k
    assert cfg['scales']['m'][2] == 1024 and cfg['scales']['x'][0] == 1.33            # unlike the v8 files
    assert get_config('yolov5', 's', 3)['nc'] == 3 and get_config('yolov5', 's', 3)['scale'] == 's'


def test_parse_model_gives_the_reference_structure():
    from mgdt_yolo_amd.nn.tasks import DetectionModel, guess_model_task, model_class_of, yaml_model_load
    g = fixture()
    m = build_model(device=None)
    sd = m.state_dict()
    assert list(sd.keys()) == g['keys'].tolist()
    assert [','.join(map(str, v.shape)) for v in sd.values()] == g['shapes'].tolist()
    assert sum(p.numel() for p in m.parameters()) == int(g['nparams'])
    assert m.stride.tolist() == g['stride'].tolist() == [8.0, 16.0, 32.0]
    assert guess_model_task(m) == 'detect' and guess_model_task(m.yaml) == 'detect' and guess_model_task('yolov5n.yaml') == 'detect'
    assert model_class_of(m.yaml) is DetectionModel
    d = yaml_model_load('yolov5s.yaml')                                               # resolves without a file
    assert d['scale'] == 's' and d['backbone'][0] == [-1, 1, 'Conv', [64, 6, 2, 2]] and d['backbone'][2] == [-1, 3, 'C3', [128]]
    s = DetectionModel('yolov5s.yaml', verbose=False)
    assert s.model[0].conv.out_channels == 32 and len(s.model[4].m) == 2 and s.model[2].cv3.conv.out_channels == 64
    x = DetectionModel(get_config('yolov5', 'x'), verbose=False)                     # depth 1.33: the 9-deep row becomes 12 bottlenecks
    assert len(x.model[6].m) == 12 and x.model[0].conv.out_channels == 80


def test_c3_state_dict_keys_are_the_reference_ones():
    g = fixture()
    for name, (args, _) in YR.C3_CASES.items():
        m = make_module('C3', args, device=None)
        assert list(m.state_dict().keys()) == g[f'{name}_keys'].tolist(), name
        assert m.c == int(args[1] * 0.5) and len(m.m) == args[2] and all(b.add == args[3] for b in m.m)
        assert all(b.cv1.conv.kernel_size == (1, 1) and b.cv2.conv.kernel_size == (3, 3) for b in m.m)


def test_stem_weight_permutation_and_its_inverse_in_float64():
    """conv2d(x, W6, stride 2, pad 2) == conv2d(S, W3, stride 1, pad 1) with the layouts the kernels use, on the fixture's own stem weights."""
    gen = torch.Generator().manual_seed(5)
    for c, co in ((3, 16), (4, 8), (1, 4)):
        w6 = torch.randn(co, c, 6, 6, generator=gen, dtype=torch.float64)
        if c == 3:
            from mgdt_yolo_amd.seeding import seeded_tensor
            w6 = seeded_tensor('conv.weight', (co, c, 6, 6), YR.MODULE_SEED).double()
        x = torch.randn(2, c, 10, 14, generator=gen, dtype=torch.float64)
        w3 = ops.stem6_w3(w6)
        assert torch.equal(w3, YR.w6_to_w3(w6)) and torch.equal(ops.stem6_w6(w3, c), w6)
        w3p = ops.stem6_w3(w6, 4 * c + 4)
        assert torch.equal(w3p[:, :4 * c], w3) and w3p[:, 4 * c:].abs().max() == 0 and torch.equal(ops.stem6_w6(w3p, c), w6)
        ref = F.conv2d(x, w6, stride=2, padding=2)
        got = F.conv2d(YR.space_to_depth2(x), w3, stride=1, padding=1)
        assert (got - ref).abs().max().item() < 1e-13
        got = F.conv2d(YR.space_to_depth2(x, 4 * c + 4), w3p, stride=1, padding=1)
        assert (got - ref).abs().max().item() < 1e-13


def test_stem_geometry_is_accepted_and_others_keep_raising():
    from mgdt_yolo_amd.nn.modules import Conv
    assert Conv(3, 16, 6, 2, 2)._geometry() == (6, 2) and Conv(4, 16, 6, 2, 2)._geometry() == (6, 2) and Conv(3, 16, 3, 2)._geometry() == (3, 2)
    for args in ((8, 16, 6, 2, 2), (3, 16, 6, 1, 2), (3, 16, 6, 2, 1), (3, 16, 4, 2, 1), (3, 16, 2, 2, 0), (3, 16, 6, 2, 2, 1, 2)):
        with pytest.raises(RuntimeError, match='outside the built kernels'):
            Conv(*args)._geometry()
    m = Conv(3, 16, 6, 2, 2).eval()
    for shape in ((1, 3, 33, 48), (1, 3, 32, 47), (1, 4, 32, 48)):                  # odd sizes / another channel count: refused before any launch
        with pytest.raises(RuntimeError, match='even H and W'):
            m(torch.zeros(shape))
    with pytest.raises(RuntimeError, match='even height and width'):
        ops.space_to_depth2(torch.zeros(1, 3, 5, 8), F32)


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'mgdt.h')).read()
    declared = set(re.findall(r'\b(mgdt_[a-z0-9_]+)\s*\(', hdr))
    lib = _lib.lib()
    for name in ('mgdt_space_to_depth2_fwd', 'mgdt_space_to_depth2_channels', 'mgdt_conv_pack_stem6', 'mgdt_stem6_wgrad_unpack'):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert [lib.mgdt_space_to_depth2_channels(c, dt) for c in (1, 2, 3, 4) for dt in (_lib.F32, _lib.BF16)] == [4, 8, 8, 8, 12, 16, 16, 16]
    assert all(lib.mgdt_space_to_depth2_channels(c, ops.dtype_code(dt)) == ops.space_to_depth2_channels(c, dt) for c in (1, 2, 3, 4) for dt in (F32, BF16))
    # refusals happen on the host, before any GPU call: null arguments, odd sizes, a wrong output channel count, a misaligned output
    assert lib.mgdt_space_to_depth2_fwd(None, 0, None, 0, None) == -4
    assert lib.mgdt_conv_pack_stem6(None, None, None, None, None, None, 0.0, 3, 16, 0, None, None, None) == -4
    assert lib.mgdt_stem6_wgrad_unpack(None, 16, 3, 12, None, None) == -4
    x = lambda h, w, c=3: _lib.View(4096, 1, h, w, c, c * h * w, w, 1, h * w)
    y = lambda h, w, c, p=4096: _lib.View(p, 1, h, w, c, h * w * c, w * c, c, 1)
    assert lib.mgdt_space_to_depth2_fwd(x(7, 8), 0, y(3, 4, 12), 0, None) == -1
    assert lib.mgdt_space_to_depth2_fwd(x(8, 8), 0, y(4, 4, 16), 0, None) == -1
    assert lib.mgdt_space_to_depth2_fwd(x(8, 8), 0, y(4, 4, 12, 4100), 0, None) == -1
    assert lib.mgdt_space_to_depth2_fwd(x(8, 8, 5), 0, y(4, 4, 20), 0, None) == -1
    assert lib.mgdt_space_to_depth2_fwd(x(8, 8), 1, y(4, 4, 12), 0, None) == -2        # a bf16 image goes to a bf16 map only


# ================================================================================================ GPU: kernels
S2D_PAIRS = [pytest.param(torch.uint8, F32, id='u8-f32'), pytest.param(torch.uint8, BF16, id='u8-bf16'), pytest.param(F32, F32, id='f32-f32'),
             pytest.param(F32, BF16, id='f32-bf16'), pytest.param(BF16, BF16, id='bf16-bf16')]


def _image(shape, dt, seed):
    r = np.random.default_rng([seed, 3])
    if dt == torch.uint8:
        return torch.from_numpy(r.integers(0, 256, shape, dtype=np.uint8))
    return torch.from_numpy(r.random(shape, dtype=np.float32)).to(dt)


@pytest.mark.gpu
@pytest.mark.parametrize('xdt,ydt', S2D_PAIRS)
@pytest.mark.parametrize('shape', [(2, 3, 8, 12), (1, 3, 34, 50), (2, 4, 6, 10), (3, 1, 4, 6)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('layout', ['nchw', 'nhwc', 'rows'])
def test_space_to_depth2(shape, xdt, ydt, layout):
    """Bit-equal to the indexing formula, pad channels exactly zero; uint8 is /255 in fp32 (then rounded once for bf16).  nchw: two-pixel loads;
    nhwc (pixel stride C) and rows (odd row stride) take the scalar loads."""
    x = _image(shape, xdt, 1)
    b, c, h, w = shape
    if layout == 'nchw':
        xd = x.to(DEV)
    elif layout == 'nhwc':
        xd = x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    else:
        big = torch.zeros(b, c, h, w + 1, dtype=xdt, device=DEV)
        big[..., :w] = x.to(DEV)
        xd = big[..., :w]
    cp = ops.space_to_depth2_channels(c, ydt)
    assert cp == {F32: {1: 4, 3: 12, 4: 16}, BF16: {1: 8, 3: 16, 4: 16}}[ydt][c]
    out = torch.full((b, cp, h // 2, w // 2), float('nan'), dtype=ydt, device=DEV).contiguous(memory_format=torch.channels_last)
    got = ops.space_to_depth2(xd, ydt, out=out)
    xf = (x.float() / 255.0) if xdt == torch.uint8 else x.float()
    ref = YR.space_to_depth2(xf, cp).to(ydt)
    assert got.dtype == ydt and got.stride(1) == 1 and tuple(got.shape) == (b, cp, h // 2, w // 2)
    assert torch.equal(got.cpu(), ref)
    if cp > 4 * c:
        assert got[:, 4 * c:].abs().max().item() == 0
    assert torch.equal(ops.space_to_depth2(xd, ydt).cpu(), ref)                       # the allocating form


def _stem():
    return make_module('Conv', YR.STEM_ARGS)


def _stem_ref64(m, x, dt):
    """float64 F.conv2d(x, W6, stride 2, padding 2) + BN + SiLU with the kernel's rounding points: the image and the (folded) weight in the compute dtype"""
    from kernel_ref import _fold, _silu
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    xq = x.to(dt).double()
    bn = (sd['bn.weight'], sd['bn.bias'], sd['bn.running_mean'], sd['bn.running_var'], m.bn.eps)
    wq, bq = _fold(sd['conv.weight'], None, bn, dt)
    return _silu(F.conv2d(xq, wq, bq, 2, 2))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
@pytest.mark.parametrize('kind', ['float', 'u8'])
def test_stem_conv_against_float64(dt, kind):
    from kernel_ref import _check
    m = _stem()
    m._cdtype = dt
    xf, xu = YR.stem_inputs()
    x = xf if kind == 'float' else xu
    names = []
    orig = ops._launch
    ops._launch = lambda name, *a, **k: (names.append(name), orig(name, *a, **k))[1]
    try:
        with torch.no_grad():
            y = m(x.to(DEV))
    finally:
        ops._launch = orig
    assert names == ['space_to_depth2_fwd', 'conv_pack', 'conv2d_fwd'], names       # the MFMA implicit GEMM, not the direct kernel
    assert y.dtype == dt and tuple(y.shape) == (2, 16, 16, 24)
    ref = _stem_ref64(m, xf if kind == 'float' else xu.float() / 255.0, dt)
    _check(y, ref, dt, f'stem {kind}')
    with torch.no_grad():
        assert torch.equal(m(x.to(DEV)), y)                                           # the cached panel


@pytest.mark.gpu
def test_stem_conv_matches_the_reference_fixture():
    g = fixture()
    m = _stem()
    xf, xu = YR.stem_inputs()
    with torch.no_grad():
        np.testing.assert_allclose(to_nchw(m(xf.to(DEV))), g['stem_y_float'], atol=1e-4, rtol=1e-4)
        np.testing.assert_allclose(to_nchw(m(xu.to(DEV))), g['stem_y_u8'], atol=1e-4, rtol=1e-4)
        y1 = m(xf.to(DEV))
        # fuse(): bn folded into the conv (weight + bias) gives the same panel up to the fold's rounding
        from mgdt_yolo_amd.yolo.utils.torch_utils import fuse_conv_and_bn
        m.conv = fuse_conv_and_bn(m.conv, m.bn)
        del m.bn
        m.__dict__.pop('_pk', None)
        np.testing.assert_allclose(to_nchw(m(xf.to(DEV))), to_nchw(y1), atol=2e-5, rtol=0)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
def test_stem_train_step_against_float64_autograd(dt):
    """train_fwd + backward(need_dx=False): output, dW in its (cout, 3, 6, 6) layout, dgamma, dbeta and the running statistics against float64 autograd of
    silu(batch_norm(conv2d(x, W6, 2, 2))) under kernel_ref._close (the bound test_reverse_kernels.py holds conv_wgrad to).  bf16: the reference rounds the
    image, the weight, the raw convolution output and dy where the kernels store them.  A second step after an in-place weight change (behind torch's
    back, as the HIP optimizer does it) must see the new weights."""
    from kernel_ref import _close
    m = _stem().train()
    m._cdtype = dt
    xf, _ = YR.stem_inputs()
    gen = torch.Generator().manual_seed(77)
    gz = torch.randn(2, 16, 16, 24, generator=gen).to(dt)
    rb = (lambda t: t.to(BF16).double()) if dt == BF16 else (lambda t: t)

    def reference():
        sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        w = sd['conv.weight'].clone().requires_grad_(True)
        ga, be = sd['bn.weight'].clone().requires_grad_(True), sd['bn.bias'].clone().requires_grad_(True)
        xq = xf.to(dt).double()
        y = F.conv2d(xq, rb(w.detach()) if dt == BF16 else w, None, 2, 2)
        if dt == BF16:                       # the raw map is stored in bf16: batch statistics, BN and the weight gradient's dy all start from the rounded map
            yq = rb(y.detach()).requires_grad_(True)
            z = F.silu(F.batch_norm(yq, None, None, ga, be, True, 0.0, m.bn.eps))
            z.backward(gz.double())
            dy = rb(yq.grad)
            dw = torch.nn.grad.conv2d_weight(xq, (16, 3, 6, 6), dy, stride=2, padding=2)
            mean, var = yq.detach().mean((0, 2, 3)), yq.detach().var((0, 2, 3), unbiased=True)
        else:
            z = F.silu(F.batch_norm(y, None, None, ga, be, True, 0.0, m.bn.eps))
            z.backward(gz.double())
            dw = w.grad
            mean, var = y.detach().mean((0, 2, 3)), y.detach().var((0, 2, 3), unbiased=True)
        mom = m.bn.momentum
        return z.detach(), dw, ga.grad, be.grad, (1 - mom) * sd['bn.running_mean'] + mom * mean, (1 - mom) * sd['bn.running_var'] + mom * var

    def step():
        ref = reference()
        with ops.force_ctx():
            z = m(xf.to(DEV).to(dt))
        with ops.defer_wgrad():              # as the model's reverse pass runs it: the inverse permutation must read final sums
            assert m.backward(gz.to(DEV).contiguous(memory_format=torch.channels_last), need_dx=False) is None
        assert tuple(m.conv.weight.grad.shape) == (16, 3, 6, 6)
        _close(z, ref[0], dt, 'z')
        _close(m.conv.weight.grad, ref[1], F32, 'dW')
        _close(m.bn.weight.grad, ref[2], F32, 'dgamma')
        _close(m.bn.bias.grad, ref[3], F32, 'dbeta')
        _close(m.bn.running_mean, ref[4], F32, 'running_mean')
        _close(m.bn.running_var, ref[5], F32, 'running_var')
        return z

    z0 = step()
    g_eager = m.conv.weight.grad.clone()
    with ops.force_ctx():
        m(xf.to(DEV).to(dt))
    m.backward(gz.to(DEV).contiguous(memory_format=torch.channels_last), need_dx=False)       # the immediate form gives the same bits
    assert torch.equal(m.conv.weight.grad, g_eager)
    with torch.no_grad():
        m.conv.weight.data.mul_(1.5)         # .data: no version bump either way; the panel cache must key on the bytes' epoch
    ops.PARAM_EPOCH[0] += 1                  # what the trainer does after the HIP optimizer moved the weights
    z1 = step()
    assert not torch.equal(z0, z1)
    with ops.force_ctx():
        m(xf.to(DEV).to(dt))
    with pytest.raises(RuntimeError, match='no data gradient'):
        m.backward(gz.to(DEV).contiguous(memory_format=torch.channels_last))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
def test_stem_panel_is_refreshed_in_place_by_repack_all(dt):
    """The 3x3 panel is packed from the live 6x6 weight: when the weight's storage is registered as live (what FlatState does), ops.repack_all() after a
    step rewrites the same panel object, bit-equal to a fresh pack, with no rebuild."""
    m = _stem().train()
    m._cdtype = dt
    store = m.conv.weight.data.untyped_storage().data_ptr()
    ops.LIVE_STORAGES.add(store)
    try:
        pk = m._stem6_packed(dt, False, raw=True)
        assert ops.pack_is_current(pk)
        m.conv.weight.data.mul_(0.5)
        ops.PARAM_EPOCH[0] += 1
        assert pk in ops.repack_all() and ops.pack_is_current(pk)
        assert m._stem6_packed(dt, False, raw=True) is pk
        fresh = ops.PackedStem6(m.conv.weight, None, None, dt)
        derived = ops.PackedConv(ops.stem6_w3(m.conv.weight, ops.space_to_depth2_channels(3, dt)), None, None, 3, dt)
        n = derived.w.numel() - 16 * 4                                               # the panel (the scale scratch behind it is never written)
        assert fresh.w.numel() == pk.w.numel() == derived.w.numel()
        assert torch.equal(fresh.w[:n], pk.w[:n]) and torch.equal(fresh.bias, pk.bias)
        assert torch.equal(derived.w[:n], pk.w[:n]) and torch.equal(derived.bias, pk.bias)
    finally:
        ops.LIVE_STORAGES.discard(store)


# ================================================================================================ GPU: C3
@pytest.mark.gpu
@pytest.mark.parametrize('name', list(YR.C3_CASES))
def test_c3_fp32_matches_the_reference_fixture(name):
    g = fixture()
    args, shape = YR.C3_CASES[name]
    m = make_module('C3', args)
    x = YR.case_input(name, shape).to(DEV).contiguous(memory_format=torch.channels_last)
    names = []
    orig = ops._launch
    ops._launch = lambda nm, *a, **k: (names.append(nm), orig(nm, *a, **k))[1]
    try:
        with torch.no_grad():
            y = m(x)
    finally:
        ops._launch = orig
    np.testing.assert_allclose(to_nchw(y), g[f'{name}_y'], atol=1e-4, rtol=1e-4)
    n = args[2]
    assert [k for k in names if k != 'conv_pack'] == ['conv2d_fwd'] * (3 + 2 * n), names       # no copy, concat or add launches
    # the fused (BN folded by model.fuse()) form computes the same
    from mgdt_yolo_amd.nn.modules import Conv
    from mgdt_yolo_amd.yolo.utils.torch_utils import fuse_conv_and_bn
    for sub in m.modules():
        if isinstance(sub, Conv):
            sub.conv = fuse_conv_and_bn(sub.conv, sub.bn)
            del sub.bn
            sub.__dict__.pop('_pk', None)
    with torch.no_grad():
        np.testing.assert_allclose(to_nchw(m(x)), to_nchw(y), atol=5e-5, rtol=0)


def _c3_torch(sd, x, n, add, eps=1e-3, rnd=lambda t: t):
    """C3 in training mode from functional torch ops (float64): `rnd` rounds where the composed route stores a map (raw conv output, BN + act output)"""
    def cba(t, p, k, res=None):
        y = rnd(F.conv2d(t, rnd(sd[p + '.conv.weight']), None, 1, k // 2))
        z = F.silu(F.batch_norm(y, None, None, sd[p + '.bn.weight'], sd[p + '.bn.bias'], True, 0.0, eps))
        return rnd(z if res is None else z + res)
    a = cba(x, 'cv1', 1)
    for j in range(n):
        a = cba(cba(a, f'm.{j}.cv1', 1), f'm.{j}.cv2', 3, a if add else None)
    return cba(torch.cat([a, cba(x, 'cv2', 1)], 1), 'cv3', 1)


class _STE(torch.autograd.Function):
    """round to bf16 in the forward, identity gradient"""
    @staticmethod
    def forward(ctx, t):
        return t.to(BF16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
@pytest.mark.parametrize('args,shape', [((32, 32, 1, True), (2, 32, 9, 13)), ((64, 48, 3, True), (2, 64, 6, 10)), ((48, 32, 1, False), (2, 48, 8, 12))],
                         ids=['n1-sc', 'n3-sc', 'n1-nosc'])
def test_c3_composed_route_against_float64_autograd(args, shape, dt):
    """Training-mode forward + explicit reverse pass of the composed route: output, dx and every parameter gradient against float64 autograd.  fp32: relative L2
    <= 2e-4 for the output and 2e-3 for gradients (the bounds test_module_backward_matches_cpu_autograd holds the other blocks to).  bf16: the reference
    rounds the input, the weights and every stored map of the forward; bound 2e-2 relative L2 (measured: output 0 - 5.5e-3, worst gradient 6.6e-3 / 8.5e-3 /
    6.6e-3 for the three cases; module docstring)."""
    n, add = args[2], args[3]
    m = make_module('C3', args).train()
    m.apply(lambda s: setattr(s, '_cdtype', dt) if hasattr(s, 'out_dtype') else None)
    x = YR.case_input('c3-train', shape)
    gen = torch.Generator().manual_seed(9)
    gy = torch.randn(shape[0], args[1], shape[2], shape[3], generator=gen).to(dt)
    sd = {k: v.detach().cpu().double().requires_grad_('running' not in k and 'tracked' not in k) for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    xr = x.to(dt).double().requires_grad_(True)
    y_ref = _c3_torch(sd, xr, n, add, rnd=_STE.apply if dt == BF16 else (lambda t: t))
    y_ref.backward(gy.double())
    with ops.force_ctx():
        y = m(x.to(DEV).to(dt).contiguous(memory_format=torch.channels_last))
    dx = m.backward(gy.to(DEV).contiguous(memory_format=torch.channels_last))
    assert all(not mod.__dict__.get('_ctx') for mod in m.modules())
    rel = lambda a, b: (a.detach().double().cpu() - b.detach().double()).norm().item() / max(b.detach().double().norm().item(), 1e-30)
    b_out, b_grad = (2e-4, 2e-3) if dt == F32 else (2e-2, 2e-2)
    worst = (rel(dx.float().contiguous(), xr.grad), 'dx')
    assert y.dtype == dt and rel(y.float().contiguous(), y_ref) < b_out, ('y', rel(y.float().contiguous(), y_ref))
    assert worst[0] < b_grad, worst
    gscale = float(np.median([v.grad.abs().max().item() for v in sd.values() if v.grad is not None]))
    for k, p in m.named_parameters():
        r = sd[k].grad
        assert p.grad is not None and r is not None, k
        # a gradient whose reference is analytically ~0 is rounding noise on both sides: measured against max(|r|, 1 % of the typical gradient)
        e = (p.grad.cpu().double() - r).norm().item() / max(r.norm().item(), 1e-2 * gscale * r.numel() ** 0.5)
        worst = max(worst, (e, k))
        assert e < b_grad, (k, e)
    print(f'C3 composed {args} {dt}: y rel {rel(y.float().contiguous(), y_ref):.3e} (bound {b_out:.3e}), worst gradient {worst[0]:.3e} at {worst[1]} (bound {b_grad:.3e})')


# ================================================================================================ GPU: the model
@pytest.mark.gpu
def test_e2e_fp32_matches_the_reference():
    """Boxes within 1e-3 px, confidences within 1e-4, head maps atol 1e-3 / rtol 1e-4; every 25th anchor at 640^2; the fused model computes the same."""
    g = fixture()
    m = build_model()
    for shape, sub in YR.E2E_SHAPES.items():
        key = 'x'.join(map(str, shape))
        x = seeded_images(*shape, seed=YR.IMG_SEED).to(DEV)
        with torch.no_grad():
            y, feats = m(x)
        assert y.shape[-1] == int(g[f'{key}_anchors'])
        y = y.cpu().numpy()
        ref = g[f'{key}_y'] if sub == 1 else g[f'{key}_ysub']
        np.testing.assert_allclose(y[:, :4, ::sub], ref[:, :4], atol=1e-3, rtol=0)
        np.testing.assert_allclose(y[:, 4:, ::sub], ref[:, 4:], atol=1e-4, rtol=0)
        if sub == 1:
            for i, f in enumerate(feats):
                np.testing.assert_allclose(to_nchw(f), g[f'{key}_feat{i}'], atol=1e-3, rtol=1e-4)
    x = seeded_images(2, 160, 224, seed=YR.IMG_SEED).to(DEV)
    with torch.no_grad():
        yf, _ = m.fuse()(x)
    assert m.is_fused() and not hasattr(m.model[0], 'bn')
    np.testing.assert_allclose(yf.cpu().numpy()[:, :4], g['2x160x224_yfused'][:, :4], atol=1e-3, rtol=0)
    np.testing.assert_allclose(yf.cpu().numpy()[:, 4:], g['2x160x224_yfused'][:, 4:], atol=1e-4, rtol=0)


@pytest.mark.gpu
def test_nms_rows_equal_the_oracle_pipeline_on_the_same_y():
    from mgdt_yolo_amd.yolo.utils.ops import nms_with_index
    from oracle import nms as ON
    m = build_model()
    with torch.no_grad():
        y, _ = m(seeded_images(2, 160, 224, seed=YR.IMG_SEED).to(DEV))
    total = 0
    for kw in (dict(conf_thres=0.25, iou_thres=0.7), dict(conf_thres=0.001, iou_thres=0.7, multi_label=True), dict(conf_thres=0.2, iou_thres=0.45, agnostic=True, max_det=50)):
        rows, kept = nms_with_index(y, **kw)
        orows, okept = ON.non_max_suppression(y.cpu().numpy(), return_index=True, **kw)
        for i in range(2):
            assert np.array_equal(kept[i].cpu().numpy().astype(np.int64), okept[i][0])
            assert np.array_equal(rows[i].cpu().numpy(), orows[i])
            total += len(okept[i][0])
    assert total > 0


@pytest.mark.gpu
def test_e2e_bf16_within_three_times_the_reference_emulation_error():
    """bf16 model against the reference's fp32 output: boxes, confidences and head maps within 3 x the error the reference shows when its own weights and
    layer outputs are rounded to bfloat16 (recorded by the generator: 0.19 - 0.24 px, 1.5e-3, 3.1e-2, i.e. bounds 0.56 - 0.71 px, 4.5e-3, 9.1e-2).  Measured
    on the MI355X: boxes 0.099 - 0.134 px, confidences 7.7e-4 - 8.1e-4, head maps 1.6e-2, the same to the printed digits for the fused model."""
    g = fixture()
    for fuse in (False, True):
        m = build_model(BF16)
        if fuse:
            m.fuse()
        for shape, sub in YR.E2E_SHAPES.items():
            key = 'x'.join(map(str, shape))
            x = seeded_images(*shape, seed=YR.IMG_SEED).to(DEV)
            with torch.no_grad():
                y, feats = m(x)
            y = y.cpu().numpy()
            ref = g[f'{key}_y'] if sub == 1 else g[f'{key}_ysub']
            d = [float(np.abs(y[:, :4, ::sub] - ref[:, :4]).max()), float(np.abs(y[:, 4:, ::sub] - ref[:, 4:]).max())]
            if sub == 1:
                d.append(max(float(np.abs(to_nchw(f) - g[f'{key}_feat{i}']).max()) for i, f in enumerate(feats)))
            bound = 3 * g[f'{key}_dbf16']
            print(f'bf16 yolov5n {key} fused={fuse}: ' + '  '.join(f'{q} {v:.3e} (bound {b:.3e})' for q, v, b in zip(YR.BF16_QUANTITIES, d, bound)))
            for q, v, b in zip(YR.BF16_QUANTITIES, d, bound):
                assert v <= b, (key, fuse, q, v, b)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')])
def test_captured_forward_equals_eager_and_replays_no_aten_op(dt):
    """forward + decode captured into one graph: bit-equal to the eager call; the fused model takes the same launches as the unfused one; uint8 input too"""
    m = build_model(dt)
    x = seeded_images(2, 160, 224, seed=YR.IMG_SEED).to(DEV)
    xu = (x * 255).round().to(torch.uint8)

    def launches(model, inp):
        names = []
        orig = ops._launch
        with torch.no_grad():
            model(inp)
            ops._launch = lambda name, *a, **k: (names.append(name), orig(name, *a, **k))[1]
            try:
                y, _ = model(inp)
            finally:
                ops._launch = orig
        return y, names
    for inp in (x, xu):
        y0, n0 = launches(m, inp)
        static = inp.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph):
            yg, _ = m(static)
        static.copy_(inp)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, y0)
    assert n0[0] == 'space_to_depth2_fwd' and 'conv_pack' not in n0
    y1, n1 = launches(m.fuse(), xu)
    assert n1 == n0
    if dt == F32:
        np.testing.assert_allclose(y1.cpu().numpy(), y0.cpu().numpy(), atol=2e-4, rtol=0)


@pytest.mark.gpu
def test_augment_runs_and_equals_its_eager_form():
    """model(x, augment=True): the three passes merged into one y equal the composition of the model's own plain forwards at the kernel-resampled inputs
    (_descale_pred + _clip_augmented restated in test_tta._compose: boxes within 1e-3 px - torch divides by the scale as a reciprocal multiply -, scores
    identical); the captured call equals the eager one bit for bit."""
    from test_tta import _compose, _scale_args
    m = build_model()
    x = seeded_images(1, 160, 224, seed=YR.IMG_SEED).to(DEV)
    with torch.no_grad():
        y0, _ = m(x, augment=True)
        xs = [x, ops.scale_img(x, *_scale_args(160, 224, 0.83, 32), True, F32), ops.scale_img(x, *_scale_args(160, 224, 0.67, 32), False, F32)]
        y_own = _compose([m(xi)[0].cpu() for xi in xs], x.shape, 3)
    from mgdt_yolo_amd.nn.tasks import tta_geometry
    assert y0.shape == y_own.shape == (1, 84, tta_geometry(160, 224, [8, 16, 32])['anchors'])
    assert (y0.cpu()[:, :4] - y_own[:, :4]).abs().max().item() < 1e-3 and torch.equal(y0.cpu()[:, 4:], y_own[:, 4:])
    static = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        yg, _ = m(static, augment=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y0)


@pytest.mark.gpu
def test_predictor_and_autobackend_take_the_graph_without_special_cases():
    """DetectionPredictor (AutoBackend(fuse=True) inside): BGR uint8 images -> letter-box on the device -> uint8 batch into the stem -> NMS -> boxes in the
    original image's coordinates, against the same steps done by hand: the oracle's letter-box, the model's own fused fp32 forward, the oracle's NMS and
    scale_boxes.  half=True selects the bf16 route."""
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    from mgdt_yolo_amd.yolo.v8.detect import DetectionPredictor
    from oracle import metrics as OM, nms as ON
    mk = lambda: seed_state_dict_(DetectionModel('yolov5n.yaml', verbose=False), 0)
    r = np.random.default_rng(3)
    imgs = [r.integers(0, 256, (120, 200, 3), dtype=np.uint8) for _ in range(2)]
    pr = DetectionPredictor(dict(imgsz=160, conf=0.2, iou=0.6))
    pr.setup_model(mk())
    assert pr.model.fp16 is False and pr.model.stride == 32 and pr.model.model.is_fused()
    res = pr(imgs)
    lb = np.stack([OM.letterbox(im, (160, 160), auto=True, stride=32) for im in imgs])
    with torch.no_grad():
        y, _ = mk().to(DEV).eval().fuse()(torch.from_numpy(lb).to(DEV))
    rows = ON.non_max_suppression(y.cpu().numpy(), conf_thres=0.2, iou_thres=0.6)
    for i in range(2):
        ref = rows[i].copy()
        ref[:, :4] = OM.scale_boxes(lb.shape[2:], ref[:, :4], imgs[i].shape)
        got = res[i].cpu().numpy()
        assert got.shape == ref.shape and got.shape[0] > 0
        np.testing.assert_allclose(got[:, :4], ref[:, :4], atol=2e-3)
        np.testing.assert_allclose(got[:, 4], ref[:, 4], atol=1e-4)
        assert np.array_equal(got[:, 5], ref[:, 5])
    pr16 = DetectionPredictor(dict(imgsz=160, conf=0.2, iou=0.6, half=True))
    pr16.setup_model(mk())
    assert pr16.model.fp16 and pr16.model.model.compute_dtype == BF16
    assert len(pr16(imgs)) == 2


@pytest.mark.gpu
def test_quantize_fp8_leaves_c3_and_the_stem_on_bf16():
    m = build_model(BF16)
    x = seeded_images(2, 160, 224, seed=YR.IMG_SEED).to(DEV)
    with torch.no_grad():
        y0, _ = m(x)
        table = m.quantize_fp8(x)
        y1, _ = m(x)
    from mgdt_yolo_amd.nn.modules import C3
    c3 = [f'model.{l.i}.' for l in m.model if isinstance(l, C3)]
    assert len(c3) == 8 and table and not any(k.startswith(tuple(c3)) or k.startswith('model.0') for k in table)
    assert any(k.startswith('model.1') for k in table)                                # the other convolutions did switch
    assert not any(mod.__dict__.get('_q8') for l in m.model if isinstance(l, C3) for mod in l.modules())
    assert (y1 - y0).abs().max().item() > 0
    m.dequantize_fp8()
    with torch.no_grad():
        assert torch.equal(m(x)[0], y0)


# ------------------------------------------------------------------------------------------------ training
def _hip_train_step(amp, x, lab, nc, seed):
    from mgdt_yolo_amd.yolo.utils.loss import loss_and_head_grads, v8DetectionLoss
    m = build_model(nc=nc, seed=seed).train()
    if amp:
        m.set_compute_dtype(BF16)
    feats = m._predict_once(x.to(DEV).to(BF16 if amp else F32))
    total, items, hg = loss_and_head_grads(v8DetectionLoss(m), feats, lab)
    m.backward(hg)
    grads = {k: p.grad.detach().float().cpu() for k, p in m.named_parameters() if p.grad is not None}
    bufs = dict(m.named_buffers())
    running = {k[:-len('.running_mean')]: (b.detach().cpu().numpy(), bufs[k[:-len('running_mean')] + 'running_var'].detach().cpu().numpy())
               for k, b in bufs.items() if k.endswith('running_mean')}
    return total, items, [to_nchw(f.float()) for f in feats], grads, running


@pytest.mark.gpu
def test_training_step_matches_the_reference_training_fixture(golden):
    """The fp32 train-mode forward, loss and reverse pass against the reference's own `model.train()(batch); loss.backward()` on the CPU
    (train_yolov5_n.npz), with the bounds of test_hip_parity.test_training_step_matches_the_reference_training_fixture."""
    from test_oracle_golden import check_train_fixture
    c = GI.TRAIN_CASE
    x, lab = GI.train_inputs()
    total, items, feats, grads, running = _hip_train_step(False, x, lab, c['nc'], c['weight_seed'])
    assert tuple(grads['model.0.conv.weight'].shape) == (16, 3, 6, 6)
    worst = check_train_fixture(golden('train_yolov5_n'), total.item(), items.cpu().numpy(), feats, grads, running,
                                dict(feat=2e-4, loss=2e-5, grad=2e-3, grad_abs=1e-2, run=1e-5))
    print('fp32: worst gradient error in units of the tensor rms', worst)


# stated bounds of the bf16 training step vs the reference's fp32 CPU step = 2 x the error measured on the MI355X (see the test's docstring)
BF16_TRAIN_BOUNDS = dict(loss=5.3e-3, feat=0.23, cos=0.976, tensor_cos=0.70, run=2.4e-2)


def _bf16_train_figures(golden):
    g = golden('train_yolov5_n')
    c = GI.TRAIN_CASE
    x, lab = GI.train_inputs()
    total, items, feats, grads, running = _hip_train_step(True, x, lab, c['nc'], c['weight_seed'])
    ferr = max(float(np.abs(f - g[f'feat{i}']).max()) for i, f in enumerate(feats))
    got, ref, per = [], [], []
    for k in str(g['grad_names']).split('\n'):
        a, _ = GI.grad_sample(grads[k])
        b = g['g/' + k].astype(np.float64)
        got.append(a.astype(np.float64)); ref.append(b)
        per.append((float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30)), float(np.linalg.norm(b)), k))
    a, b = np.concatenate(got), np.concatenate(ref)
    cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
    heavy = sorted(p for p in per if p[1] > 1e-3 * np.linalg.norm(b))
    rel = lambda a, b: float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
    rerr, rwhere = max((max(rel(mu, g[f'bn/{p}.running_mean']), rel(var, g[f'bn/{p}.running_var'])), p) for p, (mu, var) in running.items())
    lerr = abs(total.item() - float(g['loss'])) / float(g['loss'])
    print(f'bf16 yolov5n vs reference: loss {total.item():.4f} vs {float(g["loss"]):.4f} (rel {lerr:.3e}), head maps max err {ferr:.4f}, gradient cosine {cos:.5f}, '
          f'lowest per-tensor {heavy[:3]}, running stats max rel err {rerr:.2e} at {rwhere}')
    return dict(loss=lerr, feat=ferr, cos=cos, tensor_cos=heavy[0][0], run=rerr)


@pytest.mark.gpu
def test_bf16_training_step_vs_the_reference_training_fixture(golden):
    """The bf16 (amp) training step against the reference's fp32 CPU step (train_yolov5_n.npz).  Stated bounds = 2 x what was measured on the MI355X (B = 4 at
    96^2: batch statistics over 3x3 .. 12x12 maps), per quantity, as test_hip_parity.BF16_TRAIN_BOUNDS does for the v8 graphs: loss within 0.53 % (measured
    0.263 %: 69.5287 vs 69.7123), head maps within 0.23 absolute (0.1132), cosine of the gradient samples of all 219 tensors with the reference's > 0.976 (0.98813;
    the bound doubles the distance from 1), every tensor that carries a measurable share of the gradient > 0.70 (lowest: model.2.m.0.cv1.bn.weight at 0.854, then
    0.861, 0.881), running statistics within 2.4 % of max(1, |value|) (1.18 % at model.9.cv2.bn).  The figures repeat bit for bit from run to run."""
    f = _bf16_train_figures(golden)
    b = BF16_TRAIN_BOUNDS
    assert f['loss'] < b['loss'] and f['feat'] < b['feat'] and f['cos'] > b['cos'] and f['tensor_cos'] > b['tensor_cos'] and f['run'] < b['run'], (f, b)


@pytest.mark.gpu
def test_loss_backward_and_trainer_step_give_bit_equal_gradients():
    """`loss, items = model(batch); loss.backward()` (the reference trainer's call sequence) and DetectionTrainer.step on a copy of the model fill the same
    gradients bit for bit - the stem's (16, 3, 6, 6) gradient included, which the trainer's reverse pass produces from deferred final sums."""
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    c = GI.TRAIN_CASE
    x, lab = GI.train_inputs()
    m = build_model(nc=c['nc']).train()
    loss, items = m(dict(img=x.to(DEV), **lab))
    assert loss.requires_grad and items.shape == (3,)
    loss.backward()
    m2 = build_model(nc=c['nc']).train()
    tr = DetectionTrainer(m2, lr0=0.0)
    total, items2 = tr.step(dict(img=x.to(DEV), **lab))
    assert torch.equal(loss.detach(), total) and torch.equal(items, items2)
    n = 0
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        if p.grad is None:
            continue
        assert torch.equal(p.grad, p2.grad), k
        n += 1
    assert n == 219


@pytest.mark.gpu
@pytest.mark.parametrize('amp', [False, True], ids=['f32', 'bf16'])
def test_two_captured_training_steps_equal_two_eager_steps(amp):
    """DetectionTrainer(graph=True): the first step is eager, the next two are one captured graph replayed twice; losses, weights and EMA equal the eager
    trainer's bit for bit (uint8 batches, so the stem's space-to-depth launch divides by 255 inside the graph; its panel is refreshed by the captured
    re-pack like every other one)."""
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    from mgdt_yolo_amd.seeding import seeded_labels
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    nc, B, S = 4, 4, 96
    batches = []
    for r in range(3):
        lab = seeded_labels(B, nc, seed=10 + r, max_boxes=6, min_boxes=2)
        lab['bboxes'][:, 2:] = lab['bboxes'][:, 2:] * 0.5 + 0.1
        batches.append(dict(img=(seeded_images(B, S, S, seed=20 + r) * 255).to(torch.uint8), **lab))
    res = {}
    for graph in (False, True):
        m = seed_state_dict_(DetectionModel(get_config('yolov5', 'n', nc), verbose=False), 0).to(DEV)
        tr = DetectionTrainer(m, lr0=0.01, amp=amp, graph=graph, batch_size=64, nb=10, epochs=3)
        losses = [tr.step(b)[0].item() for b in batches]
        res[graph] = (losses, tr.state.data.clone(), tr.state.ema.clone())
        if graph:
            assert len(tr._graphs) == 1
            panels = next(iter(tr._graphs.values()))[2]
            assert any(isinstance(o, ops.PackedStem6) for o in panels), 'the stem panel is part of the live panel set the captured re-pack refreshes'
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    assert torch.equal(res[False][1], res[True][1]) and torch.equal(res[False][2], res[True][2])
    assert len(set(res[True][0])) == 3


# ================================================================================================ the one-launch C3 route (mode CSP_C3 of mgdt_csp_block_fwd)
from c3_ref import ref_c3_block, ref_c3_front  # noqa: E402
from knobs import forced_tile as _forced_tile  # noqa: E402

# (id, wd, n, shortcut, B, H, W, forced tile or None, cout, channel offset of the input view, BN form)
C3_KERNEL_CASES = [
    ('wd16-n1-5x7-whole-map', 16, 1, True, 1, 5, 7, None, 32, 0, False),
    ('wd16-n2-8x12-tile2x3-slice8-B3', 16, 2, False, 3, 8, 12, (2, 3), 64, 8, False),
    ('wd32-n1-8x12-tile2x2-cout20-bn', 32, 1, False, 1, 8, 12, (2, 2), 20, 0, True),
    ('wd32-n2-16x24-tile8x24', 32, 2, True, 1, 16, 24, (8, 24), 128, 0, False),
    ('wd64-n1-8x8-tile2x2', 64, 1, True, 1, 8, 8, (2, 2), 128, 0, False),
    ('wd64-n2-6x10-cout256-B3', 64, 2, True, 3, 6, 10, None, 256, 0, True),
]


def _c3_kernel_inputs(cid, wd, n, B, H, W, cout, bn, wrep=BF16):
    from kernel_ref import ConvP, _gen, _rand
    gen = _gen('c3', cid)
    ab = _rand(gen, B, 2 * wd, H, W, dt=BF16)
    mids = [ConvP(gen, wd, wd, 1 if j % 2 == 0 else 3, bn=bn, wrep=wrep) for j in range(2 * n)]
    back = ConvP(gen, cout, 2 * wd, 1, bn=bn, wrep=wrep)
    return ab, mids, back, gen


def test_c3_kernel_host_side_geometry_and_refusals():
    """mgdt_csp_block_supported / _tiles for mode 2, without a GPU: the covered classes, the tile each case forces or picks (divides the map, halo n, LDS
    3 region maps + b), and the refusals (odd H without a tiling, wd 128, wd 8, n 3, fp32, cin != 2 wd, cout % 4)."""
    import ctypes as C
    lib = _lib.lib()
    for cid, wd, n, sc, B, H, W, tile, cout, xoff, bn in C3_KERNEL_CASES:
        assert lib.mgdt_csp_block_supported(2, 2 * wd, cout, wd, n, H, W, _lib.BF16), cid
        g = (C.c_int * 8)()
        with _forced_tile(tile):
            slots = lib.mgdt_csp_block_tiles(2, B, 2 * wd, cout, wd, n, H, W, g)
        th, tw = g[0], g[1]
        assert slots == (H // th) * (W // tw) > 0 and H % th == 0 and W % tw == 0 and (tile is None or (th, tw) == tile), (cid, list(g))
        rpa, tpa = -(-(th + 2 * n) * (tw + 2 * n) // 16) * 16, -(-th * tw // 16) * 16
        assert (g[2], g[3]) == (th + 2 * n, tw + 2 * n) and g[4] == (3 * rpa + tpa) * wd * 2 <= 80 * 1024 and g[5] == B * slots and (g[6], g[7]) == (W // tw, H // th)
    facts = {(c[1], c[2]) for c in C3_KERNEL_CASES}
    assert facts == {(wd, n) for wd in (16, 32, 64) for n in (1, 2)}
    assert any(c[7] is None and c[5] % 2 for c in C3_KERNEL_CASES) and any(c[8] % 16 for c in C3_KERNEL_CASES) and any(c[9] for c in C3_KERNEL_CASES)
    for args in [(256, 64, 128, 1, 8, 8), (16, 32, 8, 1, 8, 8), (64, 64, 32, 3, 8, 8), (48, 64, 32, 1, 8, 8), (64, 30, 32, 1, 8, 8), (64, 64, 32, 0, 8, 8)]:
        assert not lib.mgdt_csp_block_supported(2, *args, _lib.BF16), args
    assert not lib.mgdt_csp_block_supported(2, 64, 64, 32, 1, 8, 8, _lib.F32) and not lib.mgdt_csp_block_supported(3, 64, 64, 32, 1, 8, 8, _lib.BF16)
    assert lib.mgdt_csp_block_supported(2, 64, 64, 32, 1, 37, 8, _lib.BF16) and lib.mgdt_csp_block_tiles(2, 1, 64, 64, 32, 1, 37, 8, None) == 0      # no tiling of 37 rows
    assert lib.mgdt_csp_block_fwd(2, None, None, None, None, None, 1, 1, None, None, 32, 1, None, None, 1, None) == -4


def test_restatement_soundness_c3_block():
    """c3_ref without its rounding points, in float64, equals the chain of plain convolutions C3 is (cv3(cat(m(cv1(x)), cv2(x))), block.py:443-447)."""
    from kernel_ref import ConvP, _gen, _rand, _silu
    gen = _gen('c3-sound')
    for wd, n, sc, cout in ((16, 1, True, 32), (32, 2, False, 20), (16, 2, True, 64)):
        x = _rand(gen, 2, 24, 7, 9, dt=F32)
        cv1, cv2 = ConvP(gen, wd, 24, 1, bn=True, dt=F32, wrep=F32), ConvP(gen, wd, 24, 1, bn=True, dt=F32, wrep=F32)
        mids = [ConvP(gen, wd, wd, 1 if j % 2 == 0 else 3, bn=bool(j % 2), dt=F32, wrep=F32) for j in range(2 * n)]
        back = ConvP(gen, cout, 2 * wd, 1, dt=F32, wrep=F32)
        f = lambda cp, t: _silu(F.conv2d(t, cp.wq, cp.bq, 1, cp.k // 2))
        a = f(cv1, x)
        for j in range(n):
            h = f(mids[2 * j + 1], f(mids[2 * j], a))
            a = a + h if sc else h
        ref = f(back, torch.cat([a, f(cv2, x)], 1))
        got = ref_c3_block(ref_c3_front(x, cv1, cv2, rnd=False), mids, sc, back, rnd=False)
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize('cid,wd,n,sc,B,H,W,tile,cout,xoff,bn', [pytest.param(*c, id=c[0]) for c in C3_KERNEL_CASES])
def test_c3_block_kernel(cid, wd, n, sc, B, H, W, tile, cout, xoff, bn):
    """y of mode CSP_C3 against c3_ref.ref_c3_block (rounding points stated there) under kernel_ref._check: whole-map and multi-tile grids, tiles smaller
    than the halo ring, image borders, a channel-slice input view, cout % 16 != 0 and 256, BN and fused-bias panels, shortcut on and off."""
    from kernel_ref import _check, _nhwc
    ab, mids, back, gen = _c3_kernel_inputs(cid, wd, n, B, H, W, cout, bn)
    xv, _ = _nhwc(ab, BF16, xoff, xoff, gen)
    with _forced_tile(tile):
        assert ops.csp_block_supported(ops.CSP_C3, xv, cout, wd, n, BF16)
        y, part, slots, tiles = ops.csp_block(ops.CSP_C3, xv, None, None, [m.pack() for m in mids], sc, back.pack(), wd, ops.ACT_SILU, cout, False)
        torch.cuda.synchronize()
    assert part is None and y.dtype == BF16 and tuple(y.shape) == (B, cout, H, W)
    if tile:
        assert tuple(tiles) == (W // tile[1], H // tile[0])
    _check(y, ref_c3_block(ab, mids, sc, back), BF16, cid)


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['odd-H-no-tiling', 'wd128', 'n3', 'fp32', 'relu', 'hooked'])
def test_c3_module_refusals_take_the_composed_route_silently(what):
    """Outside the kernel's cover the module composes, with the same result as with the fused route switched off."""
    from mgdt_yolo_amd.nn.modules import C3
    c1, c2, n, H, dt = {'odd-H-no-tiling': (32, 32, 1, 37, BF16), 'wd128': (64, 256, 1, 8, BF16), 'n3': (32, 32, 3, 8, BF16), 'fp32': (32, 32, 1, 8, F32),
                        'relu': (32, 32, 1, 8, BF16), 'hooked': (32, 32, 1, 8, BF16)}[what]
    m = make_module('C3', (c1, c2, n, True))
    m.apply(lambda s: setattr(s, '_cdtype', dt) if hasattr(s, 'out_dtype') else None)
    if what == 'relu':
        m.m[0].cv2.act = torch.nn.ReLU()
    if what == 'hooked':
        m.m[0].register_forward_hook(lambda *a: None)
    x = YR.case_input('c3-refuse-' + what, (2, c1, H, 8)).to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
    old = ops.C3_FUSED_CLASSES
    names = []
    orig = ops._launch
    try:
        ops.C3_FUSED_CLASSES = None
        probe = ops.new_act(2, 2 * m.c, H, 8, dt, DEV)
        if what in ('odd-H-no-tiling', 'wd128', 'n3', 'fp32'):
            assert not ops.csp_block_supported(ops.CSP_C3, probe, c2, m.c, n, dt)
        ops._launch = lambda name, *a, **k: (names.append(name), orig(name, *a, **k))[1]
        with torch.no_grad():
            y = m(x)
        ops._launch = orig
        ops.C3_FUSED_CLASSES = ()
        with torch.no_grad():
            y0 = m(x)
    finally:
        ops._launch, ops.C3_FUSED_CLASSES = orig, old
    assert 'csp_block_fwd' not in names and torch.equal(y, y0)


@pytest.mark.gpu
@pytest.mark.parametrize('args,shape', [((32, 32, 1, True), (2, 32, 8, 12)), ((64, 64, 2, True), (2, 64, 8, 12)), ((128, 64, 1, False), (1, 128, 10, 6)),
                                        ((128, 128, 2, False), (3, 128, 6, 10))], ids=['wd16-n1', 'wd32-n2', 'wd32-n1-nosc', 'wd64-n2-nosc'])
@pytest.mark.parametrize('fuse', [False, True], ids=['bn', 'fused-bias'])
def test_c3_module_fused_route_against_composed_route(args, shape, fuse):
    """The same bf16 module on both routes: two launches (merged [cv1 | cv2], csp_block_fwd) against 3 + 2n, under kernel_ref._check with the composed
    output as the reference (both round the same maps to bf16; they differ in accumulation order and in one rounding of the merged panel's shared
    launch - none).  ops.FUSED_CSP_BLOCK = False and an empty ops.C3_FUSED_CLASSES both switch the route off."""
    from kernel_ref import _check
    from mgdt_yolo_amd.nn.modules import Conv
    from mgdt_yolo_amd.yolo.utils.torch_utils import fuse_conv_and_bn
    m = make_module('C3', args)
    m.apply(lambda s: setattr(s, '_cdtype', BF16) if hasattr(s, 'out_dtype') else None)
    if fuse:
        for sub in m.modules():
            if isinstance(sub, Conv):
                sub.conv = fuse_conv_and_bn(sub.conv, sub.bn)
                del sub.bn
    x = YR.case_input('c3-routes', shape).to(DEV).to(BF16).contiguous(memory_format=torch.channels_last)
    old = ops.C3_FUSED_CLASSES

    def run():
        names = []
        orig = ops._launch
        ops._launch = lambda name, *a, **k: (names.append(name), orig(name, *a, **k))[1]
        try:
            with torch.no_grad():
                return m(x), [k for k in names if k != 'conv_pack']
        finally:
            ops._launch = orig
    try:
        ops.C3_FUSED_CLASSES = None
        y1, n1 = run()
        ops.FUSED_CSP_BLOCK = False
        y2, n2 = run()
        ops.FUSED_CSP_BLOCK = True
        ops.C3_FUSED_CLASSES = ()
        y0, n0 = run()
    finally:
        ops.C3_FUSED_CLASSES, ops.FUSED_CSP_BLOCK = old, True
    assert n1 == ['conv2d_fwd', 'csp_block_fwd'] and n0 == n2 == ['conv2d_fwd'] * (3 + 2 * args[2]) and torch.equal(y0, y2)
    _check(y1, y0.double().cpu(), BF16, f'C3 {args} fused vs composed')
