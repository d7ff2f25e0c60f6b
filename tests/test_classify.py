"""Image classification: the Classify head kernels (csrc/classify.hip), ClassificationModel, v8ClassificationLoss, ClassifyMetrics, the predictor
and the validator against float64 restatements (tests/cls_ref.py) and the reference's own outputs (tests/golden/cls_NN.npz, gen_cls.py)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import cls_ref as CR
from mgdt_yolo_amd import _lib, ops
from mgdt_yolo_amd.models import get_config
from mgdt_yolo_amd.seeding import seeded_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
FEAT_ATOL, FEAT_RTOL = 1e-3, 1e-4          # the project's feature-map tolerance
U32 = 2.0 ** -24                           # unit roundoff of fp32 (round to nearest)
U16 = 2.0 ** -9                            # unit roundoff of bf16


@functools.lru_cache(maxsize=None)
def fixture():
    return CR.load_fixture()


def build_model(nc, scale='n', dtype=torch.float32, device=DEV):
    from mgdt_yolo_amd.nn.tasks import ClassificationModel
    m = CR.seed_cls_(ClassificationModel(get_config('yolov8-cls', scale, nc), verbose=False), CR.WEIGHT_SEED)
    if device is not None:
        m = m.to(device)
        m.set_compute_dtype(dtype)
    return m.eval()


# ================================================================================================================ host tests (no GPU)
def test_entry_points_are_declared_bound_and_refuse_bad_arguments():
    hdr = open(os.path.join(ROOT, 'include', 'mgdt.h')).read()
    lib = _lib.lib()
    names = ('mgdt_classify_pool_fwd', 'mgdt_classify_linear_fwd', 'mgdt_cls_softmax_fwd', 'mgdt_cls_loss_fwd', 'mgdt_cls_loss_bwd', 'mgdt_cls_topk_fwd')
    for n in names:
        assert n + '(' in hdr and n in _lib.PROTOTYPES and hasattr(lib, n), n
    one = C.c_void_p(16)                                   # never dereferenced: every call below is refused before any launch
    v = _lib.View(16, 1, 2, 2, 256, 1024, 512, 256, 1)
    bad = [
        lib.mgdt_classify_pool_fwd(None, one, one, 1280, 1, 1, 1, one, 0, None),
        lib.mgdt_classify_pool_fwd(C.byref(v), None, one, 1280, 1, 1, 1, one, 0, None),
        lib.mgdt_classify_pool_fwd(C.byref(v), one, one, 1280, 3, 1, 1, one, 0, None),            # k != 1
        lib.mgdt_classify_pool_fwd(C.byref(v), one, one, 1280, 1, 2, 1, one, 0, None),            # groups
        lib.mgdt_classify_pool_fwd(C.byref(v), one, one, 1280, 1, 1, 2, one, 0, None),            # ReLU
        lib.mgdt_classify_pool_fwd(C.byref(v), one, one, 1281, 1, 1, 1, one, 0, None),            # cout % 16
        lib.mgdt_classify_pool_fwd(C.byref(v), one, one, 1280, 1, 1, 1, one, 7, None),            # dtype
        lib.mgdt_classify_pool_fwd(C.byref(_lib.View(16, 1, 2, 2, 36, 144, 72, 36, 1)), one, one, 1280, 1, 1, 1, one, 0, None),   # c1 % 8
        lib.mgdt_classify_pool_fwd(C.byref(_lib.View(16, 1, 2, 2, 256, 1024, 1, 2, 4)), one, one, 1280, 1, 1, 1, one, 0, None),   # NCHW
        lib.mgdt_classify_linear_fwd(None, one, one, 1, 1280, 10, one, None, 0, None),
        lib.mgdt_classify_linear_fwd(one, one, one, 1, 1281, 10, one, None, 0, None),
        lib.mgdt_classify_linear_fwd(one, one, one, 1, 1280, 0, one, None, 0, None),
        lib.mgdt_cls_softmax_fwd(None, 1, 1, one, None),
        lib.mgdt_cls_softmax_fwd(one, 0, 1, one, None),
        lib.mgdt_cls_loss_fwd(one, None, 1, 1, one, one, None),
        lib.mgdt_cls_loss_fwd(one, one, 1, 0, one, one, None),
        lib.mgdt_cls_loss_bwd(one, one, 1, 1, 1.0, None, None),
        lib.mgdt_cls_topk_fwd(one, 1, 0, one, None, None, None),
        lib.mgdt_cls_topk_fwd(one, 1, 3, one, None, one, None),                                   # matrix without targets
    ]
    assert all(s < 0 for s in bad), bad
    assert b'unfused chain' in (lib.mgdt_classify_pool_fwd(C.byref(v), one, one, 1280, 3, 1, 1, one, 0, None), lib.mgdt_last_error())[1]


def test_config_equals_the_reference_yaml():
    ref = json.load(open(os.path.join(CR.GOLDEN, 'cls_yaml.json')))
    for scale in 'nslmx':
        c = get_config('yolov8-cls', scale)
        assert c['scale'] == scale
        for k in ('nc', 'scales', 'backbone', 'head'):
            assert c[k] == ref[k], k
    assert get_config('yolov8-cls', 'n', 7)['nc'] == 7
    from mgdt_yolo_amd.nn.tasks import yaml_model_load
    d = yaml_model_load('yolov8s-cls.yaml')
    assert d['scale'] == 's' and d['head'] == ref['head'] and d['backbone'] == ref['backbone']


@pytest.mark.parametrize('scale', ['n', 's'])
def test_model_structure_equals_the_reference(scale):
    g = fixture()
    m = build_model(10, scale, device=None)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f'yolov8_cls_{scale}_keys']]
    assert [','.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[f'yolov8_cls_{scale}_shapes']]
    assert sum(p.numel() for p in m.parameters()) == int(g[f'yolov8_cls_{scale}_nparams'])
    head = m.model[-1]
    assert isinstance(head.pool, nn.AdaptiveAvgPool2d) and isinstance(head.drop, nn.Dropout) and isinstance(head.linear, nn.Linear)
    assert m.stride.tolist() == [1.0] and m.names == {i: str(i) for i in range(10)}
    # the reference's ClassificationModel never calls initialize_weights (tasks.py:367-381): BatchNorm keeps nn.BatchNorm2d's defaults
    bns = [b for b in m.modules() if isinstance(b, nn.BatchNorm2d)]
    assert bns and {(b.eps, b.momentum) for b in bns} == {(1e-5, 0.1)}


def test_task_guessing_and_model_class():
    from mgdt_yolo_amd.nn import tasks as T
    c = get_config('yolov8-cls', 'n', 3)
    assert T.guess_model_task(c) == 'classify' and T.model_class_of(c) is T.ClassificationModel
    assert T.guess_model_task(build_model(3, device=None)) == 'classify'
    assert T.guess_model_task('yolov8n-cls.yaml') == 'classify' and T.guess_model_task('runs/classify/train/weights/last.pt') == 'classify'
    # every earlier answer is unchanged
    assert T.guess_model_task(get_config('yolov8', 'n')) == 'detect' and T.model_class_of(get_config('yolov8', 'n')) is T.DetectionModel
    assert T.guess_model_task(get_config('yolov8-seg', 'n')) == 'segment' and T.model_class_of(get_config('yolov8-seg', 'n')) is T.SegmentationModel
    assert T.guess_model_task(get_config('yolov8-pose', 'n')) == 'pose' and T.model_class_of(get_config('yolov8-pose', 'n')) is T.PoseModel
    for name, task in (('yolov8n.yaml', 'detect'), ('yolov8n-seg.pt', 'segment'), ('a/segment/x.pt', 'segment'), ('yolov8s-pose.yaml', 'pose'),
                       ('a/pose/x.pt', 'pose'), ('whatever.pt', 'detect')):
        assert T.guess_model_task(name) == task, name


def test_clear_errors_for_what_is_not_built():
    from mgdt_yolo_amd.nn.tasks import ClassificationModel
    m = build_model(3, device=None)
    with pytest.raises(RuntimeError, match='augment=True is not built for ClassificationModel'):
        m(torch.zeros(1, 3, 64, 64), augment=True)
    with pytest.raises(NotImplementedError, match='_from_detection_model is not built'):
        ClassificationModel(model=m, nc=3)
    ClassificationModel.reshape_outputs(m, 5)
    assert m.model[-1].linear.out_features == 5


def test_classify_metrics_match_the_reference():
    from mgdt_yolo_amd.yolo.utils.metrics import ClassifyMetrics
    g, c = fixture(), CR.METRIC_CASE
    pred = torch.from_numpy(g['metric_pred'])
    t = CR.seeded_labels(c['n'], c['nc'], seed=c['seed'])
    met = ClassifyMetrics()
    met.process([t[:10], t[10:]], [pred[:10], pred[10:]])
    assert [met.top1, met.top5] == g['metric_top'].tolist()
    assert met.keys == [str(k) for k in g['metric_keys']] and met.fitness == met.top5
    assert met.results_dict == dict(zip(met.keys + ['fitness'], [met.top1, met.top5, met.top5]))


@pytest.mark.parametrize('shape,want', [((100, 160), (0, 30, 100)), ((160, 100), (30, 0, 100)), ((64, 64), (0, 0, 64)), ((7, 10), (0, 1, 7)),
                                        ((11, 6), (2, 0, 6)), ((5, 8), (0, 1, 5))])
def test_classify_crop_offsets(shape, want):
    """CenterCrop (reference augment.py:880-884): m = min(h, w), top = (h - m) // 2, left = (w - m) // 2 - landscape, portrait, square, odd sizes."""
    from mgdt_yolo_amd.yolo.v8.classify import classify_crop, classify_transforms
    assert classify_crop(shape) == want
    with pytest.raises(TypeError):
        classify_transforms((224, 224))


def test_bad_labels_are_refused_on_the_host():
    """The range check runs before anything touches the device: labels on the host, logits that are never read."""
    lg = torch.zeros(3, 4)
    for fn in (ops.cls_loss_fwd, ops.cls_loss_bwd):
        with pytest.raises(RuntimeError, match='HIP'):
            fn(lg, torch.tensor([0, 1, 2]))                                   # CPU logits: refused first
    for lab in ([0, 4, 1], [-1, 0, 0]):
        with pytest.raises(ValueError, match=r'outside \[0, 4\)'):
            ops._cls_labels(torch.tensor(lab), 3, 4, 'cpu')
    with pytest.raises(RuntimeError, match='int64'):
        ops._cls_labels(torch.tensor([0.0, 1.0, 2.0]), 3, 4, 'cpu')
    with pytest.raises(RuntimeError, match='2 labels for 3 rows'):
        ops._cls_labels(torch.tensor([0, 1]), 3, 4, 'cpu')
    from mgdt_yolo_amd.yolo.v8.classify import ClassificationValidator
    v = ClassificationValidator(device='cpu')
    v.init_metrics(4)
    with pytest.raises(ValueError, match=r'outside \[0, 4\)'):
        v.preprocess({'img': torch.zeros(1, 3, 8, 8), 'cls': torch.tensor([4])})
    with pytest.raises(RuntimeError, match='plots'):
        ClassificationValidator(device='cpu', args={'plots': True})
    with pytest.raises(RuntimeError, match='plots'):
        v.plot_val_samples(None, 0)


# ================================================================================================================ head kernels vs float64
def head_module(case, dtype, seed=0):
    """(Classify module on the GPU in eval mode, x NHWC in `dtype`, the CPU tensors it was filled from)"""
    from mgdt_yolo_amd.nn.modules import Classify
    b, c1, h, w, nc = case
    x, wc, bn, wl, bl = CR.head_inputs(*case, seed=seed)
    m = Classify(c1, nc)
    with torch.no_grad():
        m.conv.conv.weight.copy_(wc.reshape(1280, c1, 1, 1))
        for p, v in zip((m.conv.bn.weight, m.conv.bn.bias, m.conv.bn.running_mean, m.conv.bn.running_var), bn):
            p.copy_(v)
        m.linear.weight.copy_(wl)
        m.linear.bias.copy_(bl)
    m = m.to(DEV).eval()
    m._cdtype = m.conv._cdtype = dtype
    xd = x.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
    return m, xd, (x, wc, bn, wl, bl)


def head_reference(m, x, wc, bn, wl, bl, dtype):
    """float64 restatement on the operands the kernel sees (bf16: input, folded weights and linear weights rounded to bf16) and the error bounds.

    bf16 bound.  A product of two bf16 values is exact in fp32 (8 + 8 significand bits), so the only error of the GEMM is fp32 accumulation:
    |err(z)| <= (K + 8) u sum_k |x_k w_k| with u = 2^-24, whatever the order (the + 8 covers the shift addition and the matrix core's internal
    order).  SiLU has slope <= 1.1 and the hardware sigmoid is good to a few ulp: |err(silu)| <= 1.1 |err(z)| + 8 u |z|.  The mean over h*w
    pixels adds (hw + 1) u |pooled|-ish; bounded by (hw + 1) u mean|silu|.  pooled bound = the largest such sum over (image, channel).
    logits = pooled @ wl^T in fp32 (fma chain + lane tree): |err| <= sum_k |wl_k| err(pooled) + (1280 + 8) u sum_k |pooled_k wl_k|."""
    eps = m.conv.bn.eps
    r = CR.bf16r if dtype == torch.bfloat16 else (lambda t: t)
    g, b_, mu, var = bn
    s32 = g / torch.sqrt(var + eps)                                            # the fold is done in fp32 (fuse_conv_and_bn), then rounded
    wf = r(wc * s32[:, None])
    shift = (b_ - g * mu / torch.sqrt(var + eps)).double()
    xr, wlr = r(x), r(wl)
    pooled, logits, probs = CR.head64(xr, wf.double(), shift, wlr, bl)
    B, c1, h, w = x.shape
    xa = xr.double().abs().reshape(B, c1, h * w)
    sabs = torch.einsum('bkp,nk->bnp', xa, wf.double().abs())
    z = torch.einsum('bkp,nk->bnp', xr.double().reshape(B, c1, h * w), wf.double()) + shift[None, :, None]
    ez = (c1 + 8) * U32 * sabs
    es = 1.1 * ez + 8 * U32 * z.abs()
    ep = es.mean(2) + (h * w + 1) * U32 * (z * torch.sigmoid(z)).abs().mean(2)
    el = ep @ wlr.double().abs().t() + (1280 + 8) * U32 * (pooled.abs() @ wlr.double().abs().t())
    return pooled, logits, probs, ep, el


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', CR.HEAD_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_head_kernels_match_float64(case, dtype):
    """mgdt_classify_pool_fwd and mgdt_classify_linear_fwd against the float64 restatement: fp32 within the feature-map tolerance (atol 1e-3,
    rtol 1e-4); bf16 against the restatement on bf16-rounded input and weights within the bound derived in `head_reference` (fp32 accumulation of K
    exact bf16 products).  The folded shift is about 1, so one unmasked padding row of the last 16-pixel tile would move `pooled` by
    SiLU(1) / (h*w) ~ 0.7 / (h*w) >= 1.8e-3 (400 pixels), far beyond either bound for the shapes whose h*w is no multiple of 16."""
    m, xd, cpu = head_module(case, dtype)
    pooled64, logits64, probs64, ep, el = head_reference(m, *cpu, dtype)
    with torch.no_grad():
        pk = m._pool_panel(dtype)
        pooled = ops.classify_pool(xd, pk)
        wl = m.linear.weight.detach().to(dtype).contiguous()
        logits, probs = ops.classify_linear(pooled, wl, m.linear.bias.detach(), softmax=True)
        again = ops.classify_pool(xd, pk)
    assert torch.equal(pooled, again), 'the reduction order is fixed: two launches must agree bit for bit'
    pooled, logits, probs = pooled.cpu().double(), logits.cpu().double(), probs.cpu().double()
    dp, dl = (pooled - pooled64).abs(), (logits - logits64).abs()
    print(f'{case} {dtype}: pooled err {float(dp.max()):.3e} (bound min {float(ep.min()):.3e} max {float(ep.max()):.3e}), '
          f'logits err {float(dl.max()):.3e} (bound max {float(el.max()):.3e})')
    if dtype == torch.float32:
        np.testing.assert_allclose(pooled.numpy(), pooled64.numpy(), atol=FEAT_ATOL, rtol=FEAT_RTOL)
        np.testing.assert_allclose(logits.numpy(), logits64.numpy(), atol=FEAT_ATOL, rtol=FEAT_RTOL)
    else:
        assert bool((dp <= ep).all()), float((dp / ep).max())
        assert bool((dl <= el).all()), float((dl / el).max())
    # the softmax of the logits the kernel produced
    np.testing.assert_allclose(probs.numpy(), torch.softmax(logits, 1).numpy(), atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(probs.sum(1).numpy(), 1.0, atol=1e-6)


@pytest.mark.gpu
def test_softmax_of_wide_logits_is_finite_and_normalised():
    r = np.random.default_rng(5)
    lg = torch.from_numpy(r.uniform(-100.0, 100.0, (7, 1000)).astype(np.float32))
    lg[0, 3], lg[0, 4] = 100.0, -100.0
    p = ops.cls_softmax(lg.to(DEV)).cpu()
    assert bool(torch.isfinite(p).all())
    np.testing.assert_allclose(p.double().sum(1).numpy(), 1.0, atol=1e-6)
    np.testing.assert_allclose(p.double().numpy(), torch.softmax(lg.double(), 1).numpy(), atol=1e-6, rtol=2e-5)
    one = ops.cls_softmax(torch.tensor([[37.5], [-80.0]], device=DEV)).cpu()
    assert one.tolist() == [[1.0], [1.0]]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', [(2, 256, 7, 7, 10), (1, 512, 3, 5, 1000), (3, 256, 1, 1, 2)], ids=lambda c: 'x'.join(map(str, c)))
def test_fused_head_equals_the_unfused_chain_and_survives_fuse(case, dtype, monkeypatch):
    """Module level: the two-launch eval head against Conv.forward -> adaptive_avgpool -> linear as a 1x1 convolution -> softmax kernel.  fp32: the
    feature-map tolerance on the probabilities.  bf16: both routes against the float64 restatement - the fused one within the softmax image of the
    derived logits bound (|dp| <= 2 |dlogit|), the unfused one with the three bf16 stores it adds (conv map, pooled map, logits: relative 2^-9 each,
    carried through the linear layer).  After the head conv is fused the way BaseModel.fuse() does it, the fused route is bit-equal."""
    from mgdt_yolo_amd.yolo.utils.torch_utils import fuse_conv_and_bn
    m, xd, cpu = head_module(case, dtype)
    pooled64, logits64, probs64, ep, el = head_reference(m, *cpu, dtype)
    launches = []
    orig = ops._launch
    monkeypatch.setattr(ops, '_launch', lambda name, *a, **k: (launches.append(name), orig(name, *a, **k))[1])
    with torch.no_grad():
        fused = m(xd)
        assert launches == ['classify_pool_fwd', 'classify_linear_fwd'], launches
        monkeypatch.setattr(ops, 'FUSED_CLS_HEAD', False)
        del launches[:]
        unfused = m(xd)
        assert 'classify_pool_fwd' not in launches and 'adaptive_avgpool_fwd' in launches and 'cls_softmax_fwd' in launches, launches
        monkeypatch.setattr(ops, 'FUSED_CLS_HEAD', True)
    assert fused.dtype == torch.float32 and tuple(fused.shape) == (case[0], case[4]) and unfused.dtype == torch.float32
    f, u = fused.cpu().double(), unfused.cpu().double()
    if dtype == torch.float32:
        np.testing.assert_allclose(f.numpy(), probs64.numpy(), atol=1e-4, rtol=FEAT_RTOL)
        np.testing.assert_allclose(u.numpy(), f.numpy(), atol=FEAT_ATOL, rtol=FEAT_RTOL)
    else:
        wla = CR.bf16r(cpu[3]).double().abs()
        bf = 2.0 * el.max(1).values[:, None]
        assert bool(((f - probs64).abs() <= bf + 1e-6).all())
        ep_u = ep + U16 * 1.05 * pooled64.abs().max() * 2                         # conv map and pooled map stored as bf16
        el_u = ep_u @ wla.t() + (1280 + 8) * U32 * (pooled64.abs() @ wla.t()) + U16 * logits64.abs() + 8 * U16 * U16
        bu = 2.0 * el_u.max(1).values[:, None]
        print(f'{case}: fused err {float((f - probs64).abs().max()):.3e} (bound {float(bf.max()):.3e}), unfused err {float((u - probs64).abs().max()):.3e} '
              f'(bound {float(bu.max()):.3e})')
        assert bool(((u - probs64).abs() <= bu + 1e-6).all())
        assert bool(((u - f).abs() <= bu + bf + 2e-6).all())
    # fuse() of the head conv (nn/tasks.py BaseModel.fuse)
    m.conv.conv = fuse_conv_and_bn(m.conv.conv, m.conv.bn)
    delattr(m.conv, 'bn')
    m.conv.forward = m.conv.forward_fuse
    m.conv.__dict__.pop('_pk', None)
    del launches[:]
    with torch.no_grad():
        after = m(xd)
    assert launches == ['classify_pool_fwd', 'classify_linear_fwd'], launches
    assert torch.equal(after, fused)


# ================================================================================================================ model vs the reference
@pytest.mark.gpu
@pytest.mark.parametrize('tag', list(CR.CASES))
def test_cls_model_fp32_matches_reference(tag):
    """ClassificationModel (fp32) against the reference's eval probabilities and train-mode logits.  Probabilities: max(1e-4, 4 x the fixture's
    fp32-vs-fp64 difference) - 1e-4 is the project's confidence contract; our fp32 result and the reference's are two fp32 evaluations in different
    summation orders, each about one fp32-vs-fp64 difference from the exact value, with a factor 2 of headroom (as in test_pose.py).  Train-mode
    logits (batch-statistics BatchNorm): the feature-map tolerance."""
    g = fixture()
    nc, shape = CR.CASES[tag]
    m = build_model(nc)
    x = seeded_images(*shape, seed=CR.IMG_SEED).to(DEV)
    with torch.no_grad():
        p = m(x)
        m.train()
        lg = m._predict_once(x)
    assert p.dtype == torch.float32 and tuple(p.shape) == (shape[0], nc)
    bound = max(1e-4, 4 * float(g[f'{tag}_d64'][0]))
    err = float(np.abs(p.cpu().numpy().astype(np.float64) - g[f'{tag}_probs']).max())
    lerr = float(np.abs(lg.cpu().numpy().astype(np.float64) - g[f'{tag}_logits_train']).max())
    print(f'{tag}: probs err {err:.3e} (bound {bound:.3e}), train logits err {lerr:.3e}')
    assert err <= bound
    np.testing.assert_allclose(lg.cpu().numpy(), g[f'{tag}_logits_train'], atol=FEAT_ATOL, rtol=FEAT_RTOL)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', list(CR.CASES))
def test_cls_model_bf16_tracks_reference(tag):
    """bf16 compute: probabilities within 3 x the difference of the reference's bf16 emulation (gen_cls.py), argmax equal on every fixture image (the
    generator asserts a top-1 / top-2 gap of at least twice that bound)."""
    g = fixture()
    nc, shape = CR.CASES[tag]
    m = build_model(nc, dtype=torch.bfloat16)
    x = seeded_images(*shape, seed=CR.IMG_SEED).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        p = m(x).cpu().numpy()
    ref = g[f'{tag}_probs']
    err, bound = float(np.abs(p.astype(np.float64) - ref).max()), 3 * float(g[f'{tag}_dbf16'])
    print(f'{tag}: bf16 probs err {err:.3e} (bound {bound:.3e})')
    assert err <= bound
    assert np.array_equal(p.argmax(1), ref.argmax(1))


# ================================================================================================================ loss
LOSS_CASES = [(1, 1), (3, 2), (2, 10), (5, 1000)]


def loss_inputs(b, nc):
    r = np.random.default_rng([31, b, nc])
    lg = torch.from_numpy((r.standard_normal((b, nc)) * 20.0).astype(np.float32))
    lg[0, 0] = 50.0
    lg[-1, -1] = -50.0
    lab = torch.from_numpy(r.integers(0, nc, b).astype(np.int64))
    lab[0], lab[-1] = 0, nc - 1                                     # a label at each end of the range
    if b > 2:
        lab[1] = nc - 1
    return lg, lab


@pytest.mark.gpu
@pytest.mark.parametrize('b,nc', LOSS_CASES)
def test_cls_loss_kernels_match_float64(b, nc):
    """mgdt_cls_loss_fwd / _bwd against float64 cross_entropy(sum) / 64 with logits of magnitude 50 and labels at both ends of the range.  Bounds: a
    row's term logsumexp - logit[label] is computed in fp32 from values of magnitude M = max|logit| + log(nc): <= 8 ulp(M) = 8 * 2^-23 * M per row,
    summed over b rows and divided by 64.  The gradient: exp arguments of magnitude <= 100 carry half an ulp (3.8e-6) of absolute error, expf and the
    normalisation a few more ulp: relative 2e-5 on probabilities <= 1, divided by 64."""
    lg, lab = loss_inputs(b, nc)
    loss64, d64 = CR.loss64(lg, lab)
    loss, _ = ops.cls_loss_fwd(lg.to(DEV), lab.to(DEV))
    M = float(lg.abs().max()) + float(np.log(nc))
    tol = b * 8 * 2.0 ** -23 * M / 64
    print(f'({b}, {nc}): loss {float(loss):.6f} ref {float(loss64):.6f} err {abs(float(loss) - float(loss64)):.3e} (bound {tol:.3e})')
    assert abs(float(loss) - float(loss64)) <= tol
    for gs in (1.0, 2.5):
        d = ops.cls_loss_bwd(lg.to(DEV), lab.to(DEV), gs).cpu().double()
        assert float((d - d64 * gs).abs().max()) <= 2e-5 / 64 * gs
    # host labels take the same path after the range check
    assert float(ops.cls_loss_fwd(lg.to(DEV), lab)[0]) == float(loss)


@pytest.mark.gpu
def test_cls_loss_autograd_and_bad_device_labels():
    """v8ClassificationLoss: (loss, loss.detach()), backward through the autograd Function = the explicit form.  A label outside [0, nc) that is
    already on the device: NaN loss, zero gradient row, the other rows untouched (an in-bounds buffer: nothing is read past it)."""
    from mgdt_yolo_amd.yolo.utils.loss import cls_loss_and_head_grad, v8ClassificationLoss
    lg, lab = loss_inputs(3, 10)
    x = lg.to(DEV).requires_grad_(True)
    loss, item = v8ClassificationLoss()(x, {'cls': lab})
    assert item.requires_grad is False and float(item) == float(loss)
    (loss * 3.0).backward()
    l2, g2 = cls_loss_and_head_grad(lg.to(DEV), {'cls': lab.to(DEV)}, gscale=1.0)
    assert float(l2) == float(loss) and torch.equal(x.grad, g2 * 3.0)
    nograd, _ = v8ClassificationLoss()(lg.to(DEV), {'cls': lab})
    assert float(nograd) == float(loss)
    bad = lab.clone()
    bad[1] = 10
    lossb, _ = ops.cls_loss_fwd(lg.to(DEV), bad.to(DEV))
    assert bool(torch.isnan(lossb))
    d = ops.cls_loss_bwd(lg.to(DEV), bad.to(DEV)).cpu()
    assert bool((d[1] == 0).all()) and torch.equal(d[0], g2.cpu()[0]) and torch.equal(d[2], g2.cpu()[2])
    neg = lab.clone()
    neg[0] = -1
    assert bool(torch.isnan(ops.cls_loss_fwd(lg.to(DEV), neg.to(DEV))[0]))
    with pytest.raises(ValueError, match='outside'):
        ops.cls_loss_fwd(lg.to(DEV), bad)


# ================================================================================================================ training step
def _train_inputs(tag):
    nc, shape = CR.CASES[tag]
    return nc, seeded_images(*shape, seed=CR.IMG_SEED).to(DEV), CR.seeded_labels(shape[0], nc)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', CR.TRAIN_CASES)
def test_training_step_matches_the_reference(tag):
    """`loss, items = model(batch); loss.backward()` (the reference's call form: the HIP train-mode forward with batch-statistics BatchNorm, the loss
    kernels, the HIP reverse pass) against the reference's own CPU step (gen_cls.py:train_step): loss rtol 2e-5, every parameter gradient within
    2e-3 of its own rms (the fp32 bound of the whole-model training parity tests in test_hip_parity.py, with their floor of 1e-2 x the typical rms
    for tensors whose gradient is analytically ~0), BatchNorm running statistics 1e-5.  The head's gradients (layer 9) are compared whole, the
    backbone's on the stored sample and l2 norm.  The reference's own fp32-vs-fp64 gradient difference is at most 2.5e-5 of the rms
    (model.2.cv1.bn.weight, case n10_2x64x64; 1.0e-5 for n10_1x96x160), so the starting bound holds for the head's tensors as well and no wider
    one is used.  Measured on MI355X: see the printed worst tensor.  The explicit form cls_loss_and_head_grad + model.backward gives the same
    gradients bit for bit."""
    from mgdt_yolo_amd.yolo.utils.loss import cls_loss_and_head_grad
    g = fixture()
    pre = f'train_{tag}/'
    nc, x, cls = _train_inputs(tag)
    assert np.array_equal(cls.numpy(), g[pre + 'cls'])
    m = build_model(nc).train()
    loss, items = m({'img': x, 'cls': cls})
    assert loss.requires_grad and not items.requires_grad
    loss.backward()
    np.testing.assert_allclose(float(loss), float(g[pre + 'loss']), rtol=2e-5)
    grads = {k: p.grad.detach().float().cpu() for k, p in m.named_parameters() if p.grad is not None}
    names = str(g[pre + 'grad_names']).split('\n')
    assert set(names) == set(grads), set(names) ^ set(grads)
    rms_of = lambda k: float(g[pre + 'gst/' + k][0]) / np.sqrt(grads[k].numel())
    typical = float(np.median([rms_of(k) for k in names]))
    worst = (0.0, None)
    for k in names:
        denom = max(rms_of(k), 1e-2 * typical)
        if pre + 'g/' + k in g.keys():
            got, st = CR.grad_sample(grads[k])
            ref = g[pre + 'g/' + k]
        else:
            got = grads[k].numpy().reshape(-1)
            st = np.array([grads[k].double().norm().item()])
            ref = (g[pre + 'gfull/' + k] if pre + 'gfull/' + k in g.keys() else np.concatenate([g[pre + 'gfull0/' + k], g[pre + 'gfull1/' + k]])).reshape(-1)
        err = float(np.sqrt(np.mean((got.astype(np.float64) - ref) ** 2)) / denom)
        err = max(err, abs(st[0] - g[pre + 'gst/' + k][0]) / (denom * np.sqrt(grads[k].numel())))
        if err > worst[0]:
            worst = (err, k)
        assert err < 2e-3, (k, err)
    print(f'{tag}: loss {float(loss):.6f}; worst gradient error {worst[0]:.3e} of the tensor rms ({worst[1]})')
    bufs = dict(m.named_buffers())
    n_run = 0
    for key in g.keys():
        if key.startswith(pre + 'bn/'):
            np.testing.assert_allclose(bufs[key[len(pre) + 3:]].cpu().numpy(), g[key], atol=1e-5, rtol=1e-5, err_msg=key)
            n_run += 1
    assert n_run > 40
    # the explicit form
    m2 = build_model(nc).train()
    logits = m2._predict_once(x)
    loss2, hg = cls_loss_and_head_grad(logits, {'cls': cls})
    m2.backward(hg)
    assert float(loss2) == float(loss)
    for k, p in m2.named_parameters():
        assert torch.equal(p.grad.cpu(), grads[k]), k


# ================================================================================================================ top-k and confusion matrix
@pytest.mark.gpu
@pytest.mark.parametrize('b', [1, 33])
@pytest.mark.parametrize('nc', [1, 2, 5, 7, 1000])
def test_topk_and_confusion_matrix(nc, b):
    p = CR.topk_probs(b, nc, seed=17)
    t = CR.seeded_labels(b, nc, seed=4)
    n5 = min(nc, 5)
    want = p.argsort(1, descending=True)[:, :n5]
    mat = torch.zeros(nc, nc, dtype=torch.int32, device=DEV)
    got = ops.cls_topk(p.to(DEV), t.to(DEV), mat)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    ref = np.zeros((nc, nc), np.int64)
    for pi, ti in zip(want[:, 0].numpy(), t.numpy()):          # ConfusionMatrix.process_cls_preds (reference metrics.py:205-207)
        ref[pi][ti] += 1
    assert np.array_equal(mat.cpu().numpy(), ref)
    assert torch.equal(ops.cls_topk(p.to(DEV)).cpu(), want)    # without the matrix
    ops.cls_topk(p.to(DEV), t.to(DEV), mat)                    # the counts accumulate
    assert np.array_equal(mat.cpu().numpy(), 2 * ref)


@pytest.mark.gpu
def test_topk_orders_equal_values_by_lower_index():
    p = torch.full((2, 600), 0.25)
    p[1, 300], p[1, 17] = 0.5, 0.5
    got = ops.cls_topk(p.to(DEV)).cpu()
    assert got[0].tolist() == [0, 1, 2, 3, 4] and got[1].tolist() == [17, 300, 0, 1, 2]


# ================================================================================================================ the rest
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_eval_forward_replays_bit_equal_from_a_graph(dtype):
    m = build_model(10, dtype=dtype)
    xs = [seeded_images(2, 64, 64, seed=s).to(DEV).to(dtype) for s in (1, 2)]
    with torch.no_grad():
        ref = [m(x).clone() for x in xs]
        xin = xs[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(xin)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m(xin)
        for x, r in zip(xs[::-1], ref[::-1]):
            xin.copy_(x)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, r)
    assert not torch.equal(ref[0], ref[1])


@pytest.mark.gpu
def test_predictor_end_to_end_on_exact_size_crops():
    """Two seeded uint8 BGR images whose centre crop already is size x size (72 x 64 and 64 x 90 at size 64): the exact path (no interpolation).  The
    planes equal the hand-built crop + BGR->RGB + HWC->CHW, and the probabilities equal the model's on the hand-built /255 tensor within the fp32
    bound (the first convolution's uint8 loader divides by 255 itself)."""
    from mgdt_yolo_amd.yolo.v8.classify import ClassificationPredictor, classify_transforms
    r = np.random.default_rng([3, 8])
    imgs = [r.integers(0, 256, (72, 64, 3), dtype=np.uint8), r.integers(0, 256, (64, 90, 3), dtype=np.uint8)]
    crops = [imgs[0][4:68], imgs[1][:, 13:77]]
    hand = np.stack([np.ascontiguousarray(c[..., ::-1].transpose(2, 0, 1)) for c in crops])
    tf = classify_transforms(64)
    for im, h in zip(imgs, hand):
        assert np.array_equal(tf(im).cpu().numpy(), h)
    pred = ClassificationPredictor(dict(imgsz=64))
    pred.setup_model(build_model(10))
    rows = pred(imgs)
    assert len(rows) == 2 and all(tuple(p.shape) == (10,) and p.dtype == torch.float32 for p in rows)
    with torch.no_grad():
        want = pred.model(torch.from_numpy(hand).float().div(255.0).to(DEV))
    np.testing.assert_allclose(torch.stack(rows).cpu().numpy(), want.cpu().numpy(), atol=1e-4, rtol=0)
    np.testing.assert_allclose(torch.stack(rows).sum(1).cpu().numpy(), 1.0, atol=1e-5)
    # a resized crop runs too (interpolation unpinned): 100 x 80 -> 64 x 64
    assert tuple(tf(r.integers(0, 256, (100, 80, 3), dtype=np.uint8)).shape) == (3, 64, 64)


@pytest.mark.gpu
def test_validator_reproduces_the_reference_accuracies():
    """ClassificationValidator on the fixture batches (nc = 10): top-1 / top-5 equal what the reference's ClassifyMetrics gives on the reference's own
    probabilities with the same seeded targets (recomputed here from the stored probabilities by the reference's formula), and the confusion counts
    equal the reference loop."""
    from mgdt_yolo_amd.yolo.v8.classify import ClassificationValidator
    g = fixture()
    m = build_model(10)
    v = ClassificationValidator(DEV)
    v.init_metrics(m.names)
    ref_pred, ref_t = [], []
    for tag, (nc, shape) in CR.CASES.items():
        if nc != 10:
            continue
        t = CR.seeded_labels(shape[0], nc, seed=shape[1])
        batch = v.preprocess({'img': seeded_images(*shape, seed=CR.IMG_SEED), 'cls': t})
        with torch.no_grad():
            v.update_metrics(m(batch['img']), batch)
        ref_pred.append(torch.from_numpy(g[f'{tag}_probs']).argsort(1, descending=True)[:, :5])
        ref_t.append(t)
    v.finalize_metrics()
    stats = v.get_stats()
    pred, t = torch.cat(ref_pred), torch.cat(ref_t)
    correct = (t[:, None] == pred).float()
    top1, top5 = torch.stack((correct[:, 0], correct.max(1).values), dim=1).mean(0).tolist()
    assert stats == {'metrics/accuracy_top1': top1, 'metrics/accuracy_top5': top5, 'fitness': top5}
    cm = np.zeros((10, 10), np.int64)
    for pi, ti in zip(pred[:, 0].numpy(), t.numpy()):
        cm[pi][ti] += 1
    assert np.array_equal(v.confusion_matrix, cm) and int(v.confusion_matrix.sum()) == 5


@pytest.mark.gpu
def test_quantize_fp8_leaves_the_head_in_bf16():
    m = build_model(10, dtype=torch.bfloat16)
    x = seeded_images(2, 64, 64, seed=CR.IMG_SEED).to(DEV).to(torch.bfloat16)
    table = m.quantize_fp8(x)
    assert table and not any(k.startswith('model.9') for k in table), [k for k in table if k.startswith('model.9')]
    launches = []
    orig = ops._launch
    ops._launch = lambda name, *a, **k: (launches.append(name), orig(name, *a, **k))[1]
    try:
        with torch.no_grad():
            p = m(x)
    finally:
        ops._launch = orig
    assert 'conv2d_fp8_fwd' in launches and launches[-2:] == ['classify_pool_fwd', 'classify_linear_fwd']
    np.testing.assert_allclose(p.sum(1).cpu().numpy(), 1.0, atol=1e-5)
    # with the fused head off the head convolutions still run as bf16 (Classify.q8_site and the exclusion list)
    ops.FUSED_CLS_HEAD = False
    try:
        m.quantize_fp8(x)
        assert not any(k.startswith('model.9') for k in m.fp8_table)
    finally:
        ops.FUSED_CLS_HEAD = True
