"""YOLOv3 graphs (models/v3/yolov3.yaml, yolov3-spp.yaml, yolov3-tiny.yaml): nn.MaxPool2d / nn.ZeroPad2d rows, the SPP block, rows that read `from = -2`, a
two-level head, inference and training, against the reference-generated fixtures tests/golden/yolov3_NN.npz, yolov3_yaml.json, train_yolov3_tiny.npz and
train_yolov3_spp_w025.npz (tests/golden/gen_yolov3.py).  Host-side checks run without a GPU; everything that launches a kernel is marked gpu.  The kernels
and layers themselves are pinned in tests/test_pool_kernels.py.

Graphs under test (yolov3_ref.GRAPHS): `tiny` = yolov3-tiny at full width, `v3_w025` / `spp_w025` = yolov3 / yolov3-spp with width_multiple 0.25, and once
yolov3-spp at full width (the 512 -> 1024 and 1024 -> 512 3x3 convolutions).

Bounds, the rules of test_yolov6.py.  fp32 model: boxes 1e-3 px, confidences 1e-4, head maps atol 1e-3 / rtol 1e-4, each never below 4 x the reference's own
recorded fp32-vs-float64 difference (both printed; for these fixtures the contract binds everywhere, the generator prints it).  bf16 model: 3 x the bf16
emulation error the generator recorded for the reference itself.  fp32 training step: loss 2e-5, head maps 2e-4, gradients 2e-3 of the tensor's rms with
the 1e-2 x typical floor, running statistics 1e-5, each never below 4 x the reference's own fp32-vs-float64 difference.  bf16 step: loss, head maps and
running statistics within 3 x the distance of the reference's own bf16-emulated step, and for every gradient tensor whose cosine in that emulation is at
least yolov6_ref.INFORMATIVE_COS the device's cosine >= 1 - 9 x (1 - the emulation's) (3 x the relative error; test_yolov6.py derives the rule).
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import inputs as GI
import yolov3_ref as Y3
from mgdt_yolo_amd import _lib, ops
from mgdt_yolo_amd.seeding import seeded_images

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
DTS = [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')]
TAGS = list(Y3.GRAPHS)
_FIX = []


def fixture():
    if not _FIX:
        _FIX.append(Y3.load_fixture())
    return _FIX[0]


def build_model(tag, dtype=F32, nc=80, device=DEV, seed=None, gain=None):
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    g = fixture()
    name, width = (Y3.FULL[1], Y3.FULL[2]) if tag == Y3.FULL[0] else Y3.GRAPHS[tag]
    m = Y3.seed_model_(DetectionModel(Y3.graph_cfg(name, width, nc), verbose=False), int(g[f'{tag}/seed']) if seed is None else seed,
                       float(g[f'{tag}/gain']) if gain is None else gain).eval().set_compute_dtype(dtype)
    return m.to(device) if device else m


def to_nchw(t):
    return t.detach().float().contiguous().cpu().numpy()


# ================================================================================================ host side (no GPU)
def test_tables_equal_the_reference_yaml_files():
    ref = json.load(open(os.path.join(Y3.GOLDEN, 'yolov3_yaml.json')))
    from mgdt_yolo_amd.models import ALL_CONFIGS, CONFIGS, V3_CONFIGS, get_config
    assert sorted(V3_CONFIGS) == sorted(Y3.NAMES) == sorted(ref)
    for n in Y3.NAMES:
        assert ALL_CONFIGS[n] is V3_CONFIGS[n] and n not in CONFIGS
        cfg = get_config(n)
        for k in ('nc', 'depth_multiple', 'width_multiple', 'backbone', 'head'):
            assert cfg[k] == ref[n][k], (n, k)
        assert 'scales' not in cfg and get_config(n, nc=3)['nc'] == 3 and get_config(n, 'n', nc=3)['head'] == cfg['head']
    assert len(CONFIGS) == 6 and all('v8' in k for k in CONFIGS)


def test_names_resolve_without_a_file_and_have_no_scale_letter():
    from mgdt_yolo_amd.nn.tasks import DetectionModel, guess_model_scale, guess_model_task, model_class_of, yaml_model_load
    for n in Y3.NAMES:
        assert guess_model_scale(f'{n}.yaml') == '' and guess_model_task(f'{n}.yaml') == 'detect'
        d = yaml_model_load(f'{n}.yaml')
        assert d['scale'] == '' and d['yaml_file'] == f'{n}.yaml' and guess_model_task(d) == 'detect' and model_class_of(d) is DetectionModel
    assert yaml_model_load('yolov3-spp.yaml')['head'][1] == [-1, 1, 'SPP', [512, [5, 9, 13]]]
    assert yaml_model_load('yolov3-tiny.yaml')['backbone'][11:] == [[-1, 1, 'nn.ZeroPad2d', [[0, 1, 0, 1]]], [-1, 1, 'nn.MaxPool2d', [2, 1, 0]]]
    with pytest.raises(FileNotFoundError):
        yaml_model_load('yolov3-huge.yaml')


@pytest.mark.parametrize('tag', TAGS + ['v3_full', 'spp_full'])
def test_parse_model_gives_the_reference_structure(tag):
    """state-dict keys, shapes, parameter count and strides of the three graphs at full width and of the two darknet53 graphs at width 0.25"""
    from mgdt_yolo_amd.nn.modules import SPP, Bottleneck, Conv, Detect, MaxPool2d, Repeat, ZeroPad2d
    from mgdt_yolo_amd.nn.tasks import REGISTRY, DetectionModel, guess_model_task
    g = fixture()
    name, width = {'v3_full': ('yolov3', 1.0), 'spp_full': ('yolov3-spp', 1.0)}.get(tag) or Y3.GRAPHS[tag]
    before = Conv.default_act
    m = DetectionModel(f'{name}.yaml', verbose=False) if width == 1.0 else DetectionModel(Y3.graph_cfg(name, width), verbose=False)
    assert Conv.default_act is before and isinstance(before, nn.SiLU)
    sd = m.state_dict()
    assert list(sd.keys()) == g[f'{tag}/keys'].tolist()
    assert [','.join(map(str, v.shape)) for v in sd.values()] == g[f'{tag}/shapes'].tolist()
    assert sum(p.numel() for p in m.parameters()) == int(g[f'{tag}/nparams'])
    strides = [16.0, 32.0] if name == 'yolov3-tiny' else [8.0, 16.0, 32.0]
    assert m.stride.tolist() == g[f'{tag}/stride'].tolist() == strides and guess_model_task(m) == 'detect'
    head = m.model[-1]
    assert isinstance(head, Detect) and head.nl == len(strides) and head.f == ([19, 15] if name == 'yolov3-tiny' else [27, 22, 15])
    assert REGISTRY['nn.MaxPool2d'] is MaxPool2d and REGISTRY['nn.ZeroPad2d'] is ZeroPad2d and REGISTRY['SPP'] is SPP
    assert all(isinstance(c.act, nn.SiLU) for c in m.modules() if isinstance(c, Conv))
    if name == 'yolov3-tiny':
        pools = [l for l in m.model if isinstance(l, MaxPool2d)]
        assert [l.i for l in pools] == [1, 3, 5, 7, 9, 12] and all(isinstance(l, nn.MaxPool2d) for l in pools)
        assert [(l.kernel_size, l.stride, l.padding) for l in pools] == [(2, 2, 0)] * 5 + [(2, 1, 0)]
        assert isinstance(m.model[11], ZeroPad2d) and isinstance(m.model[11], nn.ZeroPad2d) and tuple(m.model[11].padding) == (0, 1, 0, 1)
        assert m.model[16].f == -2 and m._reductions[9] == 32 and m._reductions[12] == 32 and m.model[1].c2 == 16
    else:
        assert m.model[16].f == -2 and m.model[23].f == -2
        assert isinstance(m.model[6], Repeat) and len(m.model[6]) == 8 and isinstance(m.model[6][0], Bottleneck) and len(m.model[27]) == 2
        assert isinstance(m.model[12], SPP) == (name == 'yolov3-spp') and isinstance(m.model[12], Conv) == (name == 'yolov3')
        if name == 'yolov3-spp':
            c12 = int(512 * width)
            assert m.model[12].cv1.conv.out_channels == int(1024 * width) // 2 and m.model[12].cv2.conv.out_channels == c12
    assert not m._stem_fusable(torch.zeros(1, 3, 64, 64, dtype=BF16)), 'layer 0 is a stride-1 Conv: the two-layer stem kernel is not for these graphs'


@pytest.mark.parametrize('args,kw', [((3, 2, 1), {}), ((2, 2, 1), {}), ((2, 2, 0), dict(ceil_mode=True)), ((2, 2, 0, 2), {}), ((2, 2, 0), dict(return_indices=True)),
                                     ((2, 3, 0), {}), ((3,), {})], ids=['k3s2p1', 'k2s2p1', 'ceil', 'dilation2', 'indices', 'k2s3', 'k3'])
def test_other_pool_geometries_raise_at_construction(args, kw):
    from mgdt_yolo_amd.models import get_config
    from mgdt_yolo_amd.nn.modules import MaxPool2d
    from mgdt_yolo_amd.nn.tasks import parse_model
    with pytest.raises(RuntimeError, match='max pooling: only kernel 2'):
        MaxPool2d(*args, **kw)
    if not kw:
        cfg = get_config('yolov3-tiny')
        cfg['backbone'][1] = [-1, 1, 'nn.MaxPool2d', list(args)]
        with pytest.raises(RuntimeError, match='max pooling: only kernel 2'):
            parse_model(cfg, 3, verbose=False)                                         # before any launch: nothing here touches a device


def test_built_pool_geometries_other_spp_windows_and_negative_pads():
    from mgdt_yolo_amd.nn.modules import SPP, MaxPool2d, ZeroPad2d
    assert MaxPool2d(2, 2, 0)._s == 2 and MaxPool2d(2, 1, 0)._s == 1 and MaxPool2d(2)._s == 2 and MaxPool2d((2, 2), (1, 1))._s == 1
    assert ops.check_maxpool2d(2, None) == (2, 2)
    for k in ((3, 5, 7), (5, 9), (5, 9, 13, 17), [13, 9, 5]):
        with pytest.raises(RuntimeError, match='SPP: k='):
            SPP(32, 32, k)
    assert [p.kernel_size for p in SPP(32, 32, [5, 9, 13]).m] == [5, 9, 13]
    for p in ((0, -1, 0, 1), (-1, 0, 0, 0), -1):
        with pytest.raises(RuntimeError, match='ZeroPad2d: four non-negative'):
            ZeroPad2d(p)
    assert tuple(ZeroPad2d(1).padding) == (1, 1, 1, 1) and tuple(ZeroPad2d([0, 1, 0, 1]).padding) == (0, 1, 0, 1)


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'mgdt.h')).read()
    declared = set(re.findall(r'\b(mgdt_[a-z0-9_]+)\s*\(', hdr))
    lib = _lib.lib()
    for name in ('mgdt_maxpool2d_fwd', 'mgdt_maxpool2d_bwd', 'mgdt_spp_pool_bwd'):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    # refusals happen on the host, before any GPU call
    v = lambda h, w, c, p=4096, sc=1: C.byref(_lib.View(p, 2, h, w, c, h * w * c, w * c, c, sc))
    BAD_ARG, BAD_SHAPE, BAD_DTYPE = -4, -1, -2
    assert lib.mgdt_maxpool2d_fwd(None, None, 2, 2, 0, None) == BAD_ARG and lib.mgdt_maxpool2d_fwd(v(4, 4, 8), v(2, 2, 8, 0), 2, 2, 0, None) == BAD_ARG
    for k, s in ((3, 2), (2, 3), (2, 0), (5, 1)):
        assert lib.mgdt_maxpool2d_fwd(v(4, 4, 8), v(2, 2, 8), k, s, 0, None) == BAD_ARG
        assert lib.mgdt_maxpool2d_bwd(v(4, 4, 8), v(2, 2, 8), v(4, 4, 8), k, s, 0, None) == BAD_ARG
    assert lib.mgdt_maxpool2d_fwd(v(4, 4, 8), v(3, 2, 8), 2, 2, 0, None) == BAD_SHAPE          # floor((4 - 2) / 2) + 1 = 2 rows
    assert lib.mgdt_maxpool2d_fwd(v(4, 4, 8), v(2, 2, 8), 2, 1, 0, None) == BAD_SHAPE          # stride 1 gives 3 x 3
    assert lib.mgdt_maxpool2d_fwd(v(5, 5, 8), v(3, 3, 8), 2, 2, 0, None) == BAD_SHAPE          # no ceil mode
    assert lib.mgdt_maxpool2d_fwd(v(1, 4, 8), v(1, 2, 8), 2, 2, 0, None) == BAD_SHAPE          # smaller than the window
    assert lib.mgdt_maxpool2d_fwd(v(4, 4, 8), v(2, 2, 4), 2, 2, 0, None) == BAD_SHAPE
    assert lib.mgdt_maxpool2d_fwd(v(4, 4, 8, sc=2), v(2, 2, 8), 2, 2, 0, None) == BAD_SHAPE    # not NHWC
    assert lib.mgdt_maxpool2d_fwd(v(4, 4, 8), v(2, 2, 8), 2, 2, 7, None) == BAD_DTYPE
    assert lib.mgdt_maxpool2d_bwd(v(4, 4, 8), v(2, 2, 8), None, 2, 2, 0, None) == BAD_ARG
    assert lib.mgdt_maxpool2d_bwd(v(4, 4, 8), v(2, 2, 8), v(4, 3, 8), 2, 2, 0, None) == BAD_SHAPE
    assert lib.mgdt_maxpool2d_bwd(v(4, 4, 8), v(2, 2, 8), v(4, 4, 8), 2, 2, 9, None) == BAD_DTYPE
    a = v(4, 4, 8)
    assert lib.mgdt_spp_pool_bwd(a, a, a, None, 4096, 0, None) == BAD_ARG and lib.mgdt_spp_pool_bwd(a, a, a, a, None, 0, None) == BAD_ARG
    assert lib.mgdt_spp_pool_bwd(a, a, a, v(4, 5, 8), 4096, 0, None) == BAD_SHAPE and lib.mgdt_spp_pool_bwd(a, a, v(4, 4, 4), a, 4096, 0, None) == BAD_SHAPE
    assert lib.mgdt_spp_pool_bwd(a, a, a, a, 4096, 5, None) == BAD_DTYPE


# ================================================================================================ GPU: the models
def _fp32_bounds(g, key):
    """max(contract, 4 x the reference's own fp32-vs-float64 difference), per quantity (box px, conf, head maps)"""
    d64 = g[f'{key}_d64']
    contract = (1e-3, 1e-4, 1e-3)
    out = [max(c, 4 * float(d)) for c, d in zip(contract, d64)]
    print(f'{key}: contract {contract}, 4 x fp32-vs-float64 of the reference {[4 * float(d) for d in d64]} -> bounds {out}')
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
def test_e2e_fp32_matches_the_reference(tag):
    g = fixture()
    m = build_model(tag)
    for shape in Y3.E2E_SHAPES:
        key = f'{tag}/' + 'x'.join(map(str, shape))
        x = seeded_images(*shape, seed=Y3.IMG_SEED).to(DEV)
        with torch.no_grad():
            y, feats = m(x)
        assert y.shape[-1] == int(g[f'{key}_anchors']) and len(feats) == len(Y3.STRIDES[tag])
        y = y.cpu().numpy()
        bb, bc, bf = _fp32_bounds(g, key)
        print(f'{key}: box err {np.abs(y[:, :4] - g[f"{key}_y"][:, :4]).max():.3e} px, conf err {np.abs(y[:, 4:] - g[f"{key}_y"][:, 4:]).max():.3e}')
        np.testing.assert_allclose(y[:, :4], g[f'{key}_y'][:, :4], atol=bb, rtol=0)
        np.testing.assert_allclose(y[:, 4:], g[f'{key}_y'][:, 4:], atol=bc, rtol=0)
        for i, f in enumerate(feats):
            np.testing.assert_allclose(to_nchw(f), g[f'{key}_feat{i}'], atol=bf, rtol=1e-4)
    x = seeded_images(2, 64, 96, seed=Y3.IMG_SEED).to(DEV)
    with torch.no_grad():
        y0, _ = m(x)
        yf, _ = m.fuse()(x)
    assert m.is_fused() and not hasattr(m.model[0], 'bn')
    bb, bc, _ = _fp32_bounds(g, f'{tag}/2x64x96')
    np.testing.assert_allclose(yf.cpu().numpy()[:, :4], g[f'{tag}/2x64x96_yfused'][:, :4], atol=bb, rtol=0)
    np.testing.assert_allclose(yf.cpu().numpy()[:, 4:], g[f'{tag}/2x64x96_yfused'][:, 4:], atol=bc, rtol=0)
    np.testing.assert_allclose(yf.cpu().numpy()[:, :4], y0.cpu().numpy()[:, :4], atol=1e-3, rtol=0)
    np.testing.assert_allclose(yf.cpu().numpy()[:, 4:], y0.cpu().numpy()[:, 4:], atol=1e-4, rtol=0)


@pytest.mark.gpu
def test_full_width_yolov3_spp_fp32_matches_the_reference():
    """the one case that runs the 1024-channel layers (512 -> 1024 and 1024 -> 512 3x3 convolutions, SPP over 512 channels); full yolov3 is a row subset"""
    g = fixture()
    tag = Y3.FULL[0]
    m = build_model(tag)
    with torch.no_grad():
        y, _ = m(seeded_images(*Y3.FULL_SHAPE, seed=Y3.IMG_SEED).to(DEV))
    y, ref = y.cpu().numpy(), g[f'{tag}/' + 'x'.join(map(str, Y3.FULL_SHAPE)) + '_y']
    print(f'{tag}: box err {np.abs(y[:, :4] - ref[:, :4]).max():.3e} px, conf err {np.abs(y[:, 4:] - ref[:, 4:]).max():.3e}')
    np.testing.assert_allclose(y[:, :4], ref[:, :4], atol=1e-3, rtol=0)
    np.testing.assert_allclose(y[:, 4:], ref[:, 4:], atol=1e-4, rtol=0)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
def test_e2e_bf16_within_three_times_the_reference_emulation_error(tag):
    g = fixture()
    for fuse in (False, True):
        m = build_model(tag, BF16)
        if fuse:
            m.fuse()
        for shape in Y3.E2E_SHAPES:
            key = f'{tag}/' + 'x'.join(map(str, shape))
            with torch.no_grad():
                y, feats = m(seeded_images(*shape, seed=Y3.IMG_SEED).to(DEV))
            y, ref = y.cpu().numpy(), g[f'{key}_y']
            d = [float(np.abs(y[:, :4] - ref[:, :4]).max()), float(np.abs(y[:, 4:] - ref[:, 4:]).max()),
                 max(float(np.abs(to_nchw(f) - g[f'{key}_feat{i}']).max()) for i, f in enumerate(feats))]
            bound = 3 * g[f'{key}_dbf16']
            print(f'bf16 {key} fused={fuse}: ' + '  '.join(f'{q} {v:.3e} (bound {b:.3e})' for q, v, b in zip(Y3.BF16_QUANTITIES, d, bound)))
            for q, v, b in zip(Y3.BF16_QUANTITIES, d, bound):
                assert v <= b, (key, fuse, q, v, b)


def _launches(model, inp):
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


@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('tag', TAGS)
def test_fused_equals_unfused_launches_and_captured_equals_eager(tag, dt):
    """forward + decode captured into one graph: bit-equal to the eager call; the fused model takes the same launches as the unfused one, no pack launch
    enters a warm call, and the two-layer stem kernel steps aside (layer 0 has stride 1)"""
    m = build_model(tag, dt)
    x = seeded_images(2, 64, 96, seed=Y3.IMG_SEED).to(DEV)
    y0, n0 = _launches(m, x)
    static = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        yg, _ = m(static)
    static.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y0)
    assert 'conv_pack' not in n0 and 'stem2_fwd' not in n0
    assert n0.count('maxpool2d_fwd') == (6 if tag == 'tiny' else 0) and n0.count('sppf_pool_fwd') == (1 if tag == 'spp_w025' else 0)
    y1, n1 = _launches(m.fuse(), x)
    assert n1 == n0
    if dt == F32:
        np.testing.assert_allclose(y1.cpu().numpy(), y0.cpu().numpy(), atol=1e-3, rtol=0)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
def test_nms_rows_equal_the_oracle_pipeline_on_the_same_y(tag):
    from mgdt_yolo_amd.yolo.utils.ops import nms_with_index
    from oracle import nms as ON
    m = build_model(tag)
    with torch.no_grad():
        y, _ = m(seeded_images(2, 64, 96, seed=Y3.IMG_SEED).to(DEV))
    total = 0
    for kw in Y3.NMS_SETTINGS:
        rows, kept = nms_with_index(y, **kw)
        orows, okept = ON.non_max_suppression(y.cpu().numpy(), return_index=True, **kw)
        for i in range(2):
            assert np.array_equal(kept[i].cpu().numpy().astype(np.int64), okept[i][0])
            assert np.array_equal(rows[i].cpu().numpy(), orows[i])
            total += len(okept[i][0])
    assert total > 0


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
def test_augment_equals_the_three_composed_single_passes(tag):
    from test_tta import _compose, _scale_args
    from mgdt_yolo_amd.nn.tasks import tta_geometry
    m = build_model(tag)
    nl = len(Y3.STRIDES[tag])
    x = seeded_images(1, 160, 224, seed=Y3.IMG_SEED).to(DEV)
    with torch.no_grad():
        y0, _ = m(x, augment=True)
        xs = [x, ops.scale_img(x, *_scale_args(160, 224, 0.83, 32), True, F32), ops.scale_img(x, *_scale_args(160, 224, 0.67, 32), False, F32)]
        y_own = _compose([m(xi)[0].cpu() for xi in xs], x.shape, nl)
    assert y0.shape == y_own.shape == (1, 84, tta_geometry(160, 224, Y3.STRIDES[tag])['anchors'])
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
def test_predictor_load_and_fp8_take_the_graphs_without_special_cases():
    """DetectionPredictor (AutoBackend(fuse=True) inside) on yolov3-tiny against the same steps by hand; half=True selects bf16; load() transfers every
    tensor; quantize_fp8 switches the convolutions and leaves the pooling layers and SPP's pools alone (they hold no fp8 site)."""
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    from mgdt_yolo_amd.yolo.v8.detect import DetectionPredictor
    from oracle import metrics as OM, nms as ON
    g = fixture()
    mk = lambda: Y3.seed_model_(DetectionModel('yolov3-tiny.yaml', verbose=False), int(g['tiny/seed']), float(g['tiny/gain']))
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
    assert pr16.model.fp16 and pr16.model.model.compute_dtype == BF16 and len(pr16(imgs)) == 2
    a, b = mk(), DetectionModel('yolov3-tiny.yaml', verbose=False)
    b.load(a, verbose=False)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    x = seeded_images(2, 64, 96, seed=Y3.IMG_SEED).to(DEV)
    for tag, skip in (('tiny', [f'model.{i}' for i in (1, 3, 5, 7, 9, 11, 12)]), ('spp_w025', ['model.12.m'])):
        m = build_model(tag, BF16)
        with torch.no_grad():
            y0, _ = m(x)
            table = m.quantize_fp8(x)
            y1, _ = m(x)
        assert table and not any(k.split(':')[0] in skip or k.startswith('model.12.m') for k in table)
        assert (y1 - y0).abs().max().item() > 0
        m.dequantize_fp8()
        with torch.no_grad():
            assert torch.equal(m(x)[0], y0)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
def test_validator_takes_the_graph_without_special_cases(tag):
    """test_yolov6.py's validator case on these graphs' own output: mAP50 and mAP50-95 equal the oracle's numpy pipeline on the same y"""
    from mgdt_yolo_amd.yolo.v8.detect import DetectionValidator
    from oracle import metrics as OM, nms as ON, val as OV
    B, S, nc = 2, 96, 80
    m = build_model(tag)
    with torch.no_grad():
        y, _ = m(seeded_images(B, S, S, seed=Y3.IMG_SEED).to(DEV))
    r = np.random.default_rng(4)
    det_ref = ON.non_max_suppression(y.cpu().numpy(), conf_thres=0.001, iou_thres=0.7, multi_label=True, max_det=300, compiled=True)
    cls_l, box_l, idx_l = [], [], []
    for si, rows in enumerate(det_ref):
        rows = rows[:len(rows) // 2].copy()
        wh = np.stack([rows[:, 2] - rows[:, 0], rows[:, 3] - rows[:, 1]], 1)
        rows[:, :4] += (r.standard_normal((len(rows), 4)) * 0.06 * np.concatenate([wh, wh], 1)).astype(np.float32)
        ex = rows[r.integers(0, len(rows), 5)].copy()
        ex[:, :4] += r.uniform(20, 40, (5, 1)).astype(np.float32)
        rows = np.concatenate([rows, ex]).astype(np.float32)
        rows[:, [0, 2]] = rows[:, [0, 2]].clip(0, S - 1); rows[:, [1, 3]] = rows[:, [1, 3]].clip(0, S - 1)
        xywh = np.stack([(rows[:, 0] + rows[:, 2]) / 2 / S, (rows[:, 1] + rows[:, 3]) / 2 / S, (rows[:, 2] - rows[:, 0]) / S, (rows[:, 3] - rows[:, 1]) / S], 1)
        cls_l.append(rows[:, 5:6]); box_l.append(xywh.astype(np.float32)); idx_l.append(np.full(len(rows), si, np.float32))
    batch = dict(img=torch.zeros(B, 3, S, S, dtype=torch.uint8, device=DEV), cls=torch.from_numpy(np.concatenate(cls_l)), bboxes=torch.from_numpy(np.concatenate(box_l)),
                 batch_idx=torch.from_numpy(np.concatenate(idx_l)), ori_shape=[(S, S)] * B, ratio_pad=[((1.0, 1.0), (0.0, 0.0))] * B)
    iouv, stats = torch.linspace(0.5, 0.95, 10), []
    for si, det in enumerate(det_ref):
        xywh = box_l[si]
        tb = np.stack([xywh[:, 0] - xywh[:, 2] / 2, xywh[:, 1] - xywh[:, 3] / 2, xywh[:, 0] + xywh[:, 2] / 2, xywh[:, 1] + xywh[:, 3] / 2], 1).astype(np.float32) * np.float32(S)
        tb = OM.scale_boxes((S, S), tb, (S, S), ((1.0, 1.0), (0.0, 0.0)))
        predn = OM.scale_boxes((S, S), det[:, :4].copy(), (S, S), ((1.0, 1.0), (0.0, 0.0)))
        correct = OV.process_batch(torch.from_numpy(np.concatenate([predn, det[:, 4:]], 1)), torch.from_numpy(np.concatenate([cls_l[si], tb], 1)), iouv)
        stats.append((np.asarray(correct), det[:, 4], det[:, 5], cls_l[si][:, 0]))
    tp, conf, pcls, tcls = [np.concatenate(v, 0) for v in zip(*stats)]
    ap = OM.ap_per_class(tp, conf, pcls, tcls)[5]
    ref50, ref5095 = float(ap[:, 0].mean()), float(ap.mean())
    v = DetectionValidator(DEV)
    v.init_metrics(nc=nc)
    v.update_metrics(v.postprocess(y), batch)
    res = v.get_stats()
    print(f'{tag} validator: mAP50 {res["metrics/mAP50(B)"]:.6f} (oracle {ref50:.6f}), mAP50-95 {res["metrics/mAP50-95(B)"]:.6f} (oracle {ref5095:.6f}), {len(tcls)} labels')
    assert 0.05 < ref50 < 0.999
    assert abs(res['metrics/mAP50(B)'] - ref50) < 1e-6 and abs(res['metrics/mAP50-95(B)'] - ref5095) < 1e-6


# ------------------------------------------------------------------------------------------------ training
TRAIN_TAGS = list(Y3.TRAIN)
_TRAIN = {}


def _train_case(tag):
    if tag not in _TRAIN:
        _TRAIN[tag] = Y3.load_train(tag)
    g = _TRAIN[tag]
    return g, int(g['weight_seed']), float(g['gain'])


def _hip_train_step(tag, amp, x, lab, nc, seed, gain):
    from mgdt_yolo_amd.yolo.utils.loss import loss_and_head_grads, v8DetectionLoss
    m = build_model(tag, nc=nc, seed=seed, gain=gain).train()
    if amp:
        m.set_compute_dtype(BF16)
    feats = m._predict_once(x.to(DEV).to(BF16 if amp else F32))
    total, items, hg = loss_and_head_grads(v8DetectionLoss(m), feats, lab)
    m.backward(hg)
    assert all(not mod.__dict__.get('_ctx') for mod in m.modules()), 'a layer kept its context past backward()'
    grads = {k: p.grad.detach().float().cpu() for k, p in m.named_parameters() if p.grad is not None}
    bufs = dict(m.named_buffers())
    running = {k[:-len('.running_mean')]: (b.detach().cpu().numpy(), bufs[k[:-len('running_mean')] + 'running_var'].detach().cpu().numpy())
               for k, b in bufs.items() if k.endswith('running_mean')}
    return total, items, [to_nchw(f.float()) for f in feats], grads, running


def check_train_step(g, loss, items, feats, grads, running):
    """test_yolov6.check_train_step's figures: loss 2e-5, head maps 2e-4, gradients 2e-3 of the tensor's rms with the 1e-2 x typical floor, running statistics
    1e-5, each never below 4 x the difference the reference's own fp32 step shows against its float64 step (`d64`, `gd64/<name>`, `d64_run`); both printed."""
    d_loss, d_feat, _ = (float(v) for v in g['d64'])
    tl, tf, tr = max(2e-5, 4 * d_loss), max(2e-4, 4 * d_feat), max(1e-5, 4 * float(g['d64_run']))
    print(f'bounds: loss {tl:.2e} (contract 2e-5, 4 x d64 {4 * d_loss:.2e}), head maps {tf:.2e} (2e-4, {4 * d_feat:.2e}), running statistics {tr:.2e} (1e-5, {4 * float(g["d64_run"]):.2e})')
    print(f'loss {float(loss):.6f} vs {float(g["loss"]):.6f}; head maps max err {max(float(np.abs(np.asarray(f) - g[f"feat{i}"]).max()) for i, f in enumerate(feats)):.3e}')
    np.testing.assert_allclose(float(loss), float(g['loss']), rtol=tl)
    np.testing.assert_allclose(np.asarray(items, np.float64), g['items'], rtol=tl)
    for i, f in enumerate(feats):
        np.testing.assert_allclose(np.asarray(f), g[f'feat{i}'], atol=tf, rtol=tf)
    names = str(g['grad_names']).split('\n')
    numel = {k: max(int(np.prod(np.shape(grads[k]))), 1) for k in names}
    typical = float(np.median([g['gst/' + k][0] / np.sqrt(numel[k]) for k in names]))
    worst, bad, raised = (0.0, None), [], 0
    for k in names:
        assert k in grads and grads[k] is not None, f'no gradient for {k}'
        got, st = GI.grad_sample(grads[k])
        ref, rst = g['g/' + k], g['gst/' + k]
        denom = max(rst[0] / np.sqrt(numel[k]), 1e-2 * typical)
        err = max(float(np.sqrt(np.mean((got.astype(np.float64) - ref) ** 2)) / denom), abs(st[0] - rst[0]) / (denom * np.sqrt(numel[k])))
        own = 4 * float(g['gd64/' + k]) / denom
        bound = max(2e-3, own)
        raised += own > 2e-3
        if err / bound > worst[0]:
            worst = (err / bound, k, err, bound)
        if not err < bound:
            bad.append((k, err, bound))
    print(f'gradients: {raised} of {len(names)} tensors take 4 x the reference\'s own fp32-vs-float64 difference instead of 2e-3; largest share of a bound {worst}')
    assert not bad, bad
    n_run = 0
    for key in g.files:
        if key.startswith('bn/') and key.endswith('running_mean'):
            pre = key[3:-len('.running_mean')]
            mu, var = running[pre]
            np.testing.assert_allclose(np.asarray(mu), g[key], atol=tr, rtol=tr, err_msg=pre)
            np.testing.assert_allclose(np.asarray(var), g[f'bn/{pre}.running_var'], atol=tr, rtol=tr, err_msg=pre)
            n_run += 1
    assert n_run == len(running) > 15


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TRAIN_TAGS)
def test_training_step_matches_the_reference_training_fixture(tag):
    """The fp32 train-mode forward, loss and reverse pass against the reference's own `model.train()(batch); loss.backward()` on the CPU; a second step from
    the same state gives the same bits."""
    g, seed, gain = _train_case(tag)
    c = GI.TRAIN_CASE
    x, lab = GI.train_inputs()
    total, items, feats, grads, running = _hip_train_step(tag, False, x, lab, c['nc'], seed, gain)
    assert len(grads) == len(str(g['grad_names']).split('\n'))
    check_train_step(g, total.item(), items.cpu().numpy(), feats, grads, running)
    total2, _, feats2, grads2, _ = _hip_train_step(tag, False, x, lab, c['nc'], seed, gain)
    assert total2.item() == total.item() and all(np.array_equal(a, b) for a, b in zip(feats, feats2)) and all(torch.equal(grads[k], grads2[k]) for k in grads)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TRAIN_TAGS)
def test_bf16_training_step_vs_the_reference_training_fixture(tag):
    g, seed, gain = _train_case(tag)
    c = GI.TRAIN_CASE
    x, lab = GI.train_inputs()
    total, items, feats, grads, running = _hip_train_step(tag, True, x, lab, c['nc'], seed, gain)
    f = Y3.train_figures(g, total.item(), feats, grads, running)
    e = dict(zip(Y3.TRAIN_FIGURES, (float(v) for v in g['dbf16'])))
    bd = dict(loss=3 * e['loss'], feat=3 * e['feat'], run=3 * e['run'])
    print(f'bf16 {tag} figures', {k: f[k] for k in Y3.TRAIN_FIGURES}, 'bounds', bd, '(overall and lowest cosine: printed only)')
    assert all(np.isfinite(f[k]) for k in Y3.TRAIN_FIGURES) and all(np.isfinite(v) for v in f['per'].values())
    assert f['loss'] < bd['loss'] and f['feat'] < bd['feat'] and f['run'] < bd['run'], (f, bd)
    emul = {k: float(g['cbf16/' + k]) for k in f['per']}
    held = {k: 1 - 9 * (1 - v) for k, v in emul.items() if v >= Y3.INFORMATIVE_COS}
    assert len(held) >= 0.9 * len(emul), 'most tensors stay informative in the reference\'s own emulation of these graphs'
    bad = []
    for k, b in sorted(held.items()):
        if not f['per'][k] >= b:
            bad.append((k, f['per'][k], emul[k], b))
    low = sorted((f['per'][k] - held[k], k, f['per'][k], emul[k], held[k]) for k in held)[:3]
    print(f'  {len(held)} of {len(emul)} tensors held; closest to their bound (margin, name, device cosine, emulation cosine, bound): {low}')
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TRAIN_TAGS)
def test_loss_backward_and_trainer_step_give_bit_equal_gradients(tag):
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    g, seed, gain = _train_case(tag)
    c = GI.TRAIN_CASE
    x, lab = GI.train_inputs()
    m = build_model(tag, nc=c['nc'], seed=seed, gain=gain).train()
    loss, items = m(dict(img=x.to(DEV), **lab))
    assert loss.requires_grad and items.shape == (3,)
    loss.backward()
    m2 = build_model(tag, nc=c['nc'], seed=seed, gain=gain).train()
    tr = DetectionTrainer(m2, lr0=0.0)
    total, items2 = tr.step(dict(img=x.to(DEV), **lab))
    assert torch.equal(loss.detach(), total) and torch.equal(items, items2)
    n = 0
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        if p.grad is None:
            continue
        assert torch.equal(p.grad, p2.grad), k
        n += 1
    assert n == len(str(g['grad_names']).split('\n'))


@pytest.mark.gpu
@pytest.mark.parametrize('amp', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('tag', TRAIN_TAGS)
def test_two_captured_training_steps_equal_two_eager_steps(tag, amp):
    """DetectionTrainer(graph=True): the first step is eager, the next ones replay one captured graph; three steps, so two go through the graph path (capture
    + one replay) - losses, weights and EMA equal the eager trainer's bit for bit (the pooling reverse passes have no atomics and no host decision)."""
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    from mgdt_yolo_amd.seeding import seeded_labels
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    g = fixture()
    nc, B, S = 4, 4, 96
    name, width = Y3.GRAPHS[tag]
    batches = []
    for r in range(3):
        lab = seeded_labels(B, nc, seed=10 + r, max_boxes=6, min_boxes=2)
        lab['bboxes'][:, 2:] = lab['bboxes'][:, 2:] * 0.5 + 0.1
        img = seeded_images(B, S, S, seed=20 + r)
        # uint8 images go through the image stem of the direct kernel, which takes cout % 16 == 0: tiny (16) and the full-width graphs (32); at width 0.25
        # layer 0 has 8 output channels and the uint8 form raises (not built), so that graph is fed the fp32 images
        batches.append(dict(img=(img * 255).to(torch.uint8) if tag == 'tiny' else img, **lab))
    res = {}
    for graph in (False, True):
        m = Y3.seed_model_(DetectionModel(Y3.graph_cfg(name, width, nc), verbose=False), int(g[f'{tag}/seed']), float(g[f'{tag}/gain'])).to(DEV)
        tr = DetectionTrainer(m, lr0=0.01, amp=amp, graph=graph, batch_size=64, nb=10, epochs=3)
        losses = [tr.step(b)[0].item() for b in batches]
        res[graph] = (losses, tr.state.data.clone(), tr.state.ema.clone())
        if graph:
            assert len(tr._graphs) == 1
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    assert torch.equal(res[False][1], res[True][1]) and torch.equal(res[False][2], res[True][2])
    assert len(set(res[True][0])) == 3
