"""Test-time augmentation (`model(x, augment=True)`, reference nn/tasks.py:256-287) against the reference-generated fixture tests/golden/tta.npz
(tests/golden/gen_tta.py).  The geometry checks run without a GPU; everything that launches a kernel is marked gpu."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inputs as GI
from mgdt_yolo_amd.models import get_config
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images

DEV = 'cuda:0'
TAGS = list(GI.E2E_MODELS)
TTA_SHAPES = {(2, 160, 224): 10, (1, 192, 160): 5, (1, 640, 480): 50}        # every SUB-th anchor is recorded (gen_tta.py)
NMS_SHAPE = (1, 128, 96)
GEOM_SHAPES = [(1, 640, 640), (1, 640, 480), (1, 160, 224), (2, 160, 224), (1, 192, 160), (1, 128, 96)]
SCALE_CASES = [('f32_083_g32', (1, 40, 72), 0.83, False, 32, False), ('f32_083_g32_flip', (1, 40, 72), 0.83, True, 32, False),
               ('f32_067_g8_odd', (1, 37, 53), 0.67, False, 8, False), ('f32_083_g8_odd_flip', (1, 37, 53), 0.83, True, 8, False),
               ('f32_067_g32_flip', (1, 72, 120), 0.67, True, 32, False), ('u8_083_g8_flip', (2, 45, 31), 0.83, True, 8, True),
               ('u8_067_g32', (1, 64, 80), 0.67, False, 32, True)]
NMS_TTA_CASES = (('pred', dict(conf_thres=0.25, iou_thres=0.7)), ('val', dict(conf_thres=0.001, iou_thres=0.7, multi_label=True)))


def build_model(name, dtype=torch.float32, nc=80, scale='n', device=DEV):
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(get_config(name, scale, nc), verbose=False)
    seed_state_dict_(m, 0)
    m = m.eval().set_compute_dtype(dtype)
    return m.to(device) if device else m


def key(tag, shape):
    return f'{tag}_{shape[0]}x{shape[1]}x{shape[2]}'


# ------------------------------------------------------------------------------------------------ host side (no GPU)
@pytest.mark.parametrize('tag', TAGS)
def test_tta_geometry_matches_the_reference(golden, tag):
    """Per-pass sizes, per-level anchor counts, kept anchor ranges and the merged anchor count of every recorded case; the head levels run are
    exactly those whose anchors the clip keeps (for the one-level head only pass 2 survives)."""
    from mgdt_yolo_amd.nn.tasks import tta_geometry
    g = golden('tta')
    strides = g[f'{tag}_stride'].tolist()
    nl = len(strides)
    for shape in GEOM_SHAPES:
        k = key(tag, shape)
        geo = tta_geometry(shape[1], shape[2], strides)
        assert [list(p['size']) for p in geo['passes']] == g[f'{k}_sizes'].tolist(), k
        assert [p['levels'] for p in geo['passes']] == g[f'{k}_levels'].tolist(), k
        assert [list(p['keep']) for p in geo['passes']] == g[f'{k}_keep'].tolist(), k
        assert geo['anchors'] == int(g[f'{k}_anchors']), k
        run = {(pi, li) for pi, p in enumerate(geo['passes']) for li in p['levels_run']}
        if nl == 1:
            assert run == {(1, 0)}, k
        else:
            assert run == {(pi, li) for pi in range(3) for li in range(nl)} - {(0, nl - 1), (2, 0)}, k
        assert [p['a_off'] for p in geo['passes']] == [0, geo['passes'][0]['keep'][1], geo['passes'][0]['keep'][1] + geo['passes'][1]['anchors']], k


def test_tta_geometry_table_of_the_issue(golden):
    g = golden('tta')
    want = {('yolov8_n', (1, 640, 640)): 15049, ('yolov8_n', (1, 640, 480)): 11411, ('yolov8_n', (1, 160, 224)): 1430,
            ('mspa_c2f_gd_n', (1, 640, 640)): 4489, ('mspa_c2f_gd_n', (1, 640, 480)): 3350, ('mspa_c2f_gd_n', (1, 160, 224)): 408}
    for (tag, shape), n in want.items():
        assert int(g[f'{key(tag, shape)}_anchors']) == n
    assert g['mspa_c2f_gd_n_1x640x640_sizes'].tolist() == [[640, 640], [536, 536], [432, 432]]


def test_tta_geometry_refuses_a_clip_inside_a_level():
    from mgdt_yolo_amd.nn.tasks import tta_geometry
    with pytest.raises(RuntimeError, match='cuts head level'):
        tta_geometry(100, 100, [8, 16, 32])


def test_descale_and_clip_helpers_on_plain_tensors(golden):
    """_descale_pred / _clip_augmented keep the reference's semantics on CPU tensors (code that calls them directly)."""
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    p = torch.arange(2 * 6 * 5, dtype=torch.float32).reshape(2, 6, 5)
    q = DetectionModel._descale_pred(p.clone(), 3, 0.83, (40, 64))
    ref = p.clone()
    ref[:, :4] /= 0.83
    ref[:, 0] = 64 - ref[:, 0]
    assert torch.equal(q, ref)
    g = golden('tta')
    for tag, name in GI.E2E_MODELS.items():
        m = build_model(name, device=None)
        k = key(tag, (1, 640, 480))
        ys = [torch.zeros(1, 84, n) for n in g[f'{k}_levels'].sum(1).tolist()]
        kept = m._clip_augmented(ys)
        assert [t.shape[-1] for t in kept] == [hi - lo for lo, hi in g[f'{k}_keep'].tolist()]


def test_augment_in_training_and_profile_still_raise():
    m = build_model('yolov8', device=None).train()
    with pytest.raises(RuntimeError, match='inference call form'):
        m.predict(torch.zeros(1, 3, 64, 64), augment=True)
    with pytest.raises(RuntimeError, match='profile / visualize'):
        m.eval().predict(torch.zeros(1, 3, 64, 64), profile=True)


# ------------------------------------------------------------------------------------------------ resampling kernel
def _scale_args(h, w, r, gs):
    return int(h * r), int(w * r), math.ceil(h * r / gs) * gs, math.ceil(w * r / gs) * gs


@pytest.mark.gpu
@pytest.mark.parametrize('case', SCALE_CASES, ids=[c[0] for c in SCALE_CASES])
def test_scale_img_kernel_matches_reference(golden, case):
    """fp32 within 1e-6 of the reference's scale_img; uint8 input == the fp32 path on u8 / 255; bf16 output == the RNE-rounded fp32 result
    (or within 1 bf16 ulp of it)."""
    from mgdt_yolo_amd import ops
    g = golden('tta')
    name, (b, h, w), r, flip, gs, u8 = case
    ref = g[f'scale_{name}_y']
    args = _scale_args(h, w, r, gs)
    if u8:
        xu = torch.from_numpy(g[f'scale_{name}_u8']).to(DEV)
        x = (torch.from_numpy(g[f'scale_{name}_u8']).float() / 255).to(DEV)     # the host's correctly rounded division (`img /= 255`)
        yu = ops.scale_img(xu, *args, flip, torch.float32)
    else:
        x = seeded_images(b, h, w, seed=100 + [c[0] for c in SCALE_CASES].index(name)).to(DEV)
    y = ops.scale_img(x, *args, flip, torch.float32)
    assert tuple(y.shape) == ref.shape
    err = np.abs(y.cpu().numpy() - ref).max()
    print(f'scale_img {name}: max |err| {err:.2e}')
    assert err <= 1e-6, err
    if u8:
        assert torch.equal(yu, y)
    yb = ops.scale_img(x, *args, flip, torch.bfloat16)
    rne = y.to(torch.bfloat16)
    ulp = (yb.view(torch.int16).int() - rne.view(torch.int16).int()).abs().max().item()
    assert ulp <= 1, ulp
    # a strided (channels_last) input reads the same pixels
    y2 = ops.scale_img(x.contiguous(memory_format=torch.channels_last), *args, flip, torch.float32)
    assert torch.equal(y2, y)


# ------------------------------------------------------------------------------------------------ whole model
def _tta(m, x):
    with torch.no_grad():
        y, none = m(x, augment=True)
    assert none is None
    return y


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('shape', list(TTA_SHAPES), ids=lambda s: 'x'.join(map(str, s)))
def test_tta_fp32_matches_reference(golden, tag, shape):
    """e2e contract: xywh within 1e-3 px, scores within 1e-4 of the reference's _predict_augment (every SUB-th anchor recorded)."""
    g = golden('tta')
    m = build_model(GI.E2E_MODELS[tag])
    y = _tta(m, seeded_images(*shape, seed=GI.IMG_SEED).to(DEV))
    k = key(tag, shape)
    assert y.shape[-1] == int(g[f'{k}_anchors'])
    ref = g[f'{k}_ysub']
    ys = y.cpu().numpy()[:, :, ::TTA_SHAPES[shape]]
    eb, ec = np.abs(ys[:, :4] - ref[:, :4]).max(), np.abs(ys[:, 4:] - ref[:, 4:]).max()
    print(f'tta fp32 {k}: max box err {eb:.2e} px, max conf err {ec:.2e}')
    assert eb < 1e-3 and ec < 1e-4, (eb, ec)


# bf16 vs the fp32 reference: the plain forward's stated tolerances (test_hip_parity.BF16_TOL / BF16_TOL_640), boxes widened by 1 / 0.67 - the
# de-scaling of the smallest pass multiplies a box error in its own pixels by that much
BF16_TOL = {'mspa_c2f_gd_n': (1.4, 0.07), 'yolov8_n': (0.5, 0.008)}
BF16_TOL_640 = {'mspa_c2f_gd_n': (1.7, 0.10), 'yolov8_n': (1.1, 0.015)}


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('shape', list(TTA_SHAPES), ids=lambda s: 'x'.join(map(str, s)))
def test_tta_bf16_within_stated_tolerance(golden, tag, shape):
    g = golden('tta')
    m = build_model(GI.E2E_MODELS[tag], torch.bfloat16)
    y = _tta(m, seeded_images(*shape, seed=GI.IMG_SEED).to(DEV).to(torch.bfloat16))
    k = key(tag, shape)
    ref = g[f'{k}_ysub']
    ys = y.cpu().numpy()[:, :, ::TTA_SHAPES[shape]]
    tb, tc = (BF16_TOL_640 if shape[1] >= 640 else BF16_TOL)[tag]
    eb, ec = np.abs(ys[:, :4] - ref[:, :4]).max(), np.abs(ys[:, 4:] - ref[:, 4:]).max()
    print(f'tta bf16 {k}: max box err {eb:.4f} px, max conf err {ec:.4f}')
    assert eb < tb / 0.67 and ec < tc, (eb, ec)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
def test_tta_nms_matches_fixture_and_keys(golden, tag):
    """NMS kept rows on the reference's augmented output == the fixture (bit-exact, predictor and validator settings); on the product's own
    augmented output (fp32: decode route, bf16: Detect tail route) the best-class keys the epilogues wrote give the same rows as the score scan."""
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.yolo.utils.ops import non_max_suppression, nms_with_index
    g = golden('tta')
    k = key(tag, NMS_SHAPE)
    yref = torch.from_numpy(g[f'{k}_y']).to(DEV)
    for cname, kw in NMS_TTA_CASES:
        out = non_max_suppression((yref, None), **kw)
        for i, o in enumerate(out):
            ref = g[f'{k}_nms_{cname}_{i}']
            assert tuple(o.shape) == ref.shape and np.array_equal(o.cpu().numpy(), ref), (cname, i)
    for dt in (torch.float32, torch.bfloat16):
        m = build_model(GI.E2E_MODELS[tag], dt)
        y = _tta(m, seeded_images(2, 160, 224, seed=5).to(DEV).to(dt))
        assert ops._best_keys_of(y, 2, y.shape[2]) is not None
        for kw in (dict(conf_thres=0.25, iou_thres=0.7), dict(conf_thres=0.3, iou_thres=0.6, agnostic=True, max_det=50)):
            rows, kept = nms_with_index(y, **kw)
            ops.NMS_USE_BEST_KEYS = False
            try:
                rows2, kept2 = nms_with_index(y, **kw)
            finally:
                ops.NMS_USE_BEST_KEYS = True
            for i in range(2):
                assert torch.equal(rows[i], rows2[i]) and torch.equal(kept[i], kept2[i]), (dt, kw)


def _ref_scale_img(x, r, flip, gs):
    """yolo/utils/torch_utils.py:261-270 restated (CPU, fp32)."""
    x = x.flip(3) if flip else x
    if r == 1:
        return x
    h, w = x.shape[2:]
    s = (int(h * r), int(w * r))
    x = F.interpolate(x, size=s, mode='bilinear', align_corners=False)
    hp, wp = (math.ceil(v * r / gs) * gs for v in (h, w))
    return F.pad(x, [0, wp - s[1], 0, hp - s[0]], value=0.447)


def _compose(ys, x_shape, nl):
    """_descale_pred + _clip_augmented restated over the three passes' plain outputs."""
    out = []
    for y, r, flip in zip(ys, (1, 0.83, 0.67), (False, True, False)):
        y = y.clone()
        y[:, :4] /= r
        if flip:
            y[:, 0] = x_shape[3] - y[:, 0]
        out.append(y)
    g = sum(4 ** i for i in range(nl))
    i = out[0].shape[-1] // g
    out[0] = out[0][..., :-i]
    i = (out[-1].shape[-1] // g) * 4 ** (nl - 1)
    out[-1] = out[-1][..., i:]
    return torch.cat(out, -1)


@pytest.mark.gpu
def test_tta_tood_matches_composed_single_passes():
    """TOODHead (parity unpinned, as elsewhere): the augmented output vs a composition of oracle.layers.model_forward at the three scaled inputs
    (scores within 1e-3, as test_tood_model_e2e_fp32_matches_oracle states) and vs the product's own plain forwards at the kernel-resampled inputs
    (boxes within 1e-3 px - torch divides by the scale as a reciprocal multiply -, scores identical)."""
    from oracle import layers as OL
    cfg = get_config('mspa_c2f_gd_tood_yolov8', 'n', 80)
    m = build_model('mspa_c2f_gd_tood_yolov8')
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    x = seeded_images(1, 160, 192, seed=3)
    y = _tta(m, x.to(DEV)).cpu()
    xs = [_ref_scale_img(x, r, f, 8) for r, f in zip((1, 0.83, 0.67), (False, True, False))]
    y_or = _compose([OL.model_forward(cfg, sd, xi, [8.0])[0] for xi in xs], x.shape, 1)
    from mgdt_yolo_amd import ops
    xd = x.to(DEV)
    xs_own = [xd, ops.scale_img(xd, *_scale_args(160, 192, 0.83, 8), True, torch.float32), ops.scale_img(xd, *_scale_args(160, 192, 0.67, 8), False, torch.float32)]
    with torch.no_grad():
        y_own = _compose([m(xi)[0].cpu() for xi in xs_own], x.shape, 1)
    assert y.shape == y_or.shape == y_own.shape
    print('tood tta: vs oracle conf', (y[:, 4:] - y_or[:, 4:]).abs().max().item(), 'vs own passes box', (y[:, :4] - y_own[:, :4]).abs().max().item())
    np.testing.assert_allclose(y[:, 4:].numpy(), y_or[:, 4:].numpy(), atol=1e-3)
    assert (y[:, :4] - y_own[:, :4]).abs().max().item() < 1e-3 and torch.equal(y[:, 4:], y_own[:, 4:])


def _names(m, x, **kw):
    from mgdt_yolo_amd import ops
    names = []
    orig = ops._launch
    with torch.no_grad():
        m(x, **kw)                                   # panels are packed on first use
        ops._launch = lambda name, *a, **k: (names.append(name), orig(name, *a, **k))[1]
        try:
            out = m(x, **kw)
        finally:
            ops._launch = orig
    return names, out


@pytest.mark.gpu
def test_tta_launches():
    """nl = 1: one resample + exactly the launches of one plain forward at 536^2 (tail / decode through their augment entry points).  nl = 3: two
    resamples and no tail launch for the clipped levels (pass 1 runs levels 0-1, pass 2 all three, pass 3 levels 1-2)."""
    from mgdt_yolo_amd import ops
    m = build_model('mspa_c2f_gd_yolov8', torch.bfloat16)
    x = seeded_images(1, 640, 640, seed=GI.IMG_SEED).to(DEV).to(torch.bfloat16)
    n_aug, _ = _names(m, x, augment=True)
    x536 = ops.scale_img(x, 531, 531, 536, 536, True, torch.bfloat16)
    n_plain, _ = _names(m, x536)
    assert n_aug[0] == 'scale_img_fwd' and n_aug.count('scale_img_fwd') == 1
    assert [n.replace('_aug_fwd', '_fwd') for n in n_aug[1:]] == n_plain, (len(n_aug), len(n_plain))
    m3 = build_model('yolov8', torch.bfloat16)
    n3, _ = _names(m3, x, augment=True)
    assert n3.count('scale_img_fwd') == 2 and n3.count('detect_tail_aug_fwd') == 7 and 'detect_tail_fwd' not in n3, n3.count('detect_tail_aug_fwd')
    n3p, _ = _names(m3, x)
    assert n3p.count('detect_tail_fwd') == 3


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mspa_c2f_gd_yolov8', 'yolov8'])
def test_tta_graph_replay_and_fuse_are_bit_equal(name):
    """The augmented forward captures into one graph and replays bit-equal to eager (new inputs copied in); after fuse() the output equals the
    unfused model's."""
    m = build_model(name, torch.bfloat16)
    xs = [seeded_images(2, 160, 224, seed=s).to(DEV).to(torch.bfloat16) for s in (1, 2)]
    ref = [_tta(m, x).clone() for x in xs]
    xin = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        m(xin, augment=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out, _ = m(xin, augment=True)
    for x, r in zip(xs[::-1], ref[::-1]):
        xin.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, r)
    del g
    yf = _tta(m.fuse(), xs[0])
    d = (yf - ref[0]).abs().max().item()
    print(f'{name}: fused vs unfused augmented output max |d| {d:.3e}')
    assert torch.equal(yf, ref[0]), d


@pytest.mark.gpu
def test_tta_predictor_and_validator_end_to_end():
    """BasePredictor(augment=True) -> AutoBackend.forward(augment=True) -> the model's (y, None) -> NMS; the validator's postprocess takes the tuple."""
    from mgdt_yolo_amd.yolo.engine.predictor import DetectionPredictor
    from mgdt_yolo_amd.yolo.utils.ops import non_max_suppression
    from mgdt_yolo_amd.yolo.v8.detect.val import DetectionValidator
    m = build_model('mspa_c2f_gd_yolov8')
    r = np.random.default_rng(11)
    imgs = [r.integers(0, 256, (120, 200, 3), dtype=np.uint8) for _ in range(2)]
    for half in (False, True):
        p = DetectionPredictor(dict(imgsz=160, augment=True, half=half, conf=0.05))
        p.setup_model(m)
        res = p(imgs)
        im = p.preprocess(imgs)
        with torch.no_grad():
            y, none = p.model(im, augment=True)
        assert none is None
        direct = non_max_suppression(y, 0.05, 0.7)
        assert len(res) == 2 and all(a.shape == b.shape for a, b in zip(res, direct)) and sum(len(a) for a in res) > 0
        v = DetectionValidator()
        v.init_metrics()
        a, b = v.postprocess((y, None)), v.postprocess(y)
        assert all(torch.equal(s, t) for s, t in zip(a, b))
        assert p.args.augment and DetectionPredictor().args.augment is False


@pytest.mark.gpu
def test_tta_refuses_the_fp8_model():
    """fp8 (quantize_fp8) is not validated for augmented inference: a clear error, never a silent route."""
    m = build_model('mspa_c2f_gd_yolov8', torch.bfloat16)
    x = seeded_images(1, 160, 160, seed=3).to(DEV).to(torch.bfloat16)
    m.quantize_fp8(x)
    with pytest.raises(RuntimeError, match='fp8'):
        m(x, augment=True)
    m.dequantize_fp8()
    assert _tta(m, x).shape[-1] == 17 * 17
