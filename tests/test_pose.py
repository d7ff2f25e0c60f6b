"""Pose-estimation inference (Pose head, keypoint decode, NMS with keypoint columns, post-NMS scaling, PosePredictor) against the
reference-generated fixtures tests/golden/pose_NN.npz (tests/golden/gen_pose.py; merged by pose_ref.load_fixture).  Host-side checks run without a
GPU; everything that launches a kernel is marked gpu.

Tolerances.  fp32: boxes 1e-3 px and confidences 1e-4 (the project contract); keypoint x / y max(1e-3 px, 4 x the fixture's fp32-vs-fp64 difference),
visibility max(1e-4, 4 x its difference) - the factor 4 covers the MFMA's accumulation order against the CPU's; raw keypoints with the feature-map
tolerance of the segmentation tests (atol 1e-3, rtol 1e-4).  bf16: 3 x the fixture's bf16-emulation difference per quantity (accumulation order,
and the BatchNorm fold rounded once in the panel instead of per layer); the generator asserts that this bound stays below 4 px (half the smallest
stride) for keypoints, so a wrong anchor offset or stride fails.  Printed by the generator (this fixture set): fp32-vs-fp64 keypoint differences
8.9e-6 .. 3.8e-5 px (bound 1e-3 px everywhere), visibility <= 5.4e-7 (bound 1e-4); bf16 keypoint bounds 0.39 - 0.42 px (yolov8-pose), 1.55 px (MSPA-GD).
Measured on the MI355X (first run): fp32 keypoints <= 4.2e-5 px, visibility <= 6.0e-7, raw keypoints <= 2.6e-6; bf16 keypoints 0.10 - 0.15 px (yolov8-pose),
0.36 px (MSPA-GD); pose_concat 0 ulp from the restatement in every case.  The weights are pose_ref.seed_pose_ (seeded, the keypoint branch's closing 1x1 scaled so that raw keypoints stay O(1))."""
import os
import re

import numpy as np
import pytest
import torch

import pose_ref as PR
from mgdt_yolo_amd import _lib
from mgdt_yolo_amd.models import get_config
from mgdt_yolo_amd.seeding import seeded_images

DEV = 'cuda:0'
_FIX = []


def fixture():
    if not _FIX:
        _FIX.append(PR.load_fixture())
    return _FIX[0]


def build_model(name, kpt_shape=(17, 3), dtype=torch.float32, device=DEV, scale='n'):
    from mgdt_yolo_amd.nn.tasks import PoseModel
    m = PoseModel(get_config(name, scale), data_kpt_shape=kpt_shape, verbose=False)
    PR.seed_pose_(m, 0)
    m = m.eval().set_compute_dtype(dtype)
    return m.to(device) if device else m


def fp32_bounds(g, tag):
    d = dict(zip(PR.QUANTITIES, g[f'{tag}_d64'].tolist()))
    return {'box': 1e-3, 'conf': 1e-4, 'kxy': max(1e-3, 4 * d['kxy']), 'kvis': max(1e-4, 4 * d['kvis'])}


def bf16_bounds(g, tag):
    b = {q: 3 * v for q, v in zip(PR.QUANTITIES, g[f'{tag}_dbf16'].tolist())}
    assert b['kxy'] < 4.0, b
    return b


def check_within(what, got, ref, kpt_shape, bounds):
    d = PR.max_diffs(got, ref, 1, kpt_shape)
    print(f'{what}: ' + '  '.join(f'{q} {d[q]:.3e} (bound {bounds[q]:.3e})' for q in PR.QUANTITIES))
    for q in PR.QUANTITIES:
        assert d[q] <= bounds[q], (what, q, d[q], bounds[q])
    return d


# ------------------------------------------------------------------------------------------------ host side (no GPU)
def test_new_entry_points_are_declared_bound_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'mgdt.h')).read()
    declared = set(re.findall(r'\b(mgdt_[a-z0-9_]+)\s*\(', hdr))
    lib = _lib.lib()
    for name in ('mgdt_pose_concat_fwd', 'mgdt_pose_scale_fwd'):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    # null arguments are refused before any GPU call
    assert lib.mgdt_pose_concat_fwd(None, 1, 5, 1, None, None, 1, 51, 3, None, None, 0, None) == -4
    assert lib.mgdt_pose_scale_fwd(None, None, None, 1, 1, 6, 51, 3, None) == -4


def test_pose_config_equals_the_reference_yaml():
    import json
    from mgdt_yolo_amd.models import CONFIGS, POSE_CONFIGS, SEG_CONFIGS
    ref = json.load(open(os.path.join(PR.GOLDEN, 'pose_yaml.json')))
    cfg = get_config('yolov8-pose')
    for k in ('nc', 'kpt_shape', 'scales', 'backbone', 'head'):
        assert cfg[k] == ref[k], k
    assert set(POSE_CONFIGS) == {'yolov8-pose', 'mspa_c2f_gd_yolov8-pose'} and not set(POSE_CONFIGS) & (set(CONFIGS) | set(SEG_CONFIGS))
    one = get_config('mspa_c2f_gd_yolov8-pose')
    assert one['head'][-1] == [[15], 1, 'Pose', ['nc', 'kpt_shape']] and one['head'][:-1] == get_config('mspa_c2f_gd_yolov8')['head'][:-1]


@pytest.mark.parametrize('tag,name,scale,kpt', [('yolov8_pose_n', 'yolov8-pose', 'n', (17, 3)), ('yolov8_pose_s', 'yolov8-pose', 's', (17, 3)),
                                                ('mspa_c2f_gd_pose_n', 'mspa_c2f_gd_yolov8-pose', 'n', (17, 3)),
                                                ('yolov8_pose_k5x2_n', 'yolov8-pose', 'n', (5, 2))])
def test_pose_model_structure_matches_the_reference(tag, name, scale, kpt):
    g = fixture()
    m = build_model(name, kpt, device=None, scale=scale)
    sd = m.state_dict()
    assert list(sd.keys()) == g[f'{tag}_keys'].tolist()
    assert [','.join(map(str, v.shape)) for v in sd.values()] == g[f'{tag}_shapes'].tolist()
    assert sum(p.numel() for p in m.parameters()) == int(g[f'{tag}_nparams'])
    assert m.stride.tolist() == g[f'{tag}_stride'].tolist()
    head = m.model[-1]
    assert tuple(head.kpt_shape) == kpt and head.nk == kpt[0] * kpt[1] and tuple(m.kpt_shape) == kpt
    assert head.cv4[0][0].conv.out_channels == max(head.cv2[0][0].conv.in_channels // 4, head.nk)


def test_guess_model_task_and_model_class():
    from mgdt_yolo_amd.nn.tasks import DetectionModel, PoseModel, SegmentationModel, guess_model_task, model_class_of
    m = build_model('yolov8-pose', device=None)
    assert guess_model_task(m) == 'pose' and guess_model_task(m.yaml) == 'pose' and guess_model_task('yolov8n-pose.yaml') == 'pose'
    assert guess_model_task(get_config('yolov8-seg', 'n', 80)) == 'segment' and guess_model_task('yolov8n-seg.yaml') == 'segment'
    assert guess_model_task(get_config('yolov8', 'n', 80)) == 'detect' and guess_model_task('yolov8n.yaml') == 'detect'
    assert guess_model_task(get_config('mspa_c2f_gd_yolov8', 'n', 80)) == 'detect'
    assert model_class_of(m.yaml) is PoseModel and model_class_of(get_config('yolov8-seg')) is SegmentationModel
    assert model_class_of(get_config('yolov8')) is DetectionModel
    by_name = PoseModel('yolov8n-pose.yaml', verbose=False)
    assert by_name.stride.tolist() == [8.0, 16.0, 32.0] and by_name.yaml['scale'] == 'n' and by_name.yaml['nc'] == 1


def test_pose_training_and_augment_raise_clear_errors():
    m = build_model('yolov8-pose', device=None)
    with pytest.raises(NotImplementedError, match='pose training is not built'):
        m.init_criterion()
    with pytest.raises(NotImplementedError, match='pose training is not built'):
        m.model[-1].train()([torch.zeros(1, 64, 8, 8)] * 3)
    with pytest.raises(NotImplementedError, match='pose training is not built'):
        m.model[-1].backward([])
    m.eval()
    with pytest.raises(RuntimeError, match='augment=True is not built for PoseModel'):
        m(torch.zeros(1, 3, 64, 64), augment=True)


@pytest.mark.parametrize('fused', [False, True], ids=['unfused', 'fused'])
def test_padded_panels_are_zero_outside_the_real_channels(fused):
    """The tensors handed to PackedConv on the padded route (CPU tensors here): real block unchanged, everything else zero, and the padded output
    channels fold to scale * 0 and shift 0."""
    from mgdt_yolo_amd.nn.modules.head import padded_conv_params
    m = build_model('yolov8-pose', device=None)
    if fused:
        m.fuse()
    head = m.model[-1]
    for seq in head.cv4:
        c0, c1, c2 = seq
        cin = c0.conv.in_channels
        assert c2.in_channels == 51 and hasattr(c0, 'bn') != fused
        for mod, cin_r, cin_p, cout_r, cout_p in ((c0, cin, cin, 51, 56), (c1, 51, 56, 51, 56), (c2, 51, 56, 51, 52)):
            w, cb, bn = padded_conv_params(mod, cin_p, cout_p)
            conv = getattr(mod, 'conv', mod)
            assert tuple(w.shape[:2]) == (cout_p, cin_p) and torch.equal(w[:cout_r, :cin_r], conv.weight.detach())
            assert not w[cout_r:].any() and not w[:, cin_r:].any()
            if conv.bias is not None:
                assert torch.equal(cb[:cout_r], conv.bias.detach()) and not cb[cout_r:].any() and cb.shape == (cout_p,)
            else:
                assert cb is None
            if bn is None:
                assert fused or mod is c2
            else:
                gam, beta, mean, var, eps = bn
                assert all(t.shape == (cout_p,) for t in (gam, beta, mean, var)) and eps == mod.bn.eps
                assert torch.equal(gam[:cout_r], mod.bn.weight.detach()) and torch.equal(var[:cout_r], mod.bn.running_var)
                scale = gam / torch.sqrt(var + eps)
                shift = beta - mean * scale
                assert not (w * scale.view(-1, 1, 1, 1))[cout_r:].any() and not shift[cout_r:].any()
    w, _, _ = padded_conv_params(head.cv4[0][0], head.cv4[0][0].conv.in_channels, 51)         # nothing to pad: the parameters themselves
    assert torch.equal(w, head.cv4[0][0].conv.weight.detach())
    with pytest.raises(RuntimeError, match='cannot pad'):
        padded_conv_params(head.cv4[0][0], 8, 56)


def test_scale_helpers_check_arguments_before_any_launch():
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.yolo.utils import ops as yops
    with pytest.raises(RuntimeError, match='CPU tensor'):
        yops.scale_coords((160, 224), torch.zeros(3, 17, 3), (120, 200))
    with pytest.raises(RuntimeError, match='CPU tensor'):
        yops.clip_coords(torch.zeros(3, 2), (120, 200))
    gain = min(160 / 120, 224 / 200)
    assert ops.pose_scale_meta((160, 224), (120, 200)) == [gain, (224 - 200 * gain) / 2, (160 - 120 * gain) / 2, 120.0, 200.0, 0.0, 13.0, 0.0]
    assert ops.pose_scale_meta((160, 224), (134, 224))[:3] == [1.0, 0.0, 13.0] and ops.POSE_PAD_MFMA is True


# ------------------------------------------------------------------------------------------------ whole model
def _kpt_direct(prof, head):
    """Launches of mgdt_conv2d_direct_fwd in the log whose (cin, cout, k) is one of the keypoint branch's convolutions.  (With nc = 1 the closing 1x1
    convolutions of the box and class branches write 16 + 1 channels into one 17-channel map and take the direct kernel in Detect.forward in fp32,
    as does the 3-channel stem; this feature leaves those as they are.)"""
    sigs = set()
    for c0, c1, c2 in head.cv4:
        sigs |= {(c0.conv.in_channels, c0.conv.out_channels, 3), (c1.conv.in_channels, c1.conv.out_channels, 3), (c2.in_channels, c2.out_channels, 1)}
    return sum(1 for name, meta, _ in prof.rows if name == 'conv2d_direct_fwd' and (meta['shape'][1], meta['shape'][4], meta['shape'][5]) in sigs)


def _run(m, shape, dtype=torch.float32):
    with torch.no_grad():
        return m(seeded_images(*shape, seed=PR.IMG_SEED).to(DEV).to(dtype))


@pytest.mark.gpu
@pytest.mark.parametrize('tag', list(PR.CASES))
def test_pose_model_fp32_matches_reference(tag):
    """Per-quantity fp32 bounds (module docstring) against the whole recorded tensors; return structure of the reference (head.py:236)."""
    from mgdt_yolo_amd import ops
    g = fixture()
    name, kpt_shape, shape = PR.CASES[tag]
    m = build_model(name, kpt_shape)
    nk = kpt_shape[0] * kpt_shape[1]
    with ops.profile() as p:
        cat, (feats, kpt) = _run(m, shape)
    ref = g[f'{tag}_pred']
    assert tuple(cat.shape) == ref.shape and cat.dtype == torch.float32 and tuple(kpt.shape) == (shape[0], nk, ref.shape[2]) and len(feats) == len(m.stride)
    assert [list(f.shape[2:]) for f in feats] == g[f'{tag}_levels'].tolist()
    print(f'{tag}: recorded fp32-vs-fp64 differences ' + '  '.join(f'{q} {v:.3e}' for q, v in zip(PR.QUANTITIES, g[f"{tag}_d64"])))
    check_within(f'pose fp32 {tag}', cat.cpu().numpy(), ref, kpt_shape, fp32_bounds(g, tag))
    ek = np.abs(kpt.cpu().numpy() - g[f'{tag}_kpt']).max()
    print(f'pose fp32 {tag}: raw kpt max |err| {ek:.3e}')
    np.testing.assert_allclose(kpt.cpu().numpy(), g[f'{tag}_kpt'], atol=1e-3, rtol=1e-4)
    names = [r[0] for r in p.rows]
    assert names.count('pose_concat_fwd') == 1 and _kpt_direct(p, m.model[-1]) == 0, names
    m.model[-1].export = True
    out = _run(m, shape)
    assert isinstance(out, torch.Tensor) and torch.equal(out, cat)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', list(PR.CASES))
def test_pose_model_bf16_within_three_times_the_emulation(tag):
    from mgdt_yolo_amd import ops
    g = fixture()
    name, kpt_shape, shape = PR.CASES[tag]
    m = build_model(name, kpt_shape, torch.bfloat16)
    with ops.profile() as p:
        cat, (_, kpt) = _run(m, shape, torch.bfloat16)
    print(f'{tag}: recorded bf16-emulation differences ' + '  '.join(f'{q} {v:.3e}' for q, v in zip(PR.QUANTITIES, g[f"{tag}_dbf16"])))
    check_within(f'pose bf16 {tag}', cat.cpu().numpy(), g[f'{tag}_pred'], kpt_shape, bf16_bounds(g, tag))
    assert _kpt_direct(p, m.model[-1]) == 0
    catf, (_, kptf) = _run(m.fuse(), shape, torch.bfloat16)
    assert torch.equal(cat, catf) and torch.equal(kpt, kptf)                   # fuse() changes no bit


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['yolov8-pose', 'mspa_c2f_gd_yolov8-pose'])
def test_padded_mfma_switch(name):
    """Switch off: the keypoint branch goes through mgdt_conv2d_direct_fwd (the log shows it) and the fp32 output agrees with the padded-MFMA route
    within the fp32 bounds; switch on: no direct launch in fp32 or bf16.  kpt_shape (5, 2): c4 = 16 needs no padding; only the closing 1x1 (10
    outputs) differs between the two settings."""
    from mgdt_yolo_amd import ops
    g = fixture()
    tag = [t for t, c in PR.CASES.items() if c[0] == name and c[1] == (17, 3)][0]
    shape = PR.CASES[tag][2]
    outs = {}
    for dt in (torch.float32, torch.bfloat16):
        m = build_model(name, (17, 3), dt)
        for on in (True, False):
            ops.POSE_PAD_MFMA = on
            try:
                with ops.profile() as p:
                    outs[dt, on] = _run(m, shape, dt)[0]
            finally:
                ops.POSE_PAD_MFMA = True
            n_direct = _kpt_direct(p, m.model[-1])
            assert n_direct == (0 if on else 3 * len(m.stride)), (dt, on, n_direct)
    check_within(f'switch {name} fp32 on vs off', outs[torch.float32, True].cpu().numpy(), outs[torch.float32, False].cpu().numpy(), (17, 3), fp32_bounds(g, tag))
    check_within(f'switch {name} bf16 off vs fixture', outs[torch.bfloat16, False].cpu().numpy(), g[f'{tag}_pred'], (17, 3), bf16_bounds(g, tag))
    if name == 'yolov8-pose':
        m = build_model(name, (5, 2))
        for on in (True, False):
            ops.POSE_PAD_MFMA = on
            try:
                with ops.profile() as p:
                    outs[on] = _run(m, shape)[0]
            finally:
                ops.POSE_PAD_MFMA = True
            # c4 = 16 fits the MFMA kernel either way; the closing 1x1 (16 -> 10 outputs) is padded to 12 with the switch on and direct with it off
            assert _kpt_direct(p, m.model[-1]) == (0 if on else len(m.stride)), on
        k52 = 'yolov8_pose_k5x2_n_2x96x160'
        check_within('switch (5, 2) fp32 on vs off', outs[True].cpu().numpy(), outs[False].cpu().numpy(), (5, 2), fp32_bounds(g, k52))


@pytest.mark.gpu
def test_pose_forward_capture_replays_bit_equal():
    m = build_model('yolov8-pose', (17, 3), torch.bfloat16)
    xs = [seeded_images(2, 96, 160, seed=s).to(DEV).to(torch.bfloat16) for s in (1, 2)]
    with torch.no_grad():
        ref = [tuple(t.clone() for t in (lambda o: (o[0], o[1][1]))(m(x))) for x in xs]
    xin = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        m(xin)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        cat, (_, kpt) = m(xin)
    for x, r in zip(xs[::-1], ref[::-1]):
        xin.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cat, r[0]) and torch.equal(kpt, r[1])
    del graph


# ------------------------------------------------------------------------------------------------ kernels alone
@pytest.mark.gpu
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kpt_shape,cs', [((17, 3), 51), ((17, 3), 52), ((5, 2), 10), ((5, 2), 12), ((4, 3), 12), ((6, 2), 16)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else f'cs{v}')
def test_pose_concat_matches_the_decode_restatement(kpt_shape, cs, dt):
    """Levels 12x20 (stride 8) and 3x5 (stride 32), 255 anchors = three full 64-anchor tiles and a tail, one tile across the level border; channel
    stride == nk (scalar loads when nk % 4, 4-channel pieces for nk = 12) and > nk (the padded buffers).  Copied rows and the raw map exact, the
    decoded rows within 1 ulp of the float32 restatement."""
    from mgdt_yolo_amd import ops
    nk, nd = kpt_shape[0] * kpt_shape[1], kpt_shape[1]
    levels, strides, b = [(12, 20), (3, 5)], [8.0, 32.0], 2
    r = np.random.default_rng([5, nk, cs])
    y = torch.from_numpy(r.standard_normal((b, 5, 255), dtype=np.float32)).to(DEV)
    bufs = [torch.from_numpy((2 * r.standard_normal((b, cs, h, w))).astype(np.float32)).to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
            for h, w in levels]
    raw = torch.cat([t[:, :nk].float().reshape(b, nk, -1) for t in bufs], 2)
    want = PR.kpts_decode(raw, levels, strides, nd).cpu().numpy()
    for kps in ([t[:, :nk] for t in bufs], bufs):                # channel-slice views and the whole (wider) buffers
        out, kraw = ops.pose_concat(y, kps, strides, nk, nd)
        assert tuple(out.shape) == (b, 5 + nk, 255) and torch.equal(out[:, :5], y) and torch.equal(kraw, raw)
        got = out[:, 5:].cpu().numpy()
        ulp = np.abs(got - want) / np.spacing(np.abs(want).astype(np.float32))
        print(f'pose_concat {kpt_shape} cs {cs} {dt}: worst {ulp.max():.2f} ulp')
        assert ulp.max() <= 1.0, ulp.max()
    with pytest.raises(RuntimeError, match='anchors'):
        ops.pose_concat(y[:, :, :200].contiguous(), bufs, strides, nk, nd)


@pytest.mark.gpu
def test_nms_on_a_pose_prediction_matches_fixture_rows():
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.yolo.utils.ops import non_max_suppression
    g = fixture()
    pred = torch.from_numpy(g[f'{PR.FULL}_pred']).to(DEV)
    for cname in PR.NMS_CASES:
        kw = PR.settings(g, f'{PR.FULL}_nms_{cname}_kw')
        with ops.profile() as p:
            out = non_max_suppression(pred, nc=1, **kw)
        assert [r[0] for r in p.rows] == ['nms_masks_fwd']
        for i, o in enumerate(out):
            ref = g[f'{PR.FULL}_nms_{cname}_{i}']
            assert tuple(o.shape) == ref.shape and o.shape[1] == 57, (cname, i, tuple(o.shape), ref.shape)
            assert np.array_equal(o.cpu().numpy(), ref), (cname, i)
        if cname == 'few':
            assert all(0 < len(o) < kw['max_det'] for o in out)


@pytest.mark.gpu
def test_pose_scale_and_scale_coords_match_the_reference():
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.yolo.utils import ops as yops
    g = fixture()
    for name, oshape in PR.COORD_CASES.items():
        c0 = PR.seeded_coords(name)
        ref = g[f'coords_{name}']
        c = torch.from_numpy(c0).to(DEV)
        out = yops.scale_coords(PR.IN_SHAPE, c, oshape)
        assert out is c                                           # in place, like the reference
        got = c.cpu().numpy()
        e = np.abs(got[..., :2] - ref[..., :2]).max()
        print(f'scale_coords {name}: max |err| {e:.2e} px')
        assert e <= 1e-4 and np.array_equal(got[..., 2], c0[..., 2])
        for ax, lim in ((0, oshape[1]), (1, oshape[0])):          # what the reference clamped lands exactly on the border
            for border in (0.0, float(lim)):
                hit = ref[..., ax] == border
                assert hit.any() and np.all(got[..., ax][hit] == border)
        cn = yops.scale_coords(PR.IN_SHAPE, torch.from_numpy(c0).to(DEV), oshape, normalize=True).cpu().numpy()
        assert np.abs(cn[..., :2] - g[f'coords_{name}_norm'][..., :2]).max() <= 1e-6
        xy = torch.from_numpy(c0[..., :2].copy()).to(DEV)         # (n, k, 2) coordinates and clip_coords alone
        yops.clip_coords(xy, oshape)
        assert torch.equal(xy, torch.from_numpy(c0[..., :2].copy()).to(DEV).clamp_(min=0).minimum(torch.tensor([float(oshape[1]), float(oshape[0])], device=DEV)))
    # the batched launch on NMS rows: image 1 has no detection, rows past the counts keep their bytes
    args = PR.settings(g, 'predictor_args')
    per = [g['lb_0_preround'], g['lb_1_preround']]
    n0 = len(per[0])
    rows = torch.full((3, n0 + 3, 57), -7.0)
    k0 = PR.seeded_coords('rows', n0)
    rows[0, :n0, :4] = torch.from_numpy(per[0]) + torch.tensor([0.0, 13.0, 0.0, 13.0])          # back into the letter-boxed frame
    rows[0, :n0, 4:6] = torch.tensor([0.5, 0.0])
    rows[0, :n0, 6:] = torch.from_numpy(k0).reshape(n0, 51)
    rows[2] = rows[0]
    before = rows.clone()
    counts = torch.tensor([n0, 0, 5], dtype=torch.int32)
    meta = torch.tensor([ops.pose_scale_meta(PR.IN_SHAPE, PR.LB_SHAPE)] * 3, dtype=torch.float32)
    dev = rows.to(DEV)
    with ops.profile() as p:
        ops.pose_scale(dev, counts.to(DEV), meta.to(DEV), 51, 3)
    assert [r[0] for r in p.rows] == ['pose_scale_fwd']
    got = dev.cpu()
    assert torch.equal(got[1], before[1]) and torch.equal(got[2, 5:], before[2, 5:]) and torch.equal(got[0, n0:], before[0, n0:])
    assert np.array_equal(got[0, :n0, :4].numpy(), g['lb_0_boxes'][:, :4]) and torch.equal(got[0, :n0, 4:6], before[0, :n0, 4:6])
    want = k0.copy()
    want[..., 0] = np.clip(want[..., 0], 0, PR.LB_SHAPE[1])
    want[..., 1] = np.clip(want[..., 1] - np.float32(13.0), 0, PR.LB_SHAPE[0])
    assert np.array_equal(got[0, :n0, 6:].numpy().reshape(n0, 17, 3), want) and torch.equal(got[2, :5], got[0, :5])
    assert args['max_det'] >= n0


# ------------------------------------------------------------------------------------------------ predictor
@pytest.mark.gpu
def test_pose_predictor_end_to_end_fp32():
    """PosePredictor in fp32 on the letter-boxed list of two 134x224 images: the reference chain's row counts; boxes equal after rounding except
    the rows the generator lists as within 1e-3 px of a .5 boundary (at most 2 %); scores within 1e-4; keypoints within the fp32 bounds divided by
    the gain (1 here); one NMS launch, one pose_scale launch.  An image list that yields no detection at all is handled."""
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.yolo.v8.pose import PosePredictor
    g = fixture()
    args = PR.settings(g, 'predictor_args')
    m = build_model('yolov8-pose')
    p = PosePredictor(dict(imgsz=(160, 224), **args))
    assert p.args.task == 'pose'
    p.setup_model(m)
    imgs = PR.lb_images()
    p(imgs)                                                   # panels packed
    with ops.profile() as prof:
        res = p(imgs)
    names = [r[0] for r in prof.rows]
    assert names.count('nms_masks_fwd') == 1 and names.count('pose_scale_fwd') == 1 and names[-2:] == ['nms_masks_fwd', 'pose_scale_fwd']
    b = fp32_bounds(g, PR.FULL)
    gain = ops.pose_scale_meta(PR.IN_SHAPE, PR.LB_SHAPE)[0]
    total = risky_total = 0
    for i, (boxes, kpts) in enumerate(res):
        rb, rk, risky = g[f'lb_{i}_boxes'], g[f'lb_{i}_kpts'], g[f'lb_{i}_risky']
        assert tuple(boxes.shape) == rb.shape and tuple(kpts.shape) == rk.shape == (len(rb), 17, 3), (i, tuple(boxes.shape), tuple(kpts.shape))
        bx, kp = boxes.cpu().numpy(), kpts.cpu().numpy()
        assert np.array_equal(bx[~risky, :4], rb[~risky, :4]) and np.abs(bx[:, :4] - rb[:, :4]).max() <= 1.0
        assert np.abs(bx[:, 4] - rb[:, 4]).max() <= 1e-4 and np.array_equal(bx[:, 5], rb[:, 5])
        exy, ev = np.abs(kp[..., :2] - rk[..., :2]).max(), np.abs(kp[..., 2] - rk[..., 2]).max()
        print(f'predictor image {i}: {len(rb)} rows, keypoint err {exy:.2e} px (bound {b["kxy"] / gain:.2e}), visibility err {ev:.2e}')
        assert exy <= b['kxy'] / gain and ev <= b['kvis']
        total += len(rb)
        risky_total += int(risky.sum())
    assert risky_total <= 0.02 * total
    none = PosePredictor(dict(imgsz=(160, 224), conf=0.99, iou=0.7, max_det=5))
    none.setup_model(m)
    res = none(imgs)
    assert all(tuple(bx.shape) == (0, 6) and tuple(kp.shape) == (0, 17, 3) for bx, kp in res)


@pytest.mark.gpu
def test_quantize_fp8_leaves_the_pose_head_in_bf16():
    """quantize_fp8 on a Pose model runs; the head keeps bf16 operands (no fp8 launch comes from it), so on the inputs the quantised model hands
    it the head's outputs stay within the bf16 bounds of the unquantised head's."""
    from mgdt_yolo_amd import ops
    g = fixture()
    _, kpt_shape, shape = PR.CASES[PR.FULL]
    m = build_model('yolov8-pose', kpt_shape, torch.bfloat16)
    x = seeded_images(*shape, seed=PR.IMG_SEED).to(DEV).to(torch.bfloat16)
    table = m.quantize_fp8(x)
    head = m.model[-1]
    hname = [n for n, mod in m.named_modules() if mod is head][0]
    assert table and not any(k.startswith(hname + '.') or k.startswith(hname + ':') for k in table)
    seen = {}
    h = head.register_forward_pre_hook(lambda mod, a: seen.__setitem__('x', [t.clone() for t in a[0]]))
    with torch.no_grad(), ops.profile() as p:
        cat_q = m(x)[0]
    h.remove()
    assert 'conv2d_fp8_fwd' in [r[0] for r in p.rows]
    with torch.no_grad(), ops.profile() as p:
        cat_head_q = head([t.clone() for t in seen['x']])[0]
    assert 'conv2d_fp8_fwd' not in [r[0] for r in p.rows] and torch.equal(cat_head_q, cat_q)
    m.dequantize_fp8()
    with torch.no_grad():
        cat_head = head([t.clone() for t in seen['x']])[0]
    check_within('fp8 model: head on the same inputs, quantised vs not', cat_head_q.cpu().numpy(), cat_head.cpu().numpy(), kpt_shape, bf16_bounds(g, PR.FULL))
