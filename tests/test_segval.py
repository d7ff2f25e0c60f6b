"""Segmentation validation: mask IoU (mgdt_mask_iou_fwd), ground truth at another resolution (mgdt_gt_masks_resample_fwd), matching from an IoU
matrix (mgdt_val_match_iou_fwd), metrics.mask_iou and SegmentationValidator against what the reference's own code returned on seeded inputs
(tests/golden/segval_NN.npz, produced by tests/golden/gen_segval.py; inputs re-created by tests/segval_ref.py).

Output convention pinned here: entries of the IoU matrix past nlab[i] / counts[i] are WRITTEN as zero; nothing outside the (B, max_lab, max_det)
block is touched (guard values before and after)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segval_ref as R  # noqa: E402

from mgdt_yolo_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
NEW = ('mgdt_mask_iou_workspace_bytes', 'mgdt_mask_iou_fwd', 'mgdt_gt_masks_resample_fwd', 'mgdt_val_match_iou_fwd')
KEYS = [f'metrics/{k}({s})' for s in 'BM' for k in ('precision', 'recall', 'mAP50', 'mAP50-95')]
_FIX = []


def fixture():
    if not _FIX:
        _FIX.append(R.load_fixture())
    return _FIX[0]


# ------------------------------------------------------------------------------------------------ host
def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'mgdt.h')).read()
    declared = set(re.findall(r'\b(mgdt_[a-z0-9_]+)\s*\(', hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.mgdt_mask_iou_workspace_bytes(32, 300, 20) == 32 * (32 * 304 + 304 + 32) * 4
    assert lib.mgdt_mask_iou_workspace_bytes(0, 300, 20) == 0


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.lib()
    BAD_SHAPE, BAD_ARG = -1, -4
    p = 16          # a non-null address that is never dereferenced: every refusal below happens on the host
    ok = dict(pred=p, counts=p, offsets=p, n=1, max_det=300, gt=p, index=1, nlab=p, loff=None, max_lab=255, hw=640 * 640, eps=1e-7, iou=p, ws=p,
              ws_bytes=1 << 30)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mgdt_mask_iou_fwd(a['pred'], a['counts'], a['offsets'], a['n'], a['max_det'], a['gt'], a['index'], a['nlab'], a['loff'], a['max_lab'],
                                     a['hw'], a['eps'], a['iou'], a['ws'], a['ws_bytes'], None)
    for k in ('pred', 'counts', 'offsets', 'gt', 'nlab', 'iou', 'ws'):
        assert call(**{k: None}) == BAD_ARG, k
        assert b'null' in lib.mgdt_last_error()
    assert call(index=0, loff=None) == BAD_ARG                  # instance masks need their offsets
    assert call(ws_bytes=16) == BAD_ARG
    for kw in (dict(max_det=1025), dict(max_det=0), dict(max_lab=256), dict(index=0, loff=p, max_lab=257), dict(max_lab=0), dict(hw=(1 << 24) + 1),
               dict(hw=0), dict(n=0), dict(n=65536), dict(n=65535, max_det=1024)):
        assert call(**kw) == BAD_SHAPE, kw
        assert b'mask_iou' in lib.mgdt_last_error()
    assert lib.mgdt_gt_masks_resample_fwd(None, 1, p, p, 1, 4, 8, 8, 16, 16, p, None) == BAD_ARG
    assert lib.mgdt_gt_masks_resample_fwd(p, 1, p, p, 1, 256, 8, 8, 16, 16, p, None) == BAD_SHAPE
    assert lib.mgdt_gt_masks_resample_fwd(p, 1, p, p, 1, 4, 8, 0, 16, 16, p, None) == BAD_SHAPE
    assert lib.mgdt_val_match_iou_fwd(None, 1, 4, 4, p, 6, p, p, 5, p, p, 10, p, None) == BAD_ARG
    assert lib.mgdt_val_match_iou_fwd(p, 1, 4, 4, p, 6, p, p, 5, p, p, 17, p, None) == BAD_SHAPE
    assert lib.mgdt_val_match_iou_fwd(p, 1, 4, 4, p, 0, p, p, 5, p, p, 10, p, None) == BAD_SHAPE


def test_validator_refuses_host_tooling_clearly():
    from mgdt_yolo_amd.yolo.v8.segment import SegmentationValidator
    for k in ('plots', 'save_json', 'single_cls'):
        with pytest.raises(RuntimeError, match='host-side tooling'):
            SegmentationValidator(device='cpu', args={k: True})
    v = SegmentationValidator(device='cpu', args=dict(plots=False))
    with pytest.raises(RuntimeError, match='mask_mode'):
        v.init_metrics(mask_mode='process_mask_native')
    for fn in (v.pred_to_json, v.plot_predictions, v.plot_val_samples, v.eval_json):
        with pytest.raises(RuntimeError, match='host-side tooling'):
            fn()
    from mgdt_yolo_amd.yolo.utils.metrics import mask_iou
    with pytest.raises(RuntimeError, match='no CPU'):
        mask_iou(torch.zeros(2, 16), torch.zeros(3, 16))


def test_restatement_reproduces_the_fixture():
    """The int64 / float32 restatement the GPU tests lean on: IoU bit for bit, both `correct` matrices exactly, resampling outside the band."""
    g = fixture()
    for name in R.CASES:
        for k, (idx, pred, det, lab) in enumerate(R.case_inputs(name)):
            nd, nl = det.shape[0], lab.shape[0]
            key = f'{name}_{k}'
            assert g[key + '_iou'].shape == (nl, nd)
            if not (nd and nl):
                assert not g[key + '_cm'].any() and not g[key + '_cb'].any()
                continue
            iou = R.mask_iou_exact(R.instances(idx, nl), pred)
            assert np.array_equal(iou.view(np.uint32), g[key + '_iou'].view(np.uint32)), key
            assert np.array_equal(R.match(iou, lab[:, 0], det[:, 5]), g[key + '_cm']), key
            assert np.array_equal(R.match(R.box_iou_f32(lab[:, 1:], det[:, :4]), lab[:, 0], det[:, 5]), g[key + '_cb']), key
    for name in R.ASYM_CASES:
        gt, pred, _ = R.asym_inputs(name)
        assert np.array_equal(R.mask_iou_exact(gt, pred).view(np.uint32), g[name + '_iou'].view(np.uint32)), name
    for name in R.RESAMPLE_CASES:
        idx, nl, out = R.resample_inputs(name)
        ref, band = R.unpack(g[name + '_m'], (nl, *out)), R.unpack(g[name + '_u'], (nl, *out))
        vals = np.stack([R.resample_values(idx == j + 1, out) for j in range(nl)])
        assert not (((vals > 0.5) != ref) & ~band).any(), name
        assert band.mean() <= 1e-3 and (name != 'r4' or not band.any())


# ------------------------------------------------------------------------------------------------ GPU
def _batch(name, dev=DEV):
    """The images of a case in the kernels' batch layout (device tensors) + the host inputs."""
    from mgdt_yolo_amd import ops
    imgs = R.case_inputs(name)
    (h, w), _ = R.CASES[name]
    counts = [im[2].shape[0] for im in imgs]
    nl = [im[3].shape[0] for im in imgs]
    b, max_det, max_lab = len(imgs), max(max(counts), 1), max(max(nl), 1)
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dt is None else torch.tensor(a, dtype=dt).to(dev)
    masks = t(np.concatenate([im[1] for im in imgs], 0))
    idx = t(np.stack([im[0] for im in imgs]))
    inst = t(np.concatenate([R.instances(im[0], n) for im, n in zip(imgs, nl)], 0))
    rows = np.zeros((b, max_det, 6), np.float32)
    labels = np.zeros((b, max_lab, 5), np.float32)
    for i, im in enumerate(imgs):
        rows[i, :counts[i]], labels[i, :nl[i]] = im[2], im[3]
    counts_dev, nlab = t(counts, torch.int32), t(nl, torch.int32)
    return dict(imgs=imgs, h=h, w=w, b=b, counts=counts, nl=nl, max_det=max_det, max_lab=max_lab, masks=masks, idx=idx, inst=inst, rows=t(rows),
                labels=t(labels), counts_dev=counts_dev, nlab=nlab, offsets=ops.exclusive_offsets(counts_dev), lab_offsets=ops.exclusive_offsets(nlab))


def _iou_guarded(c, index_map):
    from mgdt_yolo_amd import ops
    n = c['b'] * c['max_lab'] * c['max_det']
    buf = torch.full((n + 128,), 7.5, dtype=torch.float32, device=DEV)
    out = ops.mask_iou_batch(c['masks'], c['counts_dev'], c['offsets'], c['max_det'], c['idx'] if index_map else c['inst'], c['nlab'], c['max_lab'],
                             index_map=index_map, lab_offsets=c['lab_offsets'], out=buf[64:64 + n])
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:64] == 7.5).all() and (host[64 + n:] == 7.5).all(), 'guard values around the IoU block were overwritten'
    return out.view(c['b'], c['max_lab'], c['max_det']).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('index_map', [True, False], ids=['index_map', 'instances'])
@pytest.mark.parametrize('name', list(R.CASES))
def test_mask_iou_is_bit_equal_to_the_reference(name, index_map):
    g = fixture()
    c = _batch(name)
    got = _iou_guarded(c, index_map)
    for i in range(c['b']):
        nd, nl = c['counts'][i], c['nl'][i]
        ref = g[f'{name}_{i}_iou']
        bad = int((got[i, :nl, :nd].view(np.uint32) != ref.view(np.uint32)).sum())
        print(f'{name} image {i}: nd {nd} nl {nl} differing entries {bad}')
        assert bad == 0, (name, i, bad)
        pad = got[i].copy()
        pad[:nl, :nd] = 0
        assert not pad.any(), 'entries past nlab / counts must be written as zero'


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(R.ASYM_CASES))
def test_mask_iou_on_asymmetric_data_catches_permuted_operands(name):
    """Distinct areas and pairwise distinct intersections: a transposed or permuted MFMA operand cannot reproduce this matrix."""
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.yolo.utils.metrics import mask_iou
    g = fixture()
    gt, pred, idx = R.asym_inputs(name)
    nl, nd = gt.shape[0], pred.shape[0]
    ref = g[name + '_iou']
    gt_d, pred_d = torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV)
    for form in ('uint8', 'float32'):
        a, b = (gt_d, pred_d) if form == 'uint8' else (gt_d.float(), pred_d.float())
        got = mask_iou(a.view(nl, -1), b.view(nd, -1)).cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, form)
    if idx is not None:
        one = lambda k: torch.full((1,), k, dtype=torch.int32, device=DEV)
        zero = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = ops.mask_iou_batch(pred_d, one(nd), zero, nd, torch.from_numpy(idx)[None].to(DEV), one(nl), nl, index_map=True)[0].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['b160', 'b40', 'inst40'])
def test_metrics_mask_iou_is_bit_equal_to_the_reference(name):
    from mgdt_yolo_amd.yolo.utils.metrics import mask_iou
    g = fixture()
    for i, (idx, pred, det, lab) in enumerate(R.case_inputs(name)):
        nd, nl = det.shape[0], lab.shape[0]
        n = idx.size                                              # explicit: view(0, -1) of an image without labels / detections is ambiguous
        gt = torch.from_numpy(R.instances(idx, nl)).to(DEV).float().view(nl, n)
        got = mask_iou(gt, torch.from_numpy(pred).to(DEV).float().view(nd, n)).cpu().numpy()
        assert got.shape == (nl, nd)
        if nd and nl:
            assert np.array_equal(got.view(np.uint32), g[f'{name}_{i}_iou'].view(np.uint32)), (name, i)


@pytest.mark.gpu
@pytest.mark.parametrize('overlap', [True, False], ids=['index_map', 'instances'])
@pytest.mark.parametrize('name', list(R.MATCH_CASES))
def test_correct_matrices_equal_the_reference_per_image_and_in_batch(name, overlap):
    from mgdt_yolo_amd.yolo.v8.segment import SegmentationValidator
    g = fixture()
    c = _batch(name)
    v = SegmentationValidator(device=DEV)
    v.init_metrics(nc=R.NC, overlap_mask=overlap)
    cb, cm = v.match_batch(c['rows'], c['counts_dev'], c['masks'], c['labels'], c['nlab'], c['idx'] if overlap else c['inst'], overlap=overlap)
    cb, cm = cb.cpu().numpy(), cm.cpu().numpy()
    stats = []
    for i, (idx, pred, det, lab) in enumerate(c['imgs']):
        nd, nl = c['counts'][i], c['nl'][i]
        assert np.array_equal(cb[i, :nd], g[f'{name}_{i}_cb']), (name, i, 'boxes, batch')
        assert np.array_equal(cm[i, :nd], g[f'{name}_{i}_cm']), (name, i, 'masks, batch')
        assert not cb[i, nd:].any() and not cm[i, nd:].any()
        d, l = torch.from_numpy(det).to(DEV), torch.from_numpy(lab).to(DEV)
        gt = torch.from_numpy(idx)[None].to(DEV).float() if overlap else torch.from_numpy(R.instances(idx, nl)).to(DEV).float()
        one_b = v._process_batch(d, l).cpu().numpy()
        one_m = v._process_batch(d, l, torch.from_numpy(pred).to(DEV).float(), gt, overlap=overlap, masks=True).cpu().numpy()
        assert np.array_equal(one_b, cb[i, :nd]) and np.array_equal(one_m, cm[i, :nd]), (name, i, 'per image != batch')
        if nd or nl:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
            stats.append((t(cb[i, :nd]), t(cm[i, :nd]), t(det[:, 4]), t(det[:, 5]), t(lab[:, 0])))
    v.stats = stats
    s = v.get_stats()
    got = np.array([s[k] for k in KEYS])
    print(name, 'summary', got.tolist(), 'max |delta|', float(np.abs(got - g[name + '_summary']).max()))
    assert np.abs(got - g[name + '_summary']).max() <= 1e-6
    assert v.ap.shape == v.ap_mask.shape and len(v.ap_class_index) == v.ap.shape[0] and v.nt_per_class.sum() == sum(c['nl'])


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(R.RESAMPLE_CASES))
def test_ground_truth_resampling_matches_the_reference(name):
    """Ratio 4: every weight is dyadic, the decision is exact.  Other ratios: exact outside the recorded band of |v - 0.5| <= 1e-5."""
    from mgdt_yolo_amd import ops
    g = fixture()
    idx, nl, out = R.resample_inputs(name)
    ref, band = R.unpack(g[name + '_m'], (nl, *out)), R.unpack(g[name + '_u'], (nl, *out))
    nlab = torch.tensor([nl, nl], dtype=torch.int32).to(DEV)
    loff = torch.tensor([0, nl], dtype=torch.int32).to(DEV)
    idx2 = torch.from_numpy(np.stack([idx, idx])).to(DEV)
    inst2 = torch.from_numpy(np.concatenate([R.instances(idx, nl)] * 2, 0)).to(DEV)
    for index_map, gt in ((True, idx2), (False, inst2)):
        got = ops.gt_masks_resample(gt, nlab, loff, 2 * nl, nl, out, index_map=index_map).cpu().numpy().astype(bool)
        for half in (got[:nl], got[nl:]):
            bad = (half != ref) & ~band
            assert not bad.any(), (name, index_map, int(bad.sum()))
            if name == 'r4':
                assert np.array_equal(half, ref)


@pytest.mark.gpu
def test_match_batch_resamples_ground_truth_of_another_size():
    """Predictions at 4x the ground truth's size (the process_mask_upsample route): match_batch == matching against the reference's resampled masks."""
    from mgdt_yolo_amd.yolo.v8.segment import SegmentationValidator
    g = fixture()
    idx, nl, out = R.resample_inputs('r4')
    ref = R.unpack(g['r4_m'], (nl, *out))
    r = np.random.default_rng(5)
    nd = 20
    pred = np.stack([R._shift(ref[d % nl], int(r.integers(-6, 7)), int(r.integers(-6, 7))) for d in range(nd)]).astype(np.uint8)
    det = np.zeros((1, nd, 6), np.float32)
    det[0, :, 2:4] = 5
    lab = np.zeros((1, nl, 5), np.float32)
    lab[0, :, 3:] = 5
    iou = R.mask_iou_exact(ref.astype(np.uint8), pred)
    want = R.match(iou, lab[0, :, 0], det[0, :, 5])
    assert want[:, 0].sum() >= 3
    v = SegmentationValidator(device=DEV)
    v.init_metrics(nc=R.NC)
    t = lambda a: torch.from_numpy(a).to(DEV)
    cnt = lambda k: torch.tensor([k], dtype=torch.int32).to(DEV)
    _, cm = v.match_batch(t(det), cnt(nd), t(pred), t(lab), cnt(nl), t(idx)[None], overlap=True)
    assert np.array_equal(cm[0].cpu().numpy(), want)


@pytest.mark.gpu
def test_match_batch_replays_in_a_captured_graph_equal_to_eager():
    from mgdt_yolo_amd.yolo.v8.segment import SegmentationValidator
    c = _batch('b160')
    v = SegmentationValidator(device=DEV)
    v.init_metrics(nc=R.NC)
    v.iouv = v.iouv.to(DEV)

    def step():
        return v.match_batch(c['rows'], c['counts_dev'], c['masks'], c['labels'], c['nlab'], c['idx'], overlap=True, offsets=c['offsets'],
                             lab_offsets=c['lab_offsets'])
    eager = [x.clone() for x in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(3):
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, out))
    assert bool(eager[1].any())


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_validator_on_the_models_own_predictions_matches_the_cpu_restatement(dt):
    """postprocess -> update_metrics -> get_stats on the seeded yolov8-seg n (fp32, 2x160x224, validator settings) against a CPU pipeline built from
    tests/segval_ref.py on the SAME GPU predictions (the model's parity is pinned by test_segment.py; this isolates the validator).  Labels: every
    other of an image's first 40 detections with its own mask shifted / dilated and its box jittered, plus two instances nothing predicts.
    Run in both ground-truth forms.  The seeded model's masks cover much of the image and overlap, so in index-map form (later labels overwrite
    earlier ones) few labels survive whole: the non-triviality condition (>= 5 true positives at 0.5, fewer at 0.95) is asserted on the instance
    form, at least one true positive at 0.5 on the index-map form.  Tolerance 1e-3 on the eight summary numbers, as in
    test_map50_parity_with_the_cpu_reference_pipeline; the mask `correct` matrix is integer arithmetic and must agree exactly.  bf16: the same run
    with the figures printed and no bound asserted (DESIGN.md records them)."""
    strict = dt == torch.float32
    from mgdt_yolo_amd.models import get_config
    from mgdt_yolo_amd.nn.tasks import SegmentationModel
    from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images
    from mgdt_yolo_amd.yolo.utils import ops as uops
    from mgdt_yolo_amd.yolo.v8.segment import SegmentationValidator
    from oracle import metrics as OM
    H, W, mh, mw = 160, 224, 40, 56
    m = SegmentationModel(get_config('yolov8-seg', 'n', 80), verbose=False)
    seed_state_dict_(m, 0)
    m = m.eval().set_compute_dtype(dt).to(DEV)
    x = seeded_images(2, H, W, seed=3).to(DEV).to(dt)
    with torch.no_grad():
        preds = m(x)
    v = SegmentationValidator(device=DEV)
    v.init_metrics(nc=80, conf=0.001, iou=0.7, max_det=100)
    per, proto = v.postprocess(preds)
    counts = [int(p.shape[0]) for p in per]
    assert min(counts) > 10 or not strict
    masks = uops.process_mask_batch(proto, v._nms[1], v._nms[2], (H, W), 'process_mask', torch.uint8, counts_host=counts).cpu().numpy()
    assert masks.shape[1:] == (mh, mw)
    rows = [p.cpu().numpy() for p in per]
    r = np.random.default_rng(11)
    cls_l, box_l, bidx, inst, off = [], [], [], [[], []], 0

    def add(i, g, cls, b):
        inst[i].append(g)
        cls_l.append([float(cls)])
        box_l.append([float((b[0] + b[2]) / 2 / W), float((b[1] + b[3]) / 2 / H), float((b[2] - b[0]) / W), float((b[3] - b[1]) / H)])
        bidx.append(i)
    for i in range(2):
        pm = masks[off:off + counts[i]].astype(bool)
        off += counts[i]
        for d in range(0, min(counts[i], 40), 2):
            g = R._shift(pm[d], int(r.integers(-1, 2)), int(r.integers(-1, 2)))
            if r.random() < 0.5:
                g = R._dilate(g)
            if g.any():
                add(i, g, rows[i][d, 5], rows[i][d, :4] + r.uniform(-3, 3, 4))
        for _ in range(2):
            g = R._shape(r, mh, mw, 0.2)
            add(i, g, 79.0, R._bbox(g, r, 0.0) * 4)
    maps = []
    for i in range(2):
        idx = np.zeros((mh, mw), np.uint8)
        for j, g in enumerate(inst[i]):
            idx[g] = j + 1
        maps.append(idx)
    cls_a, box_a, bidx_a = np.array(cls_l, np.float32)[:, 0], np.array(box_l, np.float32), np.array(bidx)
    whwh = np.array([W, H, W, H], np.float32)
    rp = ((1.0, 1.0), (0.0, 0.0))
    for overlap in (False, True):
        gt_all = np.stack(maps) if overlap else np.concatenate([np.stack(a) for a in inst], 0).astype(np.uint8)
        batch = dict(img=x, cls=torch.tensor(cls_l, dtype=torch.float32), bboxes=torch.tensor(box_l, dtype=torch.float32),
                     batch_idx=torch.tensor(bidx, dtype=torch.float32), masks=torch.from_numpy(gt_all), ori_shape=[(H, W)] * 2, ratio_pad=[rp] * 2)
        v.init_metrics(nc=80, conf=0.001, iou=0.7, max_det=100, overlap_mask=overlap)
        v.update_metrics((per, proto), v.preprocess(batch))
        assert v.seen == 2 and len(v.stats) == 2
        got = v.get_stats()
        # ---- the same on the CPU
        stats, off = [], 0
        for i in range(2):
            pm = masks[off:off + counts[i]]
            off += counts[i]
            sel = bidx_a == i
            nl = int(sel.sum())
            bx = box_a[sel]
            half = bx[:, 2:] / np.float32(2)
            xyxy = np.concatenate([bx[:, :2] - half, bx[:, :2] + half], 1) * whwh
            lab_boxes = OM.scale_boxes((H, W), xyxy, (H, W), ratio_pad=rp)
            predn = OM.scale_boxes((H, W), rows[i][:, :4], (H, W), ratio_pad=rp)
            lcls, dcls = cls_a[sel], rows[i][:, 5]
            gt = R.instances(maps[i], nl) if overlap else np.stack(inst[i]).astype(np.uint8)
            cb = R.match(R.box_iou_f32(lab_boxes, predn), lcls, dcls)
            cm = R.match(R.mask_iou_exact(gt, pm), lcls, dcls)
            dev_cb, dev_cm = v.stats[i][0].cpu().numpy(), v.stats[i][1].cpu().numpy()
            print(f'overlap {overlap} image {i}: {counts[i]} detections, {nl} labels, tp boxes {cb.sum(0).tolist()} masks {cm.sum(0).tolist()}, '
                  f'entries differing from the device boxes {int((cb != dev_cb).sum())} masks {int((cm != dev_cm).sum())}')
            assert np.array_equal(cm, dev_cm) or not strict, 'mask matching is exact integer arithmetic: it must agree entry for entry'
            stats.append((cb, cm, rows[i][:, 4], dcls, lcls))
        cb, cm, conf, pcls, tcls = [np.concatenate(a, 0) for a in zip(*stats)]
        if strict:
            assert cm[:, 0].sum() >= (1 if overlap else 5) and cm[:, 9].sum() < cm[:, 0].sum(), 'the metric must be non-trivial'
        want = []
        for tp in (cb, cm):
            if tp.any():
                _, _, p, rr, _, ap, _ = OM.ap_per_class(tp, conf, pcls, tcls)
                want += [p.mean(), rr.mean(), ap[:, 0].mean(), ap.mean()]
            else:
                want += [0.0] * 4
        g = np.array([got[k] for k in KEYS])
        print('device', g.tolist())
        print('cpu   ', [float(w) for w in want])
        print(f'{dt} overlap {overlap}: max |device - cpu| over the eight numbers {float(np.abs(g - np.array(want)).max()):.3e}')
        assert np.abs(g - np.array(want)).max() <= 1e-3 or not strict


@pytest.mark.gpu
def test_whole_chain_from_the_fixture_rows_and_protos():
    """process_mask_batch -> IoU -> match -> get_stats on the `val` NMS rows and protos of tests/golden/seg_NN.npz against the reference's own
    process_mask, _process_batch and ap_per_class on them (fixture chain_*).  Masks: equal to the reference outside the recorded 1e-3 band.  Box
    `correct`: equal.  Mask `correct`: equal, except for detections the fixture lists (they own a band pixel and a candidate IoU within
    band_pixels / union of a level; capped at 2 % of the detections at generation).  The eight numbers: within 1e-6 when no detection of the
    case is excepted."""
    import seg_ref as SR
    from mgdt_yolo_amd.yolo.utils import ops as uops
    from mgdt_yolo_amd.yolo.v8.segment import SegmentationValidator
    g, f = fixture(), SR.load_fixture()
    tag, (H, W) = R.CHAIN_TAG, R.CHAIN_SHAPE
    protos = torch.from_numpy(f[tag + '_p']).to(DEV)
    b, mh, mw = protos.shape[0], protos.shape[2], protos.shape[3]
    rows_h = [f[f'{tag}_nms_val_{i}'] for i in range(b)]
    counts = [r.shape[0] for r in rows_h]
    labs = [g[f'chain_{i}_lab'] for i in range(b)]
    nl = [l.shape[0] for l in labs]
    rows = np.zeros((b, max(counts), rows_h[0].shape[1]), np.float32)
    labels = np.zeros((b, max(nl), 5), np.float32)
    for i in range(b):
        rows[i, :counts[i]], labels[i, :nl[i]] = rows_h[i], labs[i]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rows_d, counts_dev, nlab = t(rows), torch.tensor(counts, dtype=torch.int32).to(DEV), torch.tensor(nl, dtype=torch.int32).to(DEV)
    masks = uops.process_mask_batch(protos, rows_d, counts_dev, (H, W), 'process_mask', torch.uint8, counts_host=counts)
    gt = t(np.concatenate([R.unpack(g[f'chain_{i}_gt'], (nl[i], mh, mw)) for i in range(b)], 0).astype(np.uint8))
    v = SegmentationValidator(device=DEV)
    v.init_metrics(nc=80, conf=0.001, iou=0.7, max_det=max(counts), overlap_mask=False)
    cb, cm = v.match_batch(rows_d, counts_dev, masks, t(labels), nlab, gt, overlap=False)
    cb, cm, masks_h = cb.cpu().numpy(), cm.cpu().numpy(), masks.cpu().numpy().astype(bool)
    stats, off, excepted = [], 0, 0
    for i in range(b):
        n = counts[i]
        ref, und = R.unpack(g[f'chain_{i}_m'], (n, mh, mw)), R.unpack(g[f'chain_{i}_u'], (n, mh, mw))
        got = masks_h[off:off + n]
        off += n
        assert not ((got != ref) & ~und).any(), f'image {i}: masks differ from the reference outside the band'
        exc = g[f'chain_{i}_exc']
        assert exc.mean() <= 0.02
        assert np.array_equal(cb[i, :n], g[f'chain_{i}_cb']), f'image {i}: box matching'
        diff = (cm[i, :n] != g[f'chain_{i}_cm']).any(1)
        print(f'image {i}: {n} detections, mask pixels differing inside the band {int((got != ref).sum())}, detections excepted {int(exc.sum())}, '
              f'detections whose mask matching differs {np.nonzero(diff)[0].tolist()}')
        assert not (diff & ~exc).any(), f'image {i}: mask matching differs for detections {np.nonzero(diff & ~exc)[0].tolist()} outside the exception list'
        excepted += int(exc.sum())
        stats.append((t(cb[i, :n]), t(cm[i, :n]), t(rows_h[i][:, 4]), t(rows_h[i][:, 5]), t(labs[i][:, 0])))
    v.stats = stats
    s = v.get_stats()
    num = np.array([s[k] for k in KEYS])
    print('summary', num.tolist(), 'max |delta|', float(np.abs(num - g['chain_summary']).max()))
    if excepted == 0:
        assert np.abs(num - g['chain_summary']).max() <= 1e-6


@pytest.mark.gpu
def test_unsorted_batch_idx_with_instance_masks_through_update_metrics():
    """overlap_mask=False: the instance masks are per-label rows and must follow the validator's stable re-sort of an unsorted batch_idx.  The rows,
    protos, labels and instance masks of test_whole_chain_from_the_fixture_rows_and_protos as a dataloader dict (normalised labels, identity
    letter-box); the labels once grouped by image, once interleaved: `stats` and `get_stats()` must be EQUAL."""
    import seg_ref as SR
    from mgdt_yolo_amd.yolo.v8.segment import SegmentationValidator
    g, f = fixture(), SR.load_fixture()
    tag, (H, W) = R.CHAIN_TAG, R.CHAIN_SHAPE
    protos = torch.from_numpy(f[tag + '_p']).to(DEV)
    b, mh, mw = protos.shape[0], protos.shape[2], protos.shape[3]
    per = [torch.from_numpy(f[f'{tag}_nms_val_{i}']).to(DEV) for i in range(b)]
    labs = [g[f'chain_{i}_lab'] for i in range(b)]
    lab = np.concatenate(labs, 0).astype(np.float32)
    bidx = np.concatenate([np.full(len(l), i, np.float32) for i, l in enumerate(labs)])
    gt = np.concatenate([R.unpack(g[f'chain_{i}_gt'], (len(labs[i]), mh, mw)) for i in range(b)], 0).astype(np.uint8)
    xywh = np.stack([(lab[:, 1] + lab[:, 3]) / 2 / W, (lab[:, 2] + lab[:, 4]) / 2 / H, (lab[:, 3] - lab[:, 1]) / W, (lab[:, 4] - lab[:, 2]) / H], 1).astype(np.float32)
    perm = np.random.default_rng(2).permutation(len(lab))
    assert min(len(l) for l in labs) > 1 and (np.diff(bidx[perm]) < 0).any()
    res = {}
    for order, p in (('sorted', np.arange(len(lab))), ('unsorted', perm)):
        batch = dict(img=torch.zeros(b, 3, H, W), cls=torch.from_numpy(lab[p, :1]), bboxes=torch.from_numpy(xywh[p]), batch_idx=torch.from_numpy(bidx[p]),
                     masks=torch.from_numpy(gt[p]), ori_shape=[(H, W)] * b, ratio_pad=[((1.0, 1.0), (0.0, 0.0))] * b)
        v = SegmentationValidator(device=DEV)
        v.init_metrics(nc=80, conf=0.001, iou=0.7, max_det=max(len(r) for r in per), overlap_mask=False)
        v.update_metrics((per, protos), v.preprocess(batch))
        assert v.seen == b and len(v.stats) == b
        res[order] = (v.stats, v.get_stats())
    assert res['sorted'][1]['metrics/mAP50(M)'] > 0, 'the mask matching must be non-trivial'
    assert res['unsorted'][1] == res['sorted'][1]
    # within an image the labels keep their shuffled order: the matches of a detection do not depend on it, the class list is a permutation
    for got, want in zip(res['unsorted'][0], res['sorted'][0]):
        assert all(torch.equal(a, e) for a, e in zip(got[:4], want[:4])) and torch.equal(got[4].sort().values, want[4].sort().values)

