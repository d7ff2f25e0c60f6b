"""Validator statistics beyond mAP: the detection confusion matrix and the counting metrics (mgdt_val_confusion_fwd, metrics.ConfusionMatrix,
metrics.CountMetrics, DetectionValidator(confusion=True, counting=True)) against what the reference's own ConfusionMatrix returned on seeded
inputs (tests/golden/confusion_00.npz, produced by tests/golden/gen_confusion.py; inputs re-created by tests/valstats_ref.py) and against the
plain-Python restatement of the counting script.

Every compared quantity is an integer and must be EQUAL; there is no tolerance.  What makes that well defined are conditions on the inputs, asserted
by the generator and again here: no IoU within 1e-5 of a threshold (the device computes the counting IoU in float32, the script in float64: they
differ by a few 1e-7), no confidence within 1e-6 of one, no two competing IoUs within 1e-5 of each other (the reference's argsort is unstable).
The float results (MAE, RMSE, R^2) are functions of the integer slots: compared with the direct float64 formulas to 1e-12 (a handful of float64
roundings on values of order 1 to 1e3)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import valstats_ref as R  # noqa: E402

from mgdt_yolo_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
MAP_KEYS = ['metrics/precision(B)', 'metrics/recall(B)', 'metrics/mAP50(B)', 'metrics/mAP50-95(B)']
_FIX, _IMGS = [], {}


def fixture():
    if not _FIX:
        _FIX.append(R.load_fixture())
    return _FIX[0]


def images(case):
    if case not in _IMGS:
        _IMGS[case] = R.case_inputs(case, int(fixture()[case + '_salt']))
    return _IMGS[case]


# ------------------------------------------------------------------------------------------------ host
def test_new_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'mgdt.h')).read()
    declared = set(re.findall(r'\b(mgdt_[a-z0-9_]+)\s*\(', hdr))
    assert 'mgdt_val_confusion_fwd' in declared and 'mgdt_val_confusion_fwd' in _lib.PROTOTYPES and hasattr(_lib.lib(), 'mgdt_val_confusion_fwd')
    from mgdt_yolo_amd import ops
    assert ops.COUNT_SLOTS == len(R.SLOTS) == int(re.search(r'#define MGDT_COUNT_SLOTS (\d+)', hdr).group(1))


@pytest.mark.parametrize('case', list(R.CASES))
def test_restatement_reproduces_the_fixture(case):
    """valstats_ref.confusion / confusion_none against the matrices the reference's process_batch produced, image by image, on the CPU; the
    counting slots are the restatement's own and must add up."""
    g = fixture()
    nc, max_det, specs = R.CASES[case]
    imgs = images(case)
    assert g[case + '_img_matrix'].shape == (len(specs), nc + 1, nc + 1) and g[case + '_img_counts'].shape == (len(specs), nc, len(R.SLOTS))
    for i, (det, lab) in enumerate(imgs):
        assert det.shape[0] <= max_det and lab.shape[0] <= 256
        mine = R.confusion(det, lab, nc) if det.shape[0] else R.confusion_none(lab[:, 0], nc)
        assert np.array_equal(mine, g[case + '_img_matrix'][i]), (case, i)
        assert mine[:, :nc].sum() == lab.shape[0], 'every label adds exactly one entry to its column'
        slots = R.counting(det, lab, nc)
        assert np.array_equal(slots, g[case + '_img_counts'][i]), (case, i)
        assert slots[:, 1].sum() == lab.shape[0] and np.array_equal(slots[:, 7] + slots[:, 9], slots[:, 1])
    assert np.array_equal(g[case + '_matrix'], g[case + '_img_matrix'].astype(np.int64).sum(0))
    assert np.array_equal(g[case + '_counts'], g[case + '_img_counts'].sum(0))
    m = g[case + '_matrix'].astype(np.float64)
    assert np.array_equal(g[case + '_tp'], m.diagonal()[:-1]) and np.array_equal(g[case + '_fp'], (m.sum(1) - m.diagonal())[:-1])


@pytest.mark.parametrize('case', list(R.CASES))
def test_fixture_inputs_keep_clear_of_thresholds_and_ties(case):
    nc = R.CASES[case][0]
    for i, (det, lab) in enumerate(images(case)):
        near_iou, near_conf, gap = R.confusion_margins(det, lab)
        cnt_iou, cnt_conf = R.counting_margins(det, lab, nc)
        assert near_iou >= R.NEAR_IOU and cnt_iou >= R.NEAR_IOU, (case, i, near_iou, cnt_iou)          # (a)
        assert near_conf >= R.NEAR_CONF and cnt_conf >= R.NEAR_CONF, (case, i, near_conf, cnt_conf)    # (b)
        assert gap >= R.NEAR_TIE, (case, i, gap)                                                       # (c)


def test_cases_cover_what_they_are_there_for():
    g = fixture()
    assert [R.CASES[c][0] for c in R.CASES] == [1, 2, 2, 80, 1000] and len(R.CASES['c2'][2]) == 5 and len(R.CASES['c1000'][2]) == 3
    kinds = {k for c in R.CASES for k, *_ in R.CASES[c][2]}
    assert {'nodet', 'nolab', 'empty', 'nomatch', 'det3lab', 'lab3det'} <= kinds
    det, lab = images('c80')[0]
    assert det.shape[0] == R.CASES['c80'][1] == 300 and lab.shape[0] == 256 and images('c80')[1][1].shape[0] == 1
    i = [k for k, *_ in R.CASES['c2'][2]].index('nomatch')
    det, lab = images('c2')[i]
    m = g['c2_img_matrix'][i]
    assert (det[:, 4] > 0.25).sum() >= 2 and m[:2, 2].sum() == 0 and m[2, :2].sum() == lab.shape[0], 'no match: no predicted-background entries'
    det, lab = images('c2q')[0]
    s = g['c2q_img_counts'][0]
    assert s[:, 7].sum() == 3 and (s[:, 2] - s[:, 8]).sum() == 1, 'one detection serves three labels'
    assert g['c2q_img_matrix'][1][:2, 2].sum() >= 2, 'one label chosen by three detections: two of them are predicted background'
    assert (R.box_iou_f32(images('c2')[0][1][:, 1:], images('c2')[0][0][:, :4]) > 0.45).sum() >= 36


def test_r2_mae_rmse_from_integer_slots_equal_the_direct_formulas():
    from mgdt_yolo_amd.yolo.utils.metrics import CountMetrics
    g = fixture()
    for case in R.CASES:
        r = CountMetrics.from_slots(g[case + '_counts'])
        for k in ('r2', 'mae', 'rmse'):
            assert np.abs(r[k] - g[case + '_' + k]).max() <= 1e-12, (case, k)
        s = g[case + '_counts']
        assert np.array_equal(r['tp'], s[:, 7]) and np.array_equal(r['fp'], s[:, 8]) and np.array_equal(r['fn'], s[:, 9])
        assert np.array_equal(r['gt'], s[:, 1]) and np.array_equal(r['pred'], s[:, 2])
    # degenerate branches: one image; constant truth with and without error; an ordinary series; a perfect prediction
    series = [([3], [5]), ([2, 2, 2], [2, 2, 2]), ([2, 2, 2], [2, 3, 2]), ([1, 4, 2, 7], [2, 4, 1, 9]), ([0, 5, 9], [0, 5, 9]), ([0, 0], [0, 0])]
    slots = np.array([[len(t), sum(t), sum(p), sum(a * a for a in t), sum(a * b for a, b in zip(t, p)), sum((a - b) ** 2 for a, b in zip(t, p)),
                       sum(abs(a - b) for a, b in zip(t, p)), 0, 0, 0] for t, p in series])
    r = CountMetrics.from_slots(slots)
    assert r['r2'][:3].tolist() == [0.0, 1.0, 0.0] and r['r2'][4] == 1.0 and r['r2'][5] == 1.0
    for k, (t, p) in enumerate(series):
        mae, rmse = R.errors(t, p)
        assert abs(r['r2'][k] - R.r2(t, p)) <= 1e-12 and abs(r['mae'][k] - mae) <= 1e-12 and abs(r['rmse'][k] - rmse) <= 1e-12, k
    empty = CountMetrics.from_slots(np.zeros((2, 10), np.int64))
    assert not any(np.asarray(v).any() for v in empty.values())


def test_cpu_tensors_classify_task_and_plots_are_refused():
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.yolo.utils.metrics import ConfusionMatrix, CountMetrics
    det, lab = torch.zeros(3, 6), torch.zeros(2, 5)
    cnt = lambda k: torch.full((1,), k, dtype=torch.int32)
    for fn in (lambda: ConfusionMatrix(2).process_batch(det, lab), lambda: ConfusionMatrix(2).process_batch(None, lab[:, 0]),
               lambda: CountMetrics(2).process_batch(det, lab), lambda: ConfusionMatrix(2).process_batch_dev(det[None], cnt(3), lab[None], cnt(2)),
               lambda: CountMetrics(2).process_batch_dev(det[None], cnt(3), lab[None], cnt(2)),
               lambda: ops.val_confusion(det[None], cnt(3), lab[None], cnt(2), 2, matrix=torch.zeros(3, 3, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match='no CPU'):
            fn()
    with pytest.raises(RuntimeError, match='ClassificationValidator'):
        ConfusionMatrix(10, task='classify')
    cm = ConfusionMatrix(3)
    for fn in (cm.plot, cm.print):
        with pytest.raises(RuntimeError, match='host-side tooling'):
            fn()
    assert cm.matrix.shape == (4, 4) and cm.matrix.dtype == np.float64 and not cm.matrix.any()
    assert len(cm.tp_fp()) == 2 and cm.tp_fp()[0].shape == (3,)
    assert CountMetrics(2).slots.shape == (2, 10) and set(CountMetrics(1).results_dict) == {f'metrics/count_{k}(0)' for k in ('tp', 'fp', 'fn', 'gt', 'pred', 'mae', 'rmse', 'r2')}


def test_limits_are_refused_before_any_launch():
    lib = _lib.lib()
    BAD_SHAPE, BAD_ARG = -1, -4
    p = 16          # a non-null address that is never dereferenced: every refusal below happens on the host
    ok = dict(det=p, ndet=p, n=1, max_det=300, lab=p, nlab=p, max_lab=40, nc=2, matrix=p, counts=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mgdt_val_confusion_fwd(a['det'], a['ndet'], a['n'], a['max_det'], a['lab'], a['nlab'], a['max_lab'], a['nc'], 0.25, 0.45, 0.25, 0.5, 1,
                                          a['matrix'], a['counts'], None)
    for kw in (dict(det=None), dict(ndet=None), dict(lab=None), dict(nlab=None), dict(matrix=None, counts=None)):
        assert call(**kw) == BAD_ARG, kw
        assert b'val_confusion' in lib.mgdt_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(max_det=0), dict(max_det=1025), dict(max_lab=0), dict(max_lab=257), dict(nc=0), dict(nc=4097)):
        assert call(**kw) == BAD_SHAPE, kw
        assert b'val_confusion' in lib.mgdt_last_error()


# ------------------------------------------------------------------------------------------------ GPU
_BATCH = {}


def _batch(case):
    """The images of a case in the kernel's batch layout, rows past ndet / nlab filled with boxes that would match (device tensors, built once per
    case and left unchanged)."""
    if case not in _BATCH:
        det, ndet, lab, nlab = R.batch_layout(case, images(case))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        _BATCH[case] = dict(det=t(det), ndet=t(ndet), lab=t(lab), nlab=t(nlab), nc=R.CASES[case][0])
    return _BATCH[case]


def _run(c, matrix=True, counts=True, guard=False):
    """One launch into fresh accumulators -> (matrix (nc+1, nc+1) int32 | None, counts (nc, 10) int64 | None) as numpy."""
    from mgdt_yolo_amd import ops
    nc = c['nc']
    nm, ncnt = (nc + 1) ** 2, nc * ops.COUNT_SLOTS
    mbuf = torch.zeros(nm + 128, dtype=torch.int32, device=DEV)
    cbuf = torch.zeros(ncnt + 128, dtype=torch.int64, device=DEV)
    if guard:
        mbuf[:64], mbuf[64 + nm:], cbuf[:64], cbuf[64 + ncnt:] = 7, 7, 7, 7
    m = mbuf[64:64 + nm] if matrix else None
    k = cbuf[64:64 + ncnt] if counts else None
    ops.val_confusion(c['det'], c['ndet'], c['lab'], c['nlab'], nc, matrix=m, counts=k, cm_conf=R.CM_CONF, cm_iou=R.CM_IOU, cnt_conf=R.CNT_CONF,
                      cnt_iou=R.CNT_IOU, trunc_labels=True)
    torch.cuda.synchronize()
    mh, ch = mbuf.cpu().numpy(), cbuf.cpu().numpy()
    if guard:
        assert (mh[:64] == 7).all() and (mh[64 + nm:] == 7).all() and (ch[:64] == 7).all() and (ch[64 + ncnt:] == 7).all(), 'guard values were overwritten'
    if not matrix:
        assert not mh.any()
    if not counts:
        assert not ch.any()
    return (mh[64:64 + nm].reshape(nc + 1, nc + 1) if matrix else None), (ch[64:64 + ncnt].reshape(nc, -1) if counts else None)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(R.CASES))
def test_matrix_and_count_slots_equal_the_fixture_exactly(case):
    g = fixture()
    c = _batch(case)
    m, k = _run(c, guard=True)
    # the batch form feeds every image; the reference's validator does not call process_batch for an image without labels, which adds nothing
    assert np.array_equal(m, g[case + '_matrix']), (case, np.argwhere(m != g[case + '_matrix'])[:8].tolist())
    assert np.array_equal(k, g[case + '_counts']), (case, np.argwhere(k != g[case + '_counts'])[:8].tolist())
    m2, k2 = _run(c)
    assert np.array_equal(m, m2) and np.array_equal(k, k2), 'two runs of the same batch must give identical buffers'
    m_only, none = _run(c, counts=False)
    none2, k_only = _run(c, matrix=False)
    assert none is None and none2 is None and np.array_equal(m_only, m) and np.array_equal(k_only, k)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['c1', 'c2', 'c2q', 'c1000'])
def test_per_image_forms_equal_the_batch_form_and_calls_accumulate(case):
    from mgdt_yolo_amd.yolo.utils.metrics import ConfusionMatrix, CountMetrics
    g = fixture()
    c = _batch(case)
    nc = c['nc']
    cm_b, ct_b = ConfusionMatrix(nc), CountMetrics(nc)
    cm_b.process_batch_dev(c['det'], c['ndet'], c['lab'], c['nlab'])
    ct_b.process_batch_dev(c['det'], c['ndet'], c['lab'], c['nlab'])
    assert cm_b.matrix.dtype == np.float64 and np.array_equal(cm_b.matrix, g[case + '_matrix']) and np.array_equal(ct_b.slots, g[case + '_counts'])
    tp, fp = cm_b.tp_fp()
    assert np.array_equal(tp, g[case + '_tp']) and np.array_equal(fp, g[case + '_fp'])
    cm_i, ct_i = ConfusionMatrix(nc), CountMetrics(nc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for i, (det, lab) in enumerate(images(case)):
        one = ConfusionMatrix(nc)
        if det.shape[0] == 0:
            one.process_batch(None, t(lab[:, 0]))              # the class vector, as the reference's validator passes it
            cm_i.process_batch(None, t(lab))                   # and the (M, 5) rows
            ct_i.process_batch(None, t(lab))
        else:
            one.process_batch(t(det), t(lab))
            cm_i.process_batch(t(det), t(lab))
            ct_i.process_batch(t(det), t(lab))
        assert np.array_equal(one.matrix, g[case + '_img_matrix'][i]), (case, i)
    assert np.array_equal(cm_i.matrix, cm_b.matrix) and np.array_equal(ct_i.slots, ct_b.slots)
    cm_b.process_batch_dev(c['det'], c['ndet'], c['lab'], c['nlab'])
    ct_b.process_batch_dev(c['det'], c['ndet'], c['lab'], c['nlab'])
    assert np.array_equal(cm_b.matrix, 2 * g[case + '_matrix']) and np.array_equal(ct_b.slots, 2 * g[case + '_counts']), 'two calls accumulate to the sum'
    r = ct_i.results_dict
    for k in ('r2', 'mae', 'rmse'):
        assert abs(r[f'metrics/count_{k}(0)'] - g[f'{case}_{k}'][0]) <= 1e-12


@pytest.mark.gpu
def test_untruncated_labels_and_other_thresholds_follow_the_restatement():
    """trunc_labels=False and thresholds other than the defaults, on the fork's own nc = 2 (margins re-checked for these settings)."""
    from mgdt_yolo_amd import ops
    c = _batch('c2')
    conf, iou = 0.4, 0.3
    want_m, want_k = np.zeros((3, 3), np.int64), np.zeros((2, 10), np.int64)
    for det, lab in images('c2'):
        assert min(R.confusion_margins(det, lab, conf, iou)[::2]) >= R.NEAR_IOU and R.counting_margins(det, lab, 2, conf, iou, False)[0] >= R.NEAR_IOU
        if lab.shape[0]:
            want_m += R.confusion(det, lab, 2, conf, iou) if det.shape[0] else R.confusion_none(lab[:, 0], 2)
        want_k += R.counting(det, lab, 2, conf, iou, trunc=False)
    m = torch.zeros(3, 3, dtype=torch.int32, device=DEV)
    k = torch.zeros(2, ops.COUNT_SLOTS, dtype=torch.int64, device=DEV)
    ops.val_confusion(c['det'], c['ndet'], c['lab'], c['nlab'], 2, matrix=m, counts=k, cm_conf=conf, cm_iou=iou, cnt_conf=conf, cnt_iou=iou, trunc_labels=False)
    assert np.array_equal(m.cpu().numpy(), want_m) and np.array_equal(k.cpu().numpy(), want_k)


def _validator_batch():
    """The synthetic batch of test_validator_update_metrics_and_stats (tests/golden/inputs.py:val_match_inputs) with one image without detections and
    one without labels added -> (preds, batch, labels per class); 60 detections by 9 labels in the other images."""
    import inputs as GI
    B, H, W, nc = 5, 384, 640, 5
    ori = [(720, 1200), (384, 640), (500, 700), (384, 640), (384, 640)]
    preds, cls_l, box_l, idx_l, rp, nlab = [], [], [], [], [], np.zeros(nc, np.int64)
    for si in range(B):
        gain = min(H / ori[si][0], W / ori[si][1])
        rp.append(((gain, gain), ((W - ori[si][1] * gain) / 2, (H - ori[si][0] * gain) / 2)))
        det, lab = GI.val_match_inputs(40 + si, 0 if si == 3 else 60, 0 if si == 4 else 9)
        det[:, [0, 2]] = det[:, [0, 2]].clip(0, W - 1); det[:, [1, 3]] = det[:, [1, 3]].clip(0, H - 1)
        lab[:, [1, 3]] = lab[:, [1, 3]].clip(1, W - 2); lab[:, [2, 4]] = lab[:, [2, 4]].clip(1, H - 2)
        preds.append(torch.from_numpy(det).to(DEV))
        xywh = np.stack([(lab[:, 1] + lab[:, 3]) / 2 / W, (lab[:, 2] + lab[:, 4]) / 2 / H, (lab[:, 3] - lab[:, 1]) / W, (lab[:, 4] - lab[:, 2]) / H], 1).astype(np.float32)
        cls_l.append(lab[:, :1]); box_l.append(xywh); idx_l.append(np.full(len(lab), si, np.float32))
        nlab += np.bincount(lab[:, 0].astype(int), minlength=nc)
    batch = dict(img=torch.zeros(B, 3, H, W, dtype=torch.uint8, device=DEV), cls=torch.from_numpy(np.concatenate(cls_l)),
                 bboxes=torch.from_numpy(np.concatenate(box_l)), batch_idx=torch.from_numpy(np.concatenate(idx_l)), ori_shape=ori, ratio_pad=rp)
    return preds, batch, nlab


@pytest.mark.gpu
def test_detection_validator_adds_the_new_keys_and_leaves_the_map_dict_unchanged():
    """update_metrics + get_stats on the synthetic batch of test_validator_update_metrics_and_stats (tests/golden/inputs.py:val_match_inputs), with
    and without the new statistics; one image without detections and one without labels are added."""
    from mgdt_yolo_amd.yolo.utils.metrics import ConfusionMatrix
    from mgdt_yolo_amd.yolo.v8.detect import DetectionValidator
    B, nc = 5, 5
    preds, batch, nlab = _validator_batch()
    res = {}
    for on in (False, True):
        v = DetectionValidator(DEV)
        v.init_metrics(nc=nc, confusion=on, counting=on) if on else v.init_metrics(nc=nc)
        v.update_metrics(preds, batch)
        res[on] = v.get_stats()
    assert list(res[False]) == MAP_KEYS, 'with both off the dict has exactly the keys it had'
    assert all(res[True][k] == res[False][k] for k in MAP_KEYS) and 0 < res[True]['metrics/mAP50-95(B)'] < 1
    extra = set(res[True]) - set(MAP_KEYS)
    assert extra == {'confusion_matrix'} | {f'metrics/count_{k}({c})' for c in range(nc) for k in ('tp', 'fp', 'fn', 'gt', 'pred', 'mae', 'rmse', 'r2')}
    cm = res[True]['confusion_matrix']
    assert isinstance(cm, ConfusionMatrix)
    m = cm.matrix
    assert m.shape == (nc + 1, nc + 1) and np.array_equal(m[:, :nc].sum(0), nlab), 'every label adds exactly one entry to its column'
    assert np.trace(m[:nc, :nc]) >= 10 and m[:nc, nc].sum() > 0 and m[nc, :nc].sum() >= 9      # image 3 has no detections: its 9 labels are background
    s = v.count_metrics.slots
    assert (s[:, 0] == B).all() and np.array_equal(s[:, 1], nlab) and np.array_equal(s[:, 7] + s[:, 9], nlab) and s[:, 7].sum() >= 10
    assert (s[:, 8] >= 0).all() and (s[:, 8] <= s[:, 2]).all()
    assert all(res[True][f'metrics/count_gt({c})'] == float(nlab[c]) for c in range(nc))


@pytest.mark.gpu
@pytest.mark.parametrize('extras', [False, True], ids=['extras_off', 'extras_on'])
def test_detection_validator_batch_path_equals_the_per_image_api(extras):
    """update_metrics matches the whole batch in one launch and slices per image; the expectation is built image by image from the per-image public
    API on the same native-space tensors: `_process_batch`, ConfusionMatrix.process_batch, CountMetrics.process_batch.  The batch of `_validator_batch`
    (one image without detections, one without labels) with the label rows shuffled, so that batch_idx is unsorted.  Everything is EQUAL."""
    from mgdt_yolo_amd.yolo.utils import ops as uops
    from mgdt_yolo_amd.yolo.utils.metrics import ConfusionMatrix, CountMetrics
    from mgdt_yolo_amd.yolo.v8.detect import DetectionValidator
    nc = 5
    preds, batch, _ = _validator_batch()
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(batch['batch_idx'])))
    batch = dict(batch, cls=batch['cls'][perm], bboxes=batch['bboxes'][perm], batch_idx=batch['batch_idx'][perm])
    assert bool((batch['batch_idx'][1:] < batch['batch_idx'][:-1]).any()), 'batch_idx is unsorted'
    H, W = batch['img'].shape[2:]
    v = DetectionValidator(DEV)
    v.init_metrics(nc=nc, confusion=extras, counting=extras)
    # ---- image by image
    want, seen, cm, ct = [], 0, ConfusionMatrix(nc), CountMetrics(nc)
    whwh = torch.tensor((W, H, W, H), dtype=torch.float32, device=DEV)
    for si, pred in enumerate(preds):
        idx = batch['batch_idx'] == si
        cls, bbox = batch['cls'][idx].to(DEV), batch['bboxes'][idx].to(DEV)
        shape, rp = batch['ori_shape'][si], batch['ratio_pad'][si]
        seen += 1
        predn = pred.clone()
        tbox = uops.xywh2xyxy(bbox.contiguous()) * whwh if len(cls) else torch.zeros(0, 4, device=DEV)
        if len(pred):
            uops.scale_boxes((H, W), predn, shape, ratio_pad=rp)
        if len(cls):
            uops.scale_boxes((H, W), tbox, shape, ratio_pad=rp)
        labelsn = torch.cat((cls, tbox), 1)
        if len(cls):                                                  # the matrix skips an image without labels, the counters count it
            cm.process_batch(predn if len(pred) else None, labelsn)
        ct.process_batch(predn if len(pred) else None, labelsn)
        if len(pred):
            want.append((v._process_batch(predn, labelsn), pred[:, 4], pred[:, 5], cls[:, 0]))
        elif len(cls):
            want.append((torch.zeros(0, 10, dtype=torch.bool, device=DEV), torch.zeros(0, device=DEV), torch.zeros(0, device=DEV), cls[:, 0]))
    assert [len(p) for p in preds] == [60, 60, 60, 0, 60] and [len(w[3]) for w in want] == [9, 9, 9, 9, 0]
    # ---- the batch
    v.update_metrics(preds, batch)
    assert v.seen == seen == 5 and len(v.stats) == len(want)
    for si, (got, exp) in enumerate(zip(v.stats, want)):
        assert len(got) == 4
        for k, (g, e) in enumerate(zip(got, exp)):
            assert g.dtype == e.dtype and g.shape == e.shape and torch.equal(g, e), (si, k)
    assert any(bool(w[0].any()) for w in want)
    if extras:
        assert np.array_equal(v.confusion_matrix.matrix, cm.matrix) and cm.matrix.sum() > 0
        assert np.array_equal(v.count_metrics.slots, ct.slots) and (ct.slots[:, 0] == 5).all()
    else:
        assert v.confusion_matrix is None and v.count_metrics is None
