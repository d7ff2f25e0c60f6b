"""Generate tests/golden/confusion_00.npz: confusion-matrix and counting fixtures (BUILD CONTAINER ONLY; the GPU box never runs this file).

    python tests/golden/gen_confusion.py

Same recipe as gen_cls.py: the reference's own `ConfusionMatrix(nc, task='detect')` (yolo/utils/metrics.py:176-264, through ref_import) is fed image
by image the way yolo/v8/detect/val.py:84-109 feeds it - `process_batch(None, cls)` for an image without detections, `process_batch(predn, labelsn)`
for one with detections and labels, nothing for one without labels - over the seeded inputs of tests/valstats_ref.py.  Stored per case: the salt
of the seeds, the matrix per image (int16) and in total, `tp_fp()`, and the counting slots per image and in total with the per-class MAE / RMSE /
R^2 of the direct float64 formulas; the counting numbers come from valstats_ref's plain-Python restatement of nn/cal_counting_metrics.py (the
script itself cannot run: hard-coded paths, cv2, sklearn, a YOLO object).
Conditions asserted here on the reference alone; the salt of a case is raised until they hold, and no image, label or detection is left out:
  (a) no pair's IoU within 1e-5 of the confusion or the counting threshold; (b) no confidence within 1e-6 of a confidence threshold;
  (c) best and second-best IoU among one detection's candidates, and among the detections that chose one label, at least 1e-5 apart (the
      reference's argsort is unstable: a tie has no defined answer).
Also asserted: the restatement valstats_ref.confusion equals the reference per image; every special image shows what it is there for (no pair over the
threshold but kept detections; one detection with three candidate labels that serves three labels; one label chosen by three detections; 300
detections; 256 labels and 1 label); image 0 of c2 has several dozen pairs over 0.45.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_import  # noqa: E402
import valstats_ref as R  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()


def conditions(case, imgs):
    nc = R.CASES[case][0]
    for i, (det, lab) in enumerate(imgs):
        near_iou, near_conf, gap = R.confusion_margins(det, lab)
        cnt_iou, cnt_conf = R.counting_margins(det, lab, nc)
        if near_iou < R.NEAR_IOU or cnt_iou < R.NEAR_IOU or near_conf < R.NEAR_CONF or cnt_conf < R.NEAR_CONF or gap < R.NEAR_TIE:
            return False
    return True


def shows(case, imgs):
    """Every special image shows what it is there for."""
    nc, max_det, specs = R.CASES[case]
    for (kind, nl, _, _), (det, lab) in zip(specs, imgs):
        kept = det[det[:, 4] > np.float32(R.CM_CONF)]
        iou = R.box_iou_f32(lab[:, 1:], kept[:, :4]) if kept.shape[0] and lab.shape[0] else np.zeros((lab.shape[0], kept.shape[0]), np.float32)
        cand = iou > np.float32(R.CM_IOU)
        slots = R.counting(det, lab, nc)
        if kind == 'nomatch' and not (kept.shape[0] >= 2 and not cand.any() and R.confusion(det, lab, nc)[:nc, nc].sum() == 0):
            return False
        if kind == 'det3lab' and not (cand.sum(0).max() == 3 and slots[:, 7].sum() == 3 and (slots[:, 2] - slots[:, 8]).sum() == 1):
            return False
        if kind == 'lab3det' and not (cand[0].sum() >= 3 and R.confusion(det, lab, nc)[:nc, nc].sum() >= 2):
            return False
        if kind == 'claims' and not (slots[:, 7].sum() > (slots[:, 2] - slots[:, 8]).sum() and cand.sum(0).max() >= 2):
            return False
        if kind == 'nodet' and det.shape[0]:
            return False
    if case == 'c2' and not (R.box_iou_f32(imgs[0][1][:, 1:], imgs[0][0][:, :4]) > 0.45).sum() >= 36:
        return False
    if case == 'c80' and not (imgs[0][0].shape[0] == max_det == 300 and imgs[0][1].shape[0] == 256 and imgs[1][1].shape[0] == 1):
        return False
    return True


def reference_matrices(nc, imgs):
    out = []
    for det, lab in imgs:
        cm = ns.metrics.ConfusionMatrix(nc=nc, conf=R.CM_CONF, iou_thres=R.CM_IOU, task='detect')
        d, l = torch.from_numpy(det.copy()), torch.from_numpy(lab.copy())
        if det.shape[0] == 0:
            if lab.shape[0]:
                cm.process_batch(detections=None, labels=l[:, 0])
        elif lab.shape[0]:
            cm.process_batch(d, l)
        m = cm.matrix
        assert m.shape == (nc + 1, nc + 1) and np.array_equal(m, np.round(m)) and m.max() < 32768
        out.append(m.astype(np.int16))
    return np.stack(out)


def main():
    arrs = {}
    for case, (nc, max_det, specs) in R.CASES.items():
        salt = 0
        while True:
            imgs = R.case_inputs(case, salt)
            if conditions(case, imgs) and shows(case, imgs):
                break
            salt += 1
            assert salt < 200, case
        per = reference_matrices(nc, imgs)
        for i, (det, lab) in enumerate(imgs):
            mine = R.confusion(det, lab, nc) if det.shape[0] else R.confusion_none(lab[:, 0], nc)
            assert np.array_equal(mine, per[i]), (case, i, 'the restatement differs from the reference')
        total = ns.metrics.ConfusionMatrix(nc=nc, conf=R.CM_CONF, iou_thres=R.CM_IOU, task='detect')
        total.matrix = per.astype(np.float64).sum(0)
        tp, fp = total.tp_fp()
        slots = np.stack([R.counting(det, lab, nc) for det, lab in imgs])
        t, p = slots[:, :, 1], slots[:, :, 2]
        arrs[case + '_salt'] = np.array(salt, np.int64)
        arrs[case + '_img_matrix'], arrs[case + '_matrix'] = per, per.astype(np.int64).sum(0)
        arrs[case + '_tp'], arrs[case + '_fp'] = np.asarray(tp, np.float64), np.asarray(fp, np.float64)
        arrs[case + '_img_counts'], arrs[case + '_counts'] = slots, slots.sum(0)
        arrs[case + '_r2'] = np.array([R.r2(t[:, c], p[:, c]) for c in range(nc)])
        err = np.array([R.errors(t[:, c], p[:, c]) for c in range(nc)])
        arrs[case + '_mae'], arrs[case + '_rmse'] = err[:, 0], err[:, 1]
        m = arrs[case + '_matrix']
        print(f'{case}: salt {salt}, images {len(imgs)}, matrix sum {int(m.sum())} diagonal {int(np.trace(m[:nc, :nc]))} background row {int(m[nc].sum())} '
              f'column {int(m[:, nc].sum())}, TP / FP / FN {slots.sum((0, 1))[7:].tolist()}')
    path = os.path.join(HERE, 'confusion_00.npz')
    np.savez_compressed(path, **arrs)
    sz = os.path.getsize(path)
    print(f'confusion_00: {len(arrs)} arrays, {sz / 1024:.1f} KiB')
    assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


if __name__ == '__main__':
    main()
