"""Host restatements and seeded inputs for the validator statistics (mgdt_val_confusion_fwd): the confusion matrix and the counting metrics.

Restated here, in plain numpy / Python, never copied:
  - `confusion`: reference yolo/utils/metrics.py:225-253 (ConfusionMatrix.process_batch past the `detections is None` branch): the confidence filter,
    box_iou in float32 with the reference's operation order, the IoU-descending sort followed by np.unique on the detection column and again on the
    label column, written as "each detection keeps its best label, each label the best detection among those that chose it", the `if n:` rule for
    predicted background; and :219-223 (`confusion_none`).
  - `counting`: reference nn/cal_counting_metrics.py:15-20 (the int() of label corners), :23-35 (the IoU helper: max(0, .) on both sides, 0 unless
    union > 0, Python floats), :58-71 and :77-88 (per-class lists, true and predicted counts per image), :90-121 (first matching prediction per
    label in order, a matched prediction is not retired, FP = predictions - distinct matched), for nc classes instead of two.  The script cannot
    run (hard-coded paths, cv2, sklearn, a YOLO object); `r2` writes out sklearn.metrics.r2_score as the script uses it (:125), by hand in float64.
Inputs of tests/golden/confusion_00.npz come from seeds: (case, image index, salt) -> boxes; the salt of every case is stored in the fixture.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FRAME = (256, 320)                 # height, width
CM_CONF, CM_IOU, CNT_CONF, CNT_IOU = 0.25, 0.45, 0.25, 0.5
NEAR_IOU, NEAR_CONF, NEAR_TIE = 1e-5, 1e-6, 1e-5
SLOTS = ('images', 'sum_t', 'sum_p', 'sum_tt', 'sum_tp', 'sum_d2', 'sum_abs', 'tp', 'fp', 'fn')

# case -> (nc, max_det of the batch layout, image specs).  An image spec: kind, labels, jittered detections per label, random detections.
CASES = {
    'c1': (1, 16, [('normal', 5, 1, 3), ('nodet', 4, 0, 0), ('nolab', 0, 0, 6), ('empty', 0, 0, 0), ('nomatch', 4, 0, 5)]),
    'c2': (2, 96, [('normal', 40, 1, 20), ('nodet', 7, 0, 0), ('nolab', 0, 0, 9), ('nomatch', 6, 0, 8), ('claims', 6, 1, 4)]),
    'c2q': (2, 24, [('det3lab', 3, 0, 2), ('lab3det', 1, 3, 2), ('empty', 0, 0, 0)]),
    'c80': (80, 300, [('normal', 256, 1, 44), ('normal', 1, 2, 38), ('normal', 30, 2, 15)]),       # 300 detections on 256 threads; nlab 256 and 1
    'c1000': (1000, 40, [('normal', 12, 1, 6), ('normal', 20, 1, 10), ('nodet', 3, 0, 0)]),
}


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, 'confusion_00.npz')))


# ------------------------------------------------------------------------------------------------ seeded inputs
def _boxes(rng, n, lo=10.0, hi=120.0, x0=0.0, x1=None):
    H, W = FRAME
    x1 = W if x1 is None else x1
    w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    cx, cy = rng.uniform(x0 + w / 2, np.maximum(x1 - w / 2, x0 + w / 2 + 1e-3)), rng.uniform(h / 2, H - h / 2)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)


def _jitter(rng, box, scale):
    """A copy of `box` (k, 4) moved and resized by up to `scale` of its size."""
    wh = np.concatenate([box[:, 2:] - box[:, :2]] * 2, 1)
    return box + rng.uniform(-scale, scale, box.shape) * wh


def image_inputs(case, index, salt):
    """-> det (nd, 6) float32 [x1, y1, x2, y2, conf, cls] in NMS order (confidence descending), lab (nl, 5) float32 [cls, x1, y1, x2, y2]."""
    nc, _, specs = CASES[case]
    kind, nl, jit, nrand = specs[index]
    rng = np.random.default_rng([sum(case.encode()), index, salt])
    H, W = FRAME
    half = kind == 'nomatch'
    if kind == 'det3lab':           # three labels around one box: one detection is a candidate of all three
        base = _boxes(rng, 1, 60, 110)
        lbox = _jitter(rng, np.repeat(base, 3, 0), 0.05)
        dbox = [_jitter(rng, base, 0.03)]
        dcls = [rng.integers(0, nc, 1)]
    else:
        lbox = _boxes(rng, nl, x1=W / 2 - 4 if half else None) if nl else np.zeros((0, 4))
        dbox, dcls = [], []
    lcls = rng.integers(0, nc, lbox.shape[0])
    if kind == 'det3lab':
        lcls[:] = dcls[0][0]       # same class: the counting part lets the one detection serve all three labels
    if kind == 'claims':            # also: the first two labels are near copies, so one detection serves two labels
        lbox[1] = _jitter(rng, lbox[0:1], 0.04)[0]
        lcls[1] = lcls[0]
    for _ in range(jit):
        if lbox.shape[0]:
            dbox.append(_jitter(rng, lbox, 0.12 if kind != 'lab3det' else 0.06))
            same = rng.random(lbox.shape[0]) < 0.8
            dcls.append(np.where(same, lcls, rng.integers(0, nc, lbox.shape[0])))
    if nrand:
        dbox.append(_boxes(rng, nrand, x0=W / 2 + 4 if half else 0.0))
        dcls.append(rng.integers(0, nc, nrand))
    if dbox:
        dbox, dcls = np.concatenate(dbox), np.concatenate(dcls)
        conf = np.sort(rng.uniform(0.05, 0.97, dbox.shape[0]))[::-1]
        perm = rng.permutation(dbox.shape[0])                # which box gets which rank
        det = np.concatenate([dbox[perm], conf[:, None], dcls[perm, None].astype(np.float64)], 1).astype(np.float32)
    else:
        det = np.zeros((0, 6), np.float32)
    lab = np.concatenate([lcls[:, None].astype(np.float64), lbox], 1).astype(np.float32)
    return det, lab


def case_inputs(case, salt):
    return [image_inputs(case, i, salt) for i in range(len(CASES[case][2]))]


def batch_layout(case, imgs, garbage=True):
    """The kernel's batch layout: det (B, max_det, 6), ndet, labels (B, max_lab, 5), nlab.  Rows past ndet / nlab hold boxes that WOULD match (copies
    of the image's labels with confidence 0.99 / of its detections), so reading one changes the result."""
    nc, max_det, _ = CASES[case]
    b = len(imgs)
    ndet, nlab = [d.shape[0] for d, _ in imgs], [l.shape[0] for _, l in imgs]
    max_lab = max(max(nlab), 1) + (3 if max(nlab) < 254 else 0)
    assert max(ndet) <= max_det
    det = np.zeros((b, max_det, 6), np.float32)
    lab = np.zeros((b, max_lab, 5), np.float32)
    for i, (d, l) in enumerate(imgs):
        if garbage:
            src = l if l.shape[0] else np.array([[0, 20, 20, 90, 90]], np.float32)
            rows = np.resize(np.arange(src.shape[0]), max_det)
            det[i, :, :4], det[i, :, 4], det[i, :, 5] = src[rows, 1:], 0.99, src[rows, 0]
            srcd = d if d.shape[0] else np.array([[20, 20, 90, 90, 0.9, 0]], np.float32)
            rows = np.resize(np.arange(srcd.shape[0]), max_lab)
            lab[i, :, 0], lab[i, :, 1:] = srcd[rows, 5], srcd[rows, :4]
        det[i, :d.shape[0]], lab[i, :l.shape[0]] = d, l
    return det, np.array(ndet, np.int32), lab, np.array(nlab, np.int32)


# ------------------------------------------------------------------------------------------------ confusion matrix
def box_iou_f32(lab_boxes, det_boxes, eps=1e-7):
    """(nl, 4) x (nd, 4) -> (nl, nd), every operation rounded to float32 in the order of the reference's box_iou (labels first)."""
    a, b = lab_boxes.astype(np.float32)[:, None, :], det_boxes.astype(np.float32)[None, :, :]
    iw = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), np.float32(0))
    ih = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), np.float32(0))
    inter = iw * ih
    return inter / ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter + np.float32(eps))


def confusion(det, lab, nc, conf=CM_CONF, iou_thres=CM_IOU):
    """-> (nc + 1, nc + 1) int64 of one image, detections given (possibly none)."""
    m = np.zeros((nc + 1, nc + 1), np.int64)
    keep = det[:, 4] > np.float32(conf)
    d = det[keep]
    dc, lc = d[:, 5].astype(int), lab[:, 0].astype(int)
    iou = box_iou_f32(lab[:, 1:], d[:, :4])
    cand = iou > np.float32(iou_thres)
    choice = np.full(d.shape[0], -1)
    for j in range(d.shape[0]):                      # pass 1: the best candidate label of each detection
        if cand[:, j].any():
            choice[j] = int(np.argmax(np.where(cand[:, j], iou[:, j], -1.0)))
    winner = np.full(lab.shape[0], -1)
    for i in range(lab.shape[0]):                    # pass 2: the best detection among those that chose the label
        js = np.nonzero(choice == i)[0]
        if js.size:
            winner[i] = int(js[np.argmax(iou[i, js])])
    any_match = bool((winner >= 0).any())
    for i in range(lab.shape[0]):
        m[dc[winner[i]] if winner[i] >= 0 else nc, lc[i]] += 1
    if any_match:
        for j in range(d.shape[0]):
            if not (winner == j).any():
                m[dc[j], nc] += 1
    return m


def confusion_none(lab_cls, nc):
    m = np.zeros((nc + 1, nc + 1), np.int64)
    for c in np.asarray(lab_cls).astype(int):
        m[nc, c] += 1
    return m


def confusion_margins(det, lab, conf=CM_CONF, iou_thres=CM_IOU):
    """-> (min |iou - threshold|, min |conf - threshold|, min gap best / second best among a detection's candidates and among a label's choosers)."""
    d = det[det[:, 4] > np.float32(conf)]
    near_conf = float(np.abs(det[:, 4].astype(np.float64) - conf).min()) if det.shape[0] else np.inf
    if not (d.shape[0] and lab.shape[0]):
        return np.inf, near_conf, np.inf
    iou = box_iou_f32(lab[:, 1:], d[:, :4]).astype(np.float64)
    near_iou = float(np.abs(iou - iou_thres).min())
    cand = iou > iou_thres - NEAR_IOU
    gap = np.inf
    choice = np.full(d.shape[0], -1)
    for j in range(d.shape[0]):
        v = np.sort(iou[cand[:, j], j])
        if v.size:
            choice[j] = int(np.argmax(np.where(cand[:, j], iou[:, j], -1.0)))
        if v.size > 1:
            gap = min(gap, float(v[-1] - v[-2]))
    for i in range(lab.shape[0]):
        v = np.sort(iou[i, choice == i])
        if v.size > 1:
            gap = min(gap, float(v[-1] - v[-2]))
    return near_iou, near_conf, gap


# ------------------------------------------------------------------------------------------------ counting
def script_iou(b1, b2):
    xi1, yi1, xi2, yi2 = max(b1[0], b2[0]), max(b1[1], b2[1]), min(b1[2], b2[2]), min(b1[3], b2[3])
    inter = max(0, xi2 - xi1) * max(0, yi2 - yi1)
    union = (b1[2] - b1[0]) * (b1[3] - b1[1]) + (b2[2] - b2[0]) * (b2[3] - b2[1]) - inter
    return inter / union if union > 0 else 0


def _count_lists(det, lab, nc, conf, trunc):
    true = [[] for _ in range(nc)]
    pred = [[] for _ in range(nc)]
    for row in lab.tolist():
        box = [int(v) for v in row[1:]] if trunc else row[1:]
        true[int(row[0])].append(box)
    for row in det.tolist():
        if row[4] > float(np.float32(conf)):
            pred[int(row[5])].append(row[:4])
    return true, pred


def counting(det, lab, nc, conf=CNT_CONF, iou=CNT_IOU, trunc=True):
    """-> (nc, 10) int64 slots of one image (SLOTS)."""
    out = np.zeros((nc, len(SLOTS)), np.int64)
    true, pred = _count_lists(det, lab, nc, conf, trunc)
    for c in range(nc):
        tp = fn = 0
        matched = set()
        for g in true[c]:
            found = False
            for i, p in enumerate(pred[c]):
                if script_iou(g, p) > iou:
                    tp += 1
                    found = True
                    matched.add(i)
                    break
            if not found:
                fn += 1
        t, p = len(true[c]), len(pred[c])
        out[c] = (1, t, p, t * t, t * p, (t - p) ** 2, abs(t - p), tp, p - len(matched), fn)
    return out


def counting_margins(det, lab, nc, conf=CNT_CONF, iou=CNT_IOU, trunc=True):
    """-> (min |iou - threshold| over same-class pairs, min |conf - threshold|)."""
    true, pred = _count_lists(det, lab, nc, -1.0, trunc)
    near = min([abs(script_iou(g, p) - iou) for c in range(nc) for g in true[c] for p in pred[c]], default=np.inf)
    return near, (float(np.abs(det[:, 4].astype(np.float64) - conf).min()) if det.shape[0] else np.inf)


def r2(true_counts, pred_counts):
    """sklearn.metrics.r2_score(y_true, y_pred) behind the script's guard, float64."""
    y, f = np.asarray(true_counts, np.float64), np.asarray(pred_counts, np.float64)
    if y.size < 2:
        return 0.0
    ss_res, ss_tot = float(((y - f) ** 2).sum()), float(((y - y.mean()) ** 2).sum())
    if ss_tot == 0.0:
        return 1.0 if ss_res == 0.0 else 0.0
    return 1.0 - ss_res / ss_tot


def errors(true_counts, pred_counts):
    """-> MAE, RMSE of the per-image counts, float64."""
    y, f = np.asarray(true_counts, np.float64), np.asarray(pred_counts, np.float64)
    return float(np.abs(f - y).mean()), float(np.sqrt(((f - y) ** 2).mean()))
