"""Seeded inputs and a float64 restatement for the pose-validation tests (tests/test_poseval.py, tests/golden/gen_poseval.py).

Inputs are re-created from seeds (numpy Generator: the same bits everywhere; the `chain` case starts from the validator NMS rows that
tests/golden/pose_NN.npz already holds), so the fixture tests/golden/poseval_00.npz holds results only: what the reference's own `kpt_iou`,
`PoseValidator._process_batch`, `scale_boxes` / `scale_coords` and `ap_per_class` returned on them.

The restatement: `kpt_iou` (yolo/utils/metrics.py:150-169) in float64 on the float32 inputs, expression for expression; area = w * h * 0.53 in float32,
operation by operation (val.py:123); matching by `segval_ref.match` (the rule documented in csrc/nms.hip)."""
import glob
import os

import numpy as np

from segval_ref import IOUV, box_iou_f32, match  # noqa: F401  (re-exported for the tests)

FRAME = (160, 224)                 # (H, W) of the synthetic cases and of the chain's letter-boxed input
JITTER = (0.01, 0.03, 0.08, 0.2)   # label keypoint jitter as a share of sqrt(box area)
NEAR = 1e-5                        # a float64 OKS this close to a level may match either way on another float32 evaluation order
OKS_SIGMA = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0

# name -> (nkpt, pred_ndim), classes, [(n_det, n_lab) per image]
CASES = {
    't1': ((17, 3), 1, [(1, 1), (0, 4), (65, 0)]),
    't2': ((17, 3), 2, [(63, 17), (300, 33)]),
    'k5': ((5, 2), 1, [(40, 6), (100, 20)]),
}
CHAIN_TAG = 'yolov8_pose_n_2x96x160'
CHAIN_LABELS = 12
# letter-box settings of the chain: (ori_shape, ratio_pad) - 134x224 padded into 160x224 (gain 1), and a gain != 1 computed from ori_shape alone
CHAIN_BOXES = {'pad': ((134, 224), ((1.0, 1.0), (0.0, 13.0))), 'gain': ((120, 200), None)}


def sigma_of(kpt_shape):
    """val.py:48-51."""
    return OKS_SIGMA if tuple(kpt_shape) == (17, 3) else np.ones(kpt_shape[0]) / kpt_shape[0]


def labels_from(r, det, kp, nl, nc, special, frame=FRAME):
    """nl labels: every other detection's keypoints with Gaussian jitter and its box jittered by a few pixels, the last two matching nothing.
    -> lab (nl, 5) [cls, x1, y1, x2, y2], gk (nl, nkpt, 3) float32 with visibility 0 / 1 / 2 (about a quarter invisible)."""
    nd, nkpt = kp.shape[0], kp.shape[1]
    H, W = frame
    lab = np.zeros((nl, 5), np.float32)
    gk = np.zeros((nl, nkpt, 3), np.float32)
    n_match = (nl - 2 if nl >= 4 else nl) if nd else 0        # two labels of an image match nothing (an image with fewer than 4 labels: none)
    for j in range(nl):
        if j < n_match and 2 * j < nd:
            d = 2 * j
            box = det[d, :4].astype(np.float64) + r.uniform(-3, 3, 4)
            side = np.sqrt(max((box[2] - box[0]) * (box[3] - box[1]), 1.0))
            xy = kp[d, :, :2].astype(np.float64) + r.normal(0.0, JITTER[j % 4] * side, (nkpt, 2))
            cls = det[d, 5] if (nc == 1 or r.random() < 0.8) else (det[d, 5] + 1) % nc
        else:
            cx, cy, w, h = r.uniform(30, W - 30), r.uniform(30, H - 30), r.uniform(15, 60), r.uniform(15, 60)
            box = np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
            xy = np.stack([r.uniform(box[0], box[2], nkpt), r.uniform(box[1], box[3], nkpt)], 1)
            cls = r.integers(0, nc)
        vis = r.choice([0.0, 1.0, 2.0], size=nkpt, p=[0.25, 0.25, 0.5])
        lab[j, 0], lab[j, 1:] = cls, box
        gk[j, :, :2], gk[j, :, 2] = xy, vis
    if special and nl >= 8:
        gk[3, :, 2] = 0.0                                  # a label with no visible keypoint
        lab[5, 3], lab[5, 4] = lab[5, 1], lab[5, 2]        # a zero-area box
    return lab, gk


def image_inputs(seed, nd, nl, kpt_shape, nc, special=False):
    """-> det (nd, 6) float32 [box, conf, cls], kp (nd, nkpt, ndim) float32 inside the frame, lab (nl, 5), gk (nl, nkpt, 3)."""
    nkpt, ndim = kpt_shape
    H, W = FRAME
    r = np.random.default_rng([seed, nd, nl, nkpt, ndim])
    det = np.zeros((nd, 6), np.float32)
    kp = np.zeros((nd, nkpt, ndim), np.float32)
    for d in range(nd):
        w, h = r.uniform(20, 90), r.uniform(20, 90)
        cx, cy = r.uniform(w / 2, W - w / 2), r.uniform(h / 2, H - h / 2)
        det[d, :4] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
        kp[d, :, 0] = r.uniform(cx - w / 2, cx + w / 2, nkpt)
        kp[d, :, 1] = r.uniform(cy - h / 2, cy + h / 2, nkpt)
        if ndim == 3:
            kp[d, :, 2] = r.random(nkpt)
        det[d, 5] = r.integers(0, nc)
    det[:, 4] = np.sort(r.uniform(0.001, 1.0, nd).astype(np.float32))[::-1]
    lab, gk = labels_from(r, det, kp, nl, nc, special)
    return det, kp, lab, gk


def case_inputs(name):
    kpt_shape, nc, images = CASES[name]
    return [image_inputs(2000 + 31 * k + len(name), nd, nl, kpt_shape, nc, special=(name == 't2')) for k, (nd, nl) in enumerate(images)]


def chain_inputs(pose_fixture):
    """The `val` NMS rows of pose_NN.npz (in the 96x160 frame of the model that made them, here taken as detections of a 160x224 letter-boxed
    input) + seeded labels in the dataloader's form: -> rows [(n_i, 57)], batch dict pieces (cls (L, 1), bboxes (L, 4) xywh normalised,
    keypoints (L, 17, 3) normalised, batch_idx (L,)) as float32 numpy."""
    H, W = FRAME
    rows = [np.asarray(pose_fixture[f'{CHAIN_TAG}_nms_val_{i}'], np.float32) for i in range(2)]
    cls, bboxes, kpts, bidx = [], [], [], []
    for i, rw in enumerate(rows):
        r = np.random.default_rng([93, i])
        kp = rw[:, 6:].reshape(-1, 17, 3)
        lab, gk = labels_from(r, rw[:, :6], kp, CHAIN_LABELS, 1, False)
        x1, y1, x2, y2 = (lab[:, k].astype(np.float64) for k in range(1, 5))
        cls.append(lab[:, 0:1])
        bboxes.append(np.stack([(x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H], 1).astype(np.float32))
        g = gk.astype(np.float64)
        g[..., 0] /= W
        g[..., 1] /= H
        kpts.append(g.astype(np.float32))
        bidx.append(np.full(CHAIN_LABELS, i, np.float32))
    return rows, dict(cls=np.concatenate(cls), bboxes=np.concatenate(bboxes), keypoints=np.concatenate(kpts), batch_idx=np.concatenate(bidx))


# ------------------------------------------------------------------------------------------------ restatement
def letterbox(in_shape, ori_shape, ratio_pad):
    """-> gain, box pad (x, y), keypoint pad (x, y) as Python floats: scale_boxes rounds the padding it computes (ops.py:104-108), scale_coords does
    not (ops.py:653-655); a given ratio_pad is used as it is by both."""
    if ratio_pad is not None:
        return ratio_pad[0][0], tuple(ratio_pad[1]), tuple(ratio_pad[1])
    gain = min(in_shape[0] / ori_shape[0], in_shape[1] / ori_shape[1])
    pad = (in_shape[1] - ori_shape[1] * gain) / 2, (in_shape[0] - ori_shape[0] * gain) / 2
    return gain, (round(pad[0] - 0.1), round(pad[1] - 0.1)), pad


def scale_xy_f32(xy, gain, pad, ori_shape):
    """(..., >= 2k) float32 with x at even and y at odd positions of the last axis -> ((v - pad) / gain) clipped to the image, float32 per operation."""
    out = xy.astype(np.float32).copy()
    g = np.float32(gain)
    out[..., 0::2] = np.clip((out[..., 0::2] - np.float32(pad[0])) / g, np.float32(0), np.float32(ori_shape[1]))
    out[..., 1::2] = np.clip((out[..., 1::2] - np.float32(pad[1])) / g, np.float32(0), np.float32(ori_shape[0]))
    return out


def scale_boxes_f32(in_shape, boxes, ori_shape, ratio_pad=None):
    gain, bpad, _ = letterbox(in_shape, ori_shape, ratio_pad)
    return scale_xy_f32(boxes[:, :4], gain, bpad, ori_shape)


def scale_coords_f32(in_shape, coords, ori_shape, ratio_pad=None):
    """coords (..., 2 | 3): x / y scaled and clipped, a visibility column untouched."""
    gain, _, kpad = letterbox(in_shape, ori_shape, ratio_pad)
    out = coords.astype(np.float32).copy()
    out[..., :2] = scale_xy_f32(out[..., :2], gain, kpad, ori_shape)
    return out


def native_labels(in_shape, cls, bboxes, keypoints, ori_shape, ratio_pad):
    """val.py:86-95 for one image's labels in the dataloader's form -> labelsn (nl, 5), tkpts (nl, nkpt, 3) in native space, float32."""
    H, W = in_shape
    b = bboxes.astype(np.float32)
    half = b[:, 2:] / np.float32(2)
    xyxy = np.concatenate([b[:, :2] - half, b[:, :2] + half], 1) * np.array([W, H, W, H], np.float32)
    tk = keypoints.astype(np.float32) * np.array([W, H, 1], np.float32)
    return (np.concatenate([cls.reshape(-1, 1).astype(np.float32), scale_boxes_f32(in_shape, xyxy, ori_shape, ratio_pad)], 1),
            scale_coords_f32(in_shape, tk, ori_shape, ratio_pad))


def area_f32(lab):
    """val.py:123 in float32: (x2 - x1) * (y2 - y1) * 0.53, rounded after every operation."""
    lab = lab.astype(np.float32)
    return ((lab[:, 3] - lab[:, 1]) * (lab[:, 4] - lab[:, 2])) * np.float32(0.53)


def kpt_iou64(gk, pk, area, sigma, eps=1e-7):
    """metrics.py:150-169 in float64: gk (N, nkpt, 3), pk (M, nkpt, 2 | 3), area (N,) -> (N, M).  The denominator is the reference's for every input
    type: an integer count plus a Python float is a float32 tensor, so count + eps is the count itself for a count >= 1 (and eps for 0)."""
    gk, pk, area = gk.astype(np.float64), pk.astype(np.float64), area.astype(np.float64)
    sigma = np.asarray(sigma, np.float64)
    d = (gk[:, None, :, 0] - pk[None, :, :, 0]) ** 2 + (gk[:, None, :, 1] - pk[None, :, :, 1]) ** 2
    mask = gk[..., 2] != 0
    e = d / (2 * sigma) ** 2 / (area[:, None, None] + eps) / 2
    return (np.exp(-e) * mask[:, None]).sum(-1) / (mask.sum(-1).astype(np.float32) + np.float32(eps))[:, None].astype(np.float64)


def near_level(oks64, lab_cls, det_cls, band=NEAR):
    """(nd,) bool: detections with a same-class candidate whose float64 OKS lies within `band` of a level of IOUV."""
    if oks64.size == 0:
        return np.zeros(oks64.shape[1], bool)
    close = (np.abs(oks64[:, :, None] - IOUV[None, None].astype(np.float64)) <= band).any(2)
    return (close & (lab_cls[:, None] == det_cls[None])).any(0)


def load_fixture():
    out = {}
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'poseval_[0-9][0-9].npz'))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    assert out, 'tests/golden/poseval_NN.npz are missing'
    return out
