"""Seeded inputs and an int64 / float64 restatement for the segmentation-validation tests (tests/test_segval.py, tests/golden/gen_segval.py).

Inputs are re-created from seeds (numpy Generator: the same bits everywhere), so the fixture tests/golden/segval_NN.npz holds results only: what the
reference's own `mask_iou`, `SegmentationValidator._process_batch` and `ap_per_class` returned on them.

The restatement: intersections and areas as int64 counts, iou = float32(inter) / ((float32(area_gt) + float32(area_pred)) - float32(inter) + eps)
rounded once per operation (numpy float32), which is what a float32 matmul of 0 / 1 values gives while every sum stays below 2^24; matching by the
rule documented in csrc/nms.hip (per level: a detection chooses its best label among {iou >= level, same class}, a label keeps the lowest-index
detection that chose it; ties to the lower label index); ground-truth resampling with float64 bilinear values and the band |v - 0.5| <= 1e-5."""
import glob
import os

import numpy as np

IOUV = np.linspace(0.5, 0.95, 10).astype(np.float32)       # == torch.linspace(0.5, 0.95, 10) (checked by the generator)
NC = 5
RESAMPLE_BAND = 1e-5

# name -> (H, W), [(n_det, n_lab) per image]; ground truth is an index map, the instance form is derived from it (idx == j + 1)
CASES = {
    'b160': ((160, 160), [(17, 12), (300, 12), (0, 5), (9, 0), (1, 1)]),
    'b40': ((40, 56), [(17, 12), (1, 1), (40, 12)]),
    'many': ((160, 160), [(300, 255)]),
    'inst40': ((160, 160), [(300, 40), (17, 1)]),
    'big640': ((640, 640), [(17, 12)]),
}
MATCH_CASES = ('b160', 'b40', 'many', 'inst40', 'big640')
ASYM_CASES = {'asym_inst': ((96, 128), 17, 12), 'asym_idx': ((160, 160), 9, 7)}
CHAIN_TAG, CHAIN_SHAPE = 'yolov8_seg_n_2x160x224', (160, 224)      # the `val` rows and protos tests/golden/seg_NN.npz holds
RESAMPLE_CASES = {'r4': ((40, 56), (160, 224), 9), 'r3': ((40, 56), (120, 168), 9), 'r2p6': ((50, 40), (130, 104), 7)}     # ratio 4 (exact), 3 and 2.6


def _shape(r, h, w, scale):
    """One seeded ellipse or rectangle as a bool (h, w) mask."""
    cy, cx = r.uniform(0, h), r.uniform(0, w)
    ry, rx = r.uniform(0.04, scale) * h + 1.5, r.uniform(0.04, scale) * w + 1.5
    ys, xs = np.mgrid[0:h, 0:w]
    if r.random() < 0.5:
        return ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0
    return (np.abs(ys - cy) <= ry) & (np.abs(xs - cx) <= rx)


def _shift(m, dy, dx):
    out = np.zeros_like(m)
    h, w = m.shape
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = m[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def _dilate(m):
    out = m.copy()
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        out |= _shift(m, dy, dx)
    return out


def _bbox(m, r, jitter):
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return np.array([1.0, 1.0, 3.0, 3.0], np.float32) + np.float32(r.uniform(0, 4))
    b = np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float64)
    return (b + r.uniform(-jitter, jitter, 4)).astype(np.float32)


def image_inputs(seed, h, w, nd, nl):
    """-> idx (h, w) uint8 index map, pred (nd, h, w) uint8, det (nd, 6) float32 [box, conf, cls], lab (nl, 5) float32 [cls, box]."""
    r = np.random.default_rng([seed, h, w, nd, nl])
    scale = 0.22 if nl <= 40 else 0.07
    idx = np.zeros((h, w), np.uint8)
    for j in range(nl):
        idx[_shape(r, h, w, scale)] = j + 1
    lab = np.zeros((nl, 5), np.float32)
    for j in range(nl):
        lab[j, 0] = r.integers(0, NC)
        lab[j, 1:] = _bbox(idx == j + 1, r, 0.0)
    pred = np.zeros((nd, h, w), np.uint8)
    det = np.zeros((nd, 6), np.float32)
    order = r.permutation(nl) if nl else np.zeros(0, int)
    for d in range(nd):
        if nl and r.random() < 0.6:
            j = int(order[d % nl])
            m = idx == j + 1
            for _ in range(int(r.integers(0, 3))):
                m = _dilate(m)
            m = _shift(m, int(r.integers(-3, 4)), int(r.integers(-3, 4)))
            m = m ^ ((r.random((h, w)) < r.uniform(0.0, 0.2)) & _dilate(m))      # seeded speckle: no two copies of a label share an IoU
            cls = lab[j, 0] if r.random() < 0.85 else (lab[j, 0] + 1) % NC
            box = _bbox(m, r, 2.5)
        else:
            m = _shape(r, h, w, scale)
            cls = r.integers(0, NC)
            box = _bbox(m, r, 2.5)
        pred[d] = m
        det[d, :4], det[d, 5] = box, cls
    det[:, 4] = np.sort(r.uniform(0.001, 1.0, nd).astype(np.float32))[::-1]
    return idx, pred, det, lab


def case_inputs(name):
    (h, w), images = CASES[name]
    return [image_inputs(1000 + 17 * k + len(name), h, w, nd, nl) for k, (nd, nl) in enumerate(images)]


def instances(idx, nl):
    return (idx[None] == (np.arange(nl, dtype=np.int64)[:, None, None] + 1)).astype(np.uint8)


def _asym_trial(name, trial):
    (h, w), nd, nl = ASYM_CASES[name]
    r = np.random.default_rng([77, len(name), nd, nl, trial])
    pred = (r.random((nd, h, w)) < np.linspace(0.15, 0.85, nd)[:, None, None]).astype(np.uint8)
    if name == 'asym_idx':
        p = np.arange(1, nl + 2, dtype=np.float64)
        idx = r.choice(nl + 1, size=(h, w), p=p / p.sum()).astype(np.uint8)
        return instances(idx, nl), pred, idx
    gt = (r.random((nl, h, w)) < np.linspace(0.8, 0.2, nl)[:, None, None]).astype(np.uint8)
    return gt, pred, None


def asym_inputs(name):
    """Every label and every detection with its own pixel density: -> gt (nl, h, w) uint8 instance masks (for 'asym_idx' derived from the returned
    index map, else overlapping and idx None), pred (nd, h, w) uint8, idx.  The first seeded trial whose areas are distinct and whose
    intersections are pairwise distinct is taken."""
    for trial in range(1000):
        gt, pred, idx = _asym_trial(name, trial)
        g, p = gt.reshape(gt.shape[0], -1).astype(np.int64), pred.reshape(pred.shape[0], -1).astype(np.int64)
        inter = g @ p.T
        if len(np.unique(g.sum(1))) == g.shape[0] and len(np.unique(p.sum(1))) == p.shape[0] and len(np.unique(inter)) == inter.size:
            return gt, pred, idx
    raise AssertionError(name)


def resample_inputs(name):
    (h, w), out, nl = RESAMPLE_CASES[name]
    r = np.random.default_rng([55, h, w, nl])
    idx = np.zeros((h, w), np.uint8)
    for j in range(nl):
        idx[_shape(r, h, w, 0.3)] = j + 1
    return idx, nl, out


# ------------------------------------------------------------------------------------------------ restatement
def mask_iou_exact(gt, pred, eps=1e-7):
    """gt (nl, ...) and pred (nd, ...) 0 / 1 arrays -> (nl, nd) float32 from int64 counts."""
    g = gt.reshape(gt.shape[0], -1).astype(np.int64)
    p = pred.reshape(pred.shape[0], -1).astype(np.int64)
    inter = (g @ p.T).astype(np.float32)
    union = (g.sum(1).astype(np.float32)[:, None] + p.sum(1).astype(np.float32)[None]) - inter
    return inter / (union + np.float32(eps))


def box_iou_f32(lab_boxes, det_boxes, eps=1e-7):
    """metrics.py:52-72 in float32, operation by operation."""
    a, b = lab_boxes.astype(np.float32), det_boxes.astype(np.float32)
    wh = np.clip(np.minimum(a[:, None, 2:], b[None, :, 2:]) - np.maximum(a[:, None, :2], b[None, :, :2]), 0, None)
    inter = wh[..., 0] * wh[..., 1]
    area_a = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None]
    area_b = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None]
    return inter / (area_a + area_b - inter + np.float32(eps))


def match(iou, lab_cls, det_cls, iouv=IOUV):
    """iou (nl, nd) float32 -> correct (nd, T) bool."""
    nl, nd = iou.shape
    correct = np.zeros((nd, len(iouv)), bool)
    if nl == 0 or nd == 0:
        return correct
    same = lab_cls[:, None] == det_cls[None]
    for t, level in enumerate(iouv):
        cand = np.where((iou >= level) & same, iou, np.float32(-1))
        best = cand.argmax(0)                                     # first maximum: the lower label index
        has = cand.max(0) >= 0
        taken = set()
        for d in range(nd):
            if has[d] and best[d] not in taken:
                taken.add(best[d])
                correct[d, t] = True
    return correct


def resample_values(mask, out):
    """One binary (h, w) mask -> float64 (oh, ow) values of F.interpolate(bilinear, align_corners=False) with float64 weights."""
    h, w = mask.shape
    oh, ow = out

    def taps(n_in, n_out):
        s = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, np.clip(s - i0, 0.0, 1.0)
    y0, y1, wy = taps(h, oh)
    x0, x1, wx = taps(w, ow)
    m = mask.astype(np.float64)
    top = m[y0][:, x0] * (1 - wx) + m[y0][:, x1] * wx
    bot = m[y1][:, x0] * (1 - wx) + m[y1][:, x1] * wx
    return top * (1 - wy)[:, None] + bot * wy[:, None]


def pack(mask_bool):
    return np.packbits(np.asarray(mask_bool, dtype=bool).reshape(-1))


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape).astype(bool)


def load_fixture():
    out = {}
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'segval_[0-9][0-9].npz'))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    assert out, 'tests/golden/segval_NN.npz are missing'
    return out
