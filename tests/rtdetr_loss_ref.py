"""Restatements of the RT-DETR criterion and of the validator's row order in plain torch (reference vit/utils/ops.py:12-111, vit/utils/loss.py,
yolo/utils/loss.py:16-53, yolo/utils/metrics.py:75-128, vit/rtdetr/val.py:90-106), written from the formulas, not copied.  Every function computes
in the dtype of its inputs, so the same code gives the float64 truth and the CPU fp32 run whose distance to it sizes the fp32 bounds of the GPU
tests.  Also: the case table and the seeded inputs shared by the fixture generator (tests/golden/gen_rtdetr_loss.py) and the tests.  The inputs
are regenerated from the seeds (numpy's frozen RandomState stream), the fixtures hold their checksums."""
import glob
import os

import numpy as np
import torch

# tag -> nq, nc, layers, ground truths per image, criterion keywords, seed (the generator walks it until every gap is >= GAP_MIN and asserts the table's value)
CASES = {
    'a': dict(nq=300, nc=80, layers=7, groups=(7, 24), kw={}, seed=0),
    'b': dict(nq=100, nc=3, layers=3, groups=(0, 1, 5), kw={}, seed=0),          # an empty image, nq not a multiple of 64
    'c': dict(nq=100, nc=3, layers=3, groups=(0, 0, 0), kw={}, seed=0),          # no ground truth at all: focal branch, zero box losses
    'd': dict(nq=8, nc=1, layers=2, groups=(8,), kw={}, seed=0),                 # every query matched
    'e': dict(nq=100, nc=3, layers=3, groups=(0, 1, 5), kw=dict(use_uni_match=True, uni_match_ind=0), seed=0),
    'f': dict(nq=100, nc=3, layers=3, groups=(0, 1, 5), kw=dict(use_vfl=False), seed=0),
    'g': dict(nq=100, nc=3, layers=3, groups=(0, 1, 5), kw={}, seed=0, dn=dict(groups=2, layers=2)),      # + a denoising pass, two groups
}
GAP_MIN = 1e-3
COST_GAIN = dict(cls=2.0, bbox=5.0, giou=2.0)        # DETRLoss's matcher
LOSS_GAIN = dict(cls=1.0, bbox=5.0, giou=2.0)
ALPHA, GAMMA = 0.25, 2.0
VAL = dict(nq=(100, 300), nc=5, labels=(4, 6), ori_shape=((480, 640), (375, 500)), seed=0)      # case (i): two images, (h, w) each


def make_inputs(tag, seed=None):
    """float64 numpy inputs of a case: boxes (l, B, nq, 4), logits (l, B, nq, nc), gt_boxes (G, 4), gt_cls (G,) int64 [, dn_boxes, dn_logits, dn_pos_idx]"""
    c = CASES[tag]
    seed = c['seed'] if seed is None else seed
    base = 'b' if tag in ('e', 'f', 'g') else tag          # e, f, g: case b's inputs
    r = np.random.RandomState(1000 * (ord(base) - ord('a')) + seed)
    l, b, nq, nc, g = c['layers'], len(c['groups']), c['nq'], c['nc'], sum(c['groups'])

    def boxes(*shape):
        return np.concatenate([r.uniform(0.1, 0.9, shape + (2,)), r.uniform(0.05, 0.4, shape + (2,))], -1)
    # fp32-representable values, so that the float64 truth and the fp32 runs start from the same numbers
    out = dict(boxes=boxes(l, b, nq), logits=r.normal(-2.0, 1.5, (l, b, nq, nc)), gt_boxes=boxes(g), gt_cls=r.randint(0, nc, (g,)).astype(np.int64))
    if 'dn' in c:
        ng, mx = c['dn']['groups'], max(c['groups'])
        ndn = mx * 2 * ng
        r2 = np.random.RandomState(7000 + seed)
        out['dn_boxes'] = np.concatenate([r2.uniform(0.1, 0.9, (c['dn']['layers'], b, ndn, 2)), r2.uniform(0.05, 0.4, (c['dn']['layers'], b, ndn, 2))], -1)
        out['dn_logits'] = r2.normal(-2.0, 1.5, (c['dn']['layers'], b, ndn, nc))
        out['dn_pos_idx'] = [np.concatenate([np.arange(n) + 2 * mx * i for i in range(ng)]).astype(np.int64) if n else np.zeros(0, np.int64) for n in c['groups']]
        out['dn_num_group'] = ng
        out['dn_num_split'] = [ndn, nq]
    for k in ('boxes', 'logits', 'gt_boxes', 'dn_boxes', 'dn_logits'):
        if k in out:
            out[k] = out[k].astype(np.float32).astype(np.float64)
    return out


def make_val_inputs(seed=None):
    """case (i): per image boxes (nq_i, 4) xywh normalised, scores (nq_i, nc) in (0, 1), labels (n_i, 5) = cls, xywh normalised.  Some predictions
    are the labels slightly moved, so that the matching has something to find."""
    v = VAL
    r = np.random.RandomState(9000 + (v['seed'] if seed is None else seed))
    out = []
    for si, (nq, nl) in enumerate(zip(v['nq'], v['labels'])):
        lab_box = np.concatenate([r.uniform(0.2, 0.8, (nl, 2)), r.uniform(0.1, 0.3, (nl, 2))], -1)
        lab_cls = r.randint(0, v['nc'], (nl,))
        boxes = np.concatenate([r.uniform(0.1, 0.9, (nq, 2)), r.uniform(0.05, 0.4, (nq, 2))], -1)
        scores = 1 / (1 + np.exp(-r.normal(-2.0, 1.5, (nq, v['nc']))))
        for j in range(nl):                                    # two predictions near every label, one with its class on top
            for k, (jit, top) in enumerate(((0.01, True), (0.04, False))):
                q = (2 * j + k) * 7 % nq
                boxes[q] = lab_box[j] + r.uniform(-jit, jit, 4)
                if top:
                    scores[q, lab_cls[j]] = 0.9 + 0.001 * j + 0.0005 * si      # distinct across the images too: get_stats sorts all rows together
        out.append(dict(boxes=boxes.astype(np.float32), scores=scores.astype(np.float32),
                        labels=np.concatenate([lab_cls[:, None].astype(np.float64), lab_box], 1).astype(np.float32)))
    return out


# ---------------------------------------------------------------------------------------------------------------- pieces
def _corners(b):
    x, y, w, h = b.unbind(-1)
    return x - w / 2, y - h / 2, x + w / 2, y + h / 2


def iou_xywh(b1, b2, giou=False, eps=1e-7):
    """bbox_iou(xywh=True[, GIoU=True]) of broadcastable (..., 4) boxes -> (...)"""
    ax1, ay1, ax2, ay2 = _corners(b1)
    bx1, by1, bx2, by2 = _corners(b2)
    inter = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(min=0) * (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(min=0)
    union = b1[..., 2] * b1[..., 3] + b2[..., 2] * b2[..., 3] - inter + eps
    iou = inter / union
    if not giou:
        return iou
    c_area = (torch.maximum(ax2, bx2) - torch.minimum(ax1, bx1)) * (torch.maximum(ay2, by2) - torch.minimum(ay1, by1)) + eps
    return iou - (c_area - union) / c_area


def cost_matrix(boxes, logits, gt_boxes, gt_cls, gain=None, alpha=ALPHA, gamma=GAMMA):
    """boxes (..., nq, 4), logits (..., nq, nc), gt_boxes (G, 4), gt_cls (G,) -> C (..., nq, G) against EVERY ground truth of the batch"""
    gain = gain or COST_GAIN
    p = torch.sigmoid(logits)[..., gt_cls]
    neg = (1 - alpha) * p ** gamma * (-(1 - p + 1e-8).log())
    pos = alpha * (1 - p) ** gamma * (-(p + 1e-8).log())
    l1 = (boxes[..., :, None, :] - gt_boxes).abs().sum(-1)
    g = 1.0 - iou_xywh(boxes[..., :, None, :], gt_boxes, giou=True)
    return gain['cls'] * (pos - neg) + gain['bbox'] * l1 + gain['giou'] * g


def solve(cost):
    """scipy on a float64 (nq, ng) block -> (queries ascending, ground truths)"""
    from scipy.optimize import linear_sum_assignment
    i, j = linear_sum_assignment(np.asarray(cost, dtype=np.float64))
    return i.astype(np.int64), j.astype(np.int64)


def assign_from_cost(C, groups):
    """C (l, B, nq, G) -> assign (l, B, nq) int64 numpy: the global ground-truth index of each query or -1, each image on its own columns"""
    C = np.asarray(C.detach() if torch.is_tensor(C) else C, dtype=np.float64)
    l, b, nq, _ = C.shape
    out = np.full((l, b, nq), -1, np.int64)
    off = np.concatenate([[0], np.cumsum(groups)])
    for li in range(l):
        for bi in range(b):
            if groups[bi]:
                i, j = solve(C[li, bi][:, off[bi]:off[bi + 1]])
                out[li, bi, i] = j + off[bi]
    return out


def gap_of(cost):
    """second-best assignment cost minus the best of a float64 (nq, ng) block: every optimal pair forbidden in turn"""
    cost = np.asarray(cost, dtype=np.float64)
    i, j = solve(cost)
    best = cost[i, j].sum()
    second = np.inf
    for a, b in zip(i, j):
        c2 = cost.copy()
        c2[a, b] = 1e9
        i2, j2 = solve(c2)
        second = min(second, c2[i2, j2].sum())
    return second - best


def uni_assign(assign, kw):
    """the assignment the criterion uses: with use_uni_match every auxiliary layer takes that of auxiliary layer uni_match_ind"""
    if kw.get('use_uni_match') and assign.shape[0] > 1:
        assign = assign.copy()
        assign[:-1] = assign[kw.get('uni_match_ind', 0)]
    return assign


def losses(boxes, logits, gt_boxes, gt_cls, assign, num_pairs, use_vfl=True, gain=None):
    """boxes (l, B, nq, 4), logits (l, B, nq, nc), assign (l, B, nq) long (-1 = unmatched) -> (out (l, 3) = class / bbox / giou, gt_score (l, B, nq));
    differentiable in boxes and logits (the target score is a constant)"""
    gain = gain or LOSS_GAIN
    nc = logits.shape[-1]
    m = assign >= 0
    if gt_boxes.shape[0] == 0:                       # nothing to index: one never-read row
        gt_boxes, gt_cls = torch.ones(1, 4, dtype=boxes.dtype), torch.zeros(1, dtype=torch.long)
    tgt = gt_boxes[assign.clamp(min=0)]
    score = torch.where(m, iou_xywh(boxes.detach(), tgt), torch.zeros_like(boxes[..., 0]))
    onehot = (torch.arange(nc)[None, None, None, :] == torch.where(m, gt_cls[assign.clamp(min=0)], torch.full_like(assign, nc))[..., None]).to(boxes.dtype)
    x = logits
    sp = torch.nn.functional.softplus(x)
    s = torch.sigmoid(x)
    if use_vfl and num_pairs > 0:
        t = score[..., None] * onehot
        el = (sp - x * t) * (0.75 * s ** 2 * (1 - onehot) + t)
    else:
        pt = onehot * s + (1 - onehot) * (1 - s)
        el = (sp - x * onehot) * (1 - pt) ** 1.5 * (onehot * 0.25 + (1 - onehot) * 0.75)
    l_cls = gain['cls'] * el.sum((1, 2, 3)) / max(num_pairs, 1)
    if num_pairs > 0:
        mf = m.to(boxes.dtype)
        l_box = gain['bbox'] * ((boxes - tgt).abs().sum(-1) * mf).sum((1, 2)) / num_pairs
        l_giou = gain['giou'] * ((1.0 - iou_xywh(boxes, tgt, giou=True)) * mf).sum((1, 2)) / num_pairs
    else:
        l_box = l_giou = torch.zeros_like(l_cls)
    return torch.stack([l_cls, l_box, l_giou], 1), score


NAMES = ('loss_class', 'loss_bbox', 'loss_giou')


def loss_dict(out, postfix=''):
    d = {f'{n}{postfix}': out[-1, i] for i, n in enumerate(NAMES)}
    d.update({f'{n}_aux{postfix}': out[:-1, i].sum() for i, n in enumerate(NAMES)})
    return d


def dn_assign(dn_pos_idx, num_group, groups, ndn):
    """(B, ndn) int64: the denoising assignment (every group repeats the image's ground truths in order), and its number of pairs"""
    a = np.full((len(groups), ndn), -1, np.int64)
    off = np.concatenate([[0], np.cumsum(groups)])
    for i, n in enumerate(groups):
        if n:
            a[i, dn_pos_idx[i]] = np.tile(np.arange(n) + off[i], num_group)
    return a, int(sum(groups)) * num_group


def criterion(tag, dtype, assign=None):
    """The whole criterion of a case in `dtype` on the CPU -> dict(cost, assign, losses (dict of floats), gt_score, d_boxes, d_logits [, dn ...]); `assign`
    (l, B, nq) replaces the solver (it is always solved on the float64 cost otherwise)."""
    c, inp = CASES[tag], make_inputs(tag)
    t = lambda k: torch.from_numpy(inp[k]).to(dtype)
    boxes, logits, gt_boxes = t('boxes').requires_grad_(), t('logits').requires_grad_(), t('gt_boxes')
    gt_cls = torch.from_numpy(inp['gt_cls'])
    groups, g = c['groups'], sum(c['groups'])
    cost = cost_matrix(boxes.detach(), logits.detach(), gt_boxes, gt_cls)
    if assign is None:
        assign = assign_from_cost(cost_matrix(t('boxes').double(), t('logits').double(), gt_boxes.double(), gt_cls), groups)
    used = uni_assign(np.asarray(assign), c['kw'])
    out, score = losses(boxes, logits, gt_boxes, gt_cls, torch.from_numpy(used), g, use_vfl=c['kw'].get('use_vfl', True))
    d = loss_dict(out)
    res = dict(cost=cost, assign=np.asarray(assign), used=used, gt_score=score.detach())
    total = out.sum()
    if 'dn' in c:
        db, dl = t('dn_boxes').requires_grad_(), t('dn_logits').requires_grad_()
        a, npairs = dn_assign(inp['dn_pos_idx'], inp['dn_num_group'], groups, db.shape[2])
        a = np.broadcast_to(a, (db.shape[0],) + a.shape).copy()
        dout, _ = losses(db, dl, gt_boxes, gt_cls, torch.from_numpy(a), npairs, use_vfl=c['kw'].get('use_vfl', True))
        d.update(loss_dict(dout, '_dn'))
        total = total + dout.sum()
        res['dn_assign'] = a
    else:
        d.update({f'{k}_dn': torch.zeros((), dtype=dtype) for k in list(d)})
    total.backward()
    res.update(losses={k: float(v.detach()) for k, v in d.items()}, d_boxes=boxes.grad if boxes.grad is not None else torch.zeros_like(boxes.detach()), d_logits=logits.grad)
    if 'dn' in c:
        res.update(dn_d_boxes=db.grad, dn_d_logits=dl.grad)
    return res


def val_rows(boxes, scores):
    """boxes (nq, 4) xywh, scores (nq, nc) -> rows (nq, 6) = xyxy, conf, cls: descending confidence, equal confidences by ascending query index"""
    b = boxes
    xyxy = torch.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2], -1)
    sc, cl = scores.max(-1)
    order = torch.from_numpy(np.argsort(-sc.numpy(), kind='stable'))
    return torch.cat([xyxy, sc[:, None], cl[:, None].to(xyxy.dtype)], -1)[order]


def checksum(a):
    return float(np.asarray(a, dtype=np.float64).sum())


def load_fixtures(golden_dir):
    """every array of tests/golden/rtdetr_loss_NN.npz in one dict"""
    out = {}
    for p in sorted(glob.glob(os.path.join(golden_dir, 'rtdetr_loss_[0-9][0-9].npz'))):
        with np.load(p, allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    return out
