"""TEST INFRASTRUCTURE for tests/test_nms_kernels.py: input generators, the NMS key maker and a host model of nms_kernel's segment plan.

`nms_plan` RESTATES DEVICE-SIDE CONTROL FLOW of mgdt_yolo_amd/csrc/nms.hip (nms_kernel): which candidates form a segment, how the segment edge is
found (score histogram or radix rank select), how many keys it holds, which sort runs on them and whether the scan is still going when the segment
starts.  It computes nothing the kernel's result depends on; it exists so that every GPU case can state the route it is there for and a host test
can hold it to that statement (a retune of the kernel's constants or of its planner then fails the census instead of silently moving the cases
onto other routes).  The numbers it needs from the kernel (NMS_THREADS, NMS_LDS_KEYS, NMS_BINS, KPT) are repeated here and compared with the
source text by test_plan_constants_match_the_kernel.
"""
import os
import re

import numpy as np
import torch

from oracle import nms as ON

F32 = np.float32
NMS_THREADS, NMS_LDS_KEYS, NMS_BINS, KPT = 1024, 16384, 2048, 8
FIRST_SEG = 1024                 # `unsigned done = 0, seg = 1024`; seg *= 4 after every segment
NMS_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mgdt_yolo_amd', 'csrc', 'nms.hip')


def kernel_constants():
    """NMS_THREADS, NMS_LDS_KEYS, NMS_BINS and KPT as nms.hip spells them."""
    src = open(NMS_HIP).read()
    out = {}
    for name in ('NMS_THREADS', 'NMS_LDS_KEYS', 'NMS_BINS'):
        m = re.findall(r'^#define\s+%s\s+(\d+)\s*$' % name, src, re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    m = re.findall(r'constexpr\s+int\s+KPT\s*=\s*(\d+)\s*;', src)
    assert len(m) == 1, m
    out['KPT'] = int(m[0])
    return out


def lds_bytes(max_det):
    """Dynamic LDS of one nms_kernel workgroup (nms_run): sort keys | kept float4 + area (padded to 8 bytes) | kept keys."""
    return NMS_LDS_KEYS * 8 + (5 * max_det + (max_det & 1)) * 4 + max_det * 8


LDS_LIMIT = 150 * 1024


def score_bits(score):
    return np.ascontiguousarray(score, F32).view(np.uint32).astype(np.uint64)


def make_key_np(score, cand):
    return ((np.uint64(0xFFFFFFFF) - score_bits(score)) << np.uint64(32)) | np.asarray(cand).astype(np.uint64)


def make_key(score, cand):
    """The kernel's 64-bit sort key as an int64 tensor: ((0xFFFFFFFF - bits(score)) << 32) | cand with cand = anchor * nc + cls; ascending key
    order is descending score, then ascending candidate id."""
    return torch.from_numpy(make_key_np(np.asarray(score, F32), cand).view(np.int64).copy())


def best_keys(pred, nc):
    """[B][A] keys of every anchor's best class (first maximal index), unfiltered: what the Detect tail kernel leaves next to y."""
    p = np.asarray(pred, F32)
    sc = p[:, 4:4 + nc]
    cls = sc.argmax(1)                                             # (B, A), first maximum
    best = np.take_along_axis(sc, cls[:, None], 1)[:, 0]
    cand = np.arange(p.shape[2], dtype=np.int64)[None] * nc + cls
    return make_key(best, cand)


def nms_plan(pred_img, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300, nc=None, max_nms=30000,
             max_wh=7680):
    """Host model of nms_kernel's control flow for ONE image (4+nc[+nm], A) - a restatement of device code, see the module docstring.

    Returns dict(ncand, K, total, cached, kept, segments) with segments = [(selector 'hist' | 'rank', keys, np2, sort 'shuffle' | 'lds' | 'global',
    kept at the segment's start)].  `kept at start` = oracle keepers among the first `done` sorted candidates, capped at max_det; the kernel stops
    in front of a segment once it has reached max_det."""
    p = np.asarray(pred_img, F32)
    nc = nc or p.shape[0] - 4
    A = p.shape[1]
    ml = bool(multi_label and nc > 1)
    b, conf, cls, anc = ON.nms_candidates(p, conf_thres, ml, classes, nc)
    ncand = len(conf)
    K = min(ncand, max_nms)
    total = A * nc if ml else A
    key = make_key_np(conf, anc * nc + cls)
    order = np.argsort(key, kind='stable')
    assert len(np.unique(key)) == ncand
    # oracle keepers along the sorted list
    bs = b[order][:K]
    off = cls[order][:K].astype(F32) * F32(0 if agnostic else max_wh)
    keep = ON.greedy_nms((bs + off[:, None]).astype(F32), iou_thres)
    kept_upto = np.zeros(K + 1, np.int64)
    np.add.at(kept_upto, keep + 1, 1)
    kept_upto = np.minimum(np.cumsum(kept_upto), max_det)
    # suffix histogram: shist[b] = candidates in bins >= b
    bins = np.minimum(NMS_BINS - 1, (conf * F32(NMS_BINS)).astype(np.int64))
    shist = np.zeros(NMS_BINS + 1, np.int64)
    shist[:NMS_BINS] = np.cumsum(np.bincount(bins, minlength=NMS_BINS)[::-1])[::-1]
    segs = []
    done, seg, use_hist, bin_hi = 0, FIRST_SEG, True, NMS_BINS
    while done < K:
        nkept = int(kept_upto[done])
        if nkept >= max_det:
            break
        tail = K - done <= seg + seg // 2
        by_hist, R = False, 0
        if use_hist:
            base, cap = shist[bin_hi], (seg + seg // 2 if tail else seg)
            T = bin_hi
            for bb in range(bin_hi):                               # exactly one b (shist is monotone)
                if shist[bb] - base <= cap and (bb == 0 or shist[bb - 1] - base > cap):
                    T = bb
            c = shist[T] - base
            if c >= 1 and done + c <= K:
                by_hist, R, bin_hi = True, done + int(c), T
        if not by_hist:
            use_hist = False
            R = K if tail else done + seg
        cnt = R - done
        np2 = 1
        while np2 < cnt:
            np2 <<= 1
        sort = 'shuffle' if np2 <= NMS_THREADS else ('lds' if np2 <= NMS_LDS_KEYS else 'global')
        segs.append(('hist' if by_hist else 'rank', cnt, np2, sort, nkept))
        done, seg = R, seg * 4
    return dict(ncand=ncand, K=K, total=total, cached=total <= KPT * NMS_THREADS, kept=int(kept_upto[min(done, K)]), segments=segs)


def distinct_scores(rng, n, lo, hi):
    """n different fp32 scores spread evenly over (lo, hi), shuffled."""
    s = (lo + (hi - lo) * (rng.permutation(n) + 0.5) / n).astype(F32)
    assert len(np.unique(s)) == n
    return s


def clusters(seed, A, nc, grid, pitch, size, jitter, scores, cls=None):
    """One image (4+nc, A): box centres on a grid x grid lattice of spacing `pitch` (a random cell per anchor), width and height size +- jitter, and one
    non-zero class score per anchor.  With pitch=100, size=40, jitter=1.5 the boxes of a cell suppress each other at iou_thres=0.5 (IoU >=
    (38.5 / 41.5)^2 = 0.86) and boxes of different cells never touch: about grid^2 x nc boxes are kept however many candidates the scan walks through.

    scores: a float (every anchor the same score), (lo, hi) -> distinct scores in that interval, an (A,) array, or an (nc, A) array that fills every
    class row (multi-label inputs; `cls` is then unused).  cls: None -> a random class per anchor, or an (A,) array."""
    r = np.random.default_rng(seed)
    y = np.zeros((4 + nc, A), F32)
    cell = r.integers(0, grid * grid, A)
    y[0] = (cell % grid) * pitch + pitch / 2
    y[1] = (cell // grid) * pitch + pitch / 2
    y[2] = size + r.uniform(-jitter, jitter, A)
    y[3] = size + r.uniform(-jitter, jitter, A)
    if isinstance(scores, tuple):
        scores = distinct_scores(r, A, *scores)
    elif np.isscalar(scores):
        scores = np.full(A, scores, F32)
    scores = np.asarray(scores, F32)
    if scores.ndim == 2:
        assert scores.shape == (nc, A)
        y[4:] = scores
        return y
    c = r.integers(0, nc, A) if cls is None else np.asarray(cls)
    y[4 + c, np.arange(A)] = scores
    return y


def chain(length, start, step=10.0, box=40.0, y0=2000.0):
    """xywh of `length` box x box squares on a line, `step` apart: IoU with the neighbour 0.6, with the next-but-one 1/3 (step 10, box 40)."""
    xy = np.zeros((4, length), F32)
    xy[0] = start + step * np.arange(length)
    xy[1] = y0
    xy[2] = box
    xy[3] = box
    return xy


# ------------------------------------------------------------------------------------------------ validator matching inputs
def _rows(*rows):
    return np.asarray(rows, F32).reshape(-1, len(rows[0])) if rows else None


def val_random(seed, nd, nl, ncls=5, wrong_cls=0.15):
    """Labels on a lattice (some of them overlapping pairs), detections = jittered copies of random labels (so one label is chosen by many detections,
    from every round of 256), a share of them with another class.  Continuous jitter: exact IoU ties do not occur (test_val_match_inputs_have_no_tie
    checks)."""
    r = np.random.default_rng(seed)
    lab = np.zeros((nl, 5), F32)
    for i in range(nl):
        cx, cy = 60.0 * (i % 8) + 40, 60.0 * (i // 8) + 40
        if i % 3 == 2:                                             # overlaps its predecessor: a detection between them sees two labels
            cx, cy = lab[i - 1, 1] + lab[i - 1, 3], lab[i - 1, 2] + lab[i - 1, 4]
            cx, cy = cx / 2 + 9, cy / 2 + 4
        w, h = r.uniform(24, 44, 2)
        lab[i] = [r.integers(0, ncls) if i % 3 != 2 else lab[i - 1, 0], cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]
    det = np.zeros((nd, 6), F32)
    src = r.integers(0, nl, nd)
    j = r.normal(0, 1, (nd, 4)) * r.choice([0.5, 2.0, 5.0], (nd, 1))
    det[:, :4] = lab[src, 1:] + j
    det[:, 4] = np.sort(r.uniform(0.05, 1, nd))[::-1]
    det[:, 5] = np.where(r.random(nd) < wrong_cls, (lab[src, 0] + 1) % ncls, lab[src, 0])
    return det, lab


def val_crafted():
    """Hand-made images, each (name, det (nd, 6), lab (nl, 5)).  Boxes are xyxy; labels are [cls, x1, y1, x2, y2]."""
    def pad(det, n, cls=9.0):                                      # filler detections far from every label, of a class of their own
        out = np.zeros((n, 6), F32)
        out[:, 0] = 5000 + 50 * np.arange(n); out[:, 1] = 5000; out[:, 2] = out[:, 0] + 30; out[:, 3] = 5030; out[:, 4] = 0.5; out[:, 5] = cls
        for i, row in det.items():
            out[i] = row
        return out
    cases = []
    # a label whose only matching detection has index >= 256 (second round), another one matched in the third round only
    lab = _rows([1, 10, 10, 50, 50], [2, 100, 10, 140, 50], [4, 300, 300, 340, 340])
    cases.append(('late_only', pad({300: [11, 10, 51, 50, .9, 1], 599: [100, 12, 140, 52, .8, 2]}, 600), lab))
    # one label chosen by detections of two (three) different rounds: the lowest index wins although the later ones overlap better
    lab = _rows([1, 10, 10, 50, 50], [3, 200, 200, 260, 260])
    cases.append(('cross_round', pad({10: [14, 14, 54, 54, .9, 1], 400: [10, 10, 50, 50, .8, 1], 580: [11, 10, 51, 50, .7, 1],
                                      255: [205, 205, 265, 265, .6, 3], 256: [200, 200, 260, 260, .5, 3]}, 600), lab))
    # IoU exactly on a level in fp32 (small integers: inter 1 / union 2 = 0.5, inter 3 / union 4 = 0.75; union + 1e-7 rounds back to the union),
    # next to pairs one ulp-ish below (a slightly larger box)
    lab = _rows([0, 0, 0, 1, 1], [0, 10, 0, 13, 1], [0, 20, 0, 21, 1], [0, 30, 0, 33, 1])
    cases.append(('iou_on_level', pad({0: [0, 0, 2, 1, .9, 0], 1: [10, 0, 14, 1, .8, 0], 2: [20, 0, 22.000002, 1, .7, 0], 3: [30, 0, 34.000004, 1, .6, 0]}, 8), lab))
    # labels of a class that no detection has, and detections of a class that no label has
    d, l = val_random(7, 40, 6, ncls=3)
    l[:, 0] += 10
    cases.append(('class_never_seen', d, l))
    return cases


def val_has_tie(det, lab, iouv):
    """True if some detection sees two same-class labels with IoU >= the lowest level and EQUAL IoU (the reference's unstable sort decides those)."""
    from oracle import val as OV
    if len(det) == 0 or len(lab) == 0:
        return False
    d, l = torch.from_numpy(np.asarray(det, F32)), torch.from_numpy(np.asarray(lab, F32))
    iou = OV.box_iou(l[:, 1:], d[:, :4]).numpy()
    ok = (l[:, 0:1] == d[:, 5]).numpy() & (iou >= float(min(iouv)))
    for k in range(iou.shape[1]):
        v = iou[ok[:, k], k]
        if len(np.unique(v)) != len(v):
            return True
    return False
