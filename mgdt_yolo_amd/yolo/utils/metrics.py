"""Box, mask and keypoint overlap functions and the validator's AP reduction with the reference's names (reference: yolo/utils/metrics.py).

`box_iou`, `bbox_iou` (IoU / GIoU / DIoU / CIoU, forward values), `mask_iou` and `kpt_iou` run as HIP kernels (mgdt_box_iou / mgdt_bbox_iou /
mgdt_mask_iou_fwd / mgdt_kpt_iou_fwd).  `ap_per_class` keeps
the reference's signature and return tuple: the O(detections) part - per-class cumulative TP / FP, recall / precision curves, compute_ap's
envelope, 101-point interpolation and integration, the 1000-point P / R-vs-confidence curves - runs on the device in fp64 with numpy's own
arithmetic order (mgdt_ap_per_class: the AP matrix equals the reference's bit for bit); grouping the detections by (class, confidence) is a
device sort; the last few lines (F1 smoothing over 1000 points, arg-max, counts) are the reference's numpy expressions on a (nc, 1000) array."""
import numpy as np
import torch

from ... import _lib as L
from ... import ops as hip

OKS_SIGMA = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0     # the COCO keypoint constants (metrics.py:15)


def box_iou(box1, box2, eps=1e-7):
    """Pairwise IoU of (N, 4) and (M, 4) xyxy boxes -> (N, M) (metrics.py:52-72)."""
    hip._need_gpu(box1)
    b1, b2 = box1.float().contiguous(), box2.float().contiguous()
    out = torch.empty(b1.shape[0], b2.shape[0], dtype=torch.float32, device=b1.device)
    L.check(L.lib().mgdt_box_iou(hip.ptr(b1), b1.shape[0], hip.ptr(b2), b2.shape[0], float(eps), hip.ptr(out), hip.stream()), 'box_iou')
    return out


def bbox_iou(box1, box2, xywh=True, GIoU=False, DIoU=False, CIoU=False, eps=1e-7):
    """IoU / GIoU / DIoU / CIoU of box1 (1, 4) or (n, 4) against box2 (n, 4) -> (n, 1), forward values (metrics.py:75-128).
    (The training loss has its own fused CIoU forward + backward inside mgdt_detect_loss_fwd / _bwd.)"""
    hip._need_gpu(box1)
    b1, b2 = box1.float().contiguous().view(-1, 4), box2.float().contiguous().view(-1, 4)
    n = max(b1.shape[0], b2.shape[0])
    if b1.shape[0] not in (1, n) or b2.shape[0] not in (1, n):
        raise RuntimeError(f'bbox_iou: cannot broadcast {tuple(box1.shape)} with {tuple(box2.shape)}')
    mode = 3 if CIoU else 2 if DIoU else 1 if GIoU else 0
    out = torch.empty(n, 1, dtype=torch.float32, device=b1.device)
    L.check(L.lib().mgdt_bbox_iou(hip.ptr(b1), 4 if b1.shape[0] == n and n > 1 or b1.shape[0] == n == 1 else 0, hip.ptr(b2),
                                  4 if b2.shape[0] == n and n > 1 or b2.shape[0] == n == 1 else 0, n, int(bool(xywh)), mode, float(eps), hip.ptr(out),
                                  hip.stream()), 'bbox_iou')
    return out


def mask_iou(mask1, mask2, eps=1e-7):
    """IoU of 0 / 1 masks: mask1 (N, n) ground truth, mask2 (M, n) predictions, float32 or uint8 holding 0 / 1 ONLY
    (the reference accepts any float; other values are refused by a device-side assertion) -> (N, M) float32 (metrics.py:131-147), on the
    mask bytes with the int8 matrix cores (mgdt_mask_iou_fwd).  Intersections and areas are exact integers, so the result equals the reference's
    float32 matmul bit for bit for n <= 2^24.  More rows than the kernel's limits (256 / 1024) are processed in blocks."""
    hip._need_gpu(mask1)
    if mask1.dim() != 2 or mask2.dim() != 2 or mask1.shape[1] != mask2.shape[1]:
        raise RuntimeError(f'mask_iou: (N, n) and (M, n) masks expected, got {tuple(mask1.shape)} and {tuple(mask2.shape)}')
    def u8(m):
        if m.dtype != torch.uint8:
            if hasattr(torch, '_assert_async'):       # no host sync; the conversion below truncates, so anything but 0 / 1 would change the answer
                torch._assert_async(((m == 0) | (m == 1)).all(), 'mask_iou: masks must hold 0 / 1 only')
            m = m.to(torch.uint8)
        return m.contiguous()
    m1, m2 = u8(mask1), u8(mask2)
    N, M, n = m1.shape[0], m2.shape[0], m1.shape[1]
    out = torch.zeros(N, M, dtype=torch.float32, device=m1.device)
    if N == 0 or M == 0 or n == 0:
        return out
    cnt = lambda k: torch.full((1,), k, dtype=torch.int32, device=m1.device)
    zero = torch.zeros(1, dtype=torch.int32, device=m1.device)
    for i in range(0, N, hip.MASK_IOU_MAX_LAB):
        a = m1[i:i + hip.MASK_IOU_MAX_LAB]
        for j in range(0, M, hip.MASK_IOU_MAX_DET):
            b = m2[j:j + hip.MASK_IOU_MAX_DET]
            out[i:i + a.shape[0], j:j + b.shape[0]] = hip.mask_iou_batch(b.view(-1, 1, n), cnt(b.shape[0]), zero, b.shape[0], a.view(-1, 1, n),
                                                                         cnt(a.shape[0]), a.shape[0], index_map=False, lab_offsets=zero, eps=eps)[0]
    return out


def kpt_iou(kpt1, kpt2, area, sigma, eps=1e-7):
    """Object keypoint similarity: kpt1 (N, nkpt, 3) ground truth [x, y, visibility], kpt2 (M, nkpt, 2 | 3) predictions, area (N,) of the ground
    truth, sigma nkpt keypoint scales (list / numpy / tensor) -> (N, M) float32 (metrics.py:150-169), one mgdt_kpt_iou_fwd launch.  More rows than
    the kernel's limits (256 / 1024) are processed in blocks."""
    hip._need_gpu(kpt1)
    hip._need_gpu(kpt2)
    if kpt1.dim() != 3 or kpt2.dim() != 3 or kpt1.shape[2] != 3 or kpt2.shape[2] not in (2, 3) or kpt1.shape[1] != kpt2.shape[1]:
        raise RuntimeError(f'kpt_iou: (N, nkpt, 3) labels and (M, nkpt, 2 | 3) predictions expected, got {tuple(kpt1.shape)} and {tuple(kpt2.shape)}')
    dev = kpt1.device
    g, p = kpt1.float().contiguous(), kpt2.float().contiguous()
    a = (area if torch.is_tensor(area) else torch.as_tensor(np.asarray(area))).to(dev).float().contiguous().view(-1)
    sg = (sigma if torch.is_tensor(sigma) else torch.as_tensor(np.asarray(sigma, dtype=np.float32))).to(dev).float().contiguous().view(-1)
    N, M, nkpt = g.shape[0], p.shape[0], g.shape[1]
    if a.numel() != N or sg.numel() != nkpt:
        raise RuntimeError(f'kpt_iou: {a.numel()} areas for {N} labels, {sg.numel()} sigmas for {nkpt} keypoints')
    out = torch.zeros(N, M, dtype=torch.float32, device=dev)
    if N == 0 or M == 0 or nkpt == 0:
        return out
    cnt = lambda k: torch.full((1,), k, dtype=torch.int32, device=dev)
    for i in range(0, N, hip.KPT_IOU_MAX_LAB):
        gi, ai = g[i:i + hip.KPT_IOU_MAX_LAB], a[i:i + hip.KPT_IOU_MAX_LAB]
        for j in range(0, M, hip.KPT_IOU_MAX_DET):
            pj = p[j:j + hip.KPT_IOU_MAX_DET]
            out[i:i + gi.shape[0], j:j + pj.shape[0]] = hip.kpt_iou_batch(pj[None], cnt(pj.shape[0]), pj.shape[0], gi[None], ai[None], cnt(gi.shape[0]), sg,
                                                                        eps=eps)[0]
    return out


def smooth(y, f=0.05):
    """Box filter of fraction f (metrics.py:293-298)."""
    nf = round(len(y) * f * 2) // 2 + 1
    p = np.ones(nf // 2)
    yp = np.concatenate((p * y[0], y, p * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode='valid')


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, on_plot=None, save_dir=None, names=(), eps=1e-16, prefix='', device=None):
    """Average precision per class (metrics.py:410-497): same arguments (numpy arrays or tensors) and the same 7-tuple
    (tp, fp, p, r, f1, ap, unique_classes).  Plotting is host tooling outside the path (plot must be False)."""
    if plot:
        raise RuntimeError('ap_per_class: plotting is host-side tooling outside the detection path')
    dev = torch.device(device or (tp.device if torch.is_tensor(tp) and tp.is_cuda else 'cuda:0'))
    t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev).to(dt)
    tp_d, conf_d, pcls_d = t(tp, torch.uint8), t(conf, torch.float32), t(pred_cls, torch.float32)
    tcls = np.asarray(target_cls.detach().cpu() if torch.is_tensor(target_cls) else target_cls)
    unique_classes, nt = np.unique(tcls, return_counts=True)                       # metrics.py:445
    nc, T = unique_classes.shape[0], tp_d.shape[1]
    n = tp_d.shape[0]
    # group by class (ascending) and, inside a class, by descending confidence: two stable device sorts (np.argsort(-conf) in the reference;
    # equal confidences keep their input order here)
    o1 = torch.sort(conf_d, descending=True, stable=True).indices
    o2 = torch.sort(pcls_d[o1], stable=True).indices
    order = o1[o2]
    tp_s, conf_s, cls_s = tp_d[order].contiguous(), conf_d[order].contiguous(), pcls_d[order]
    uc = torch.from_numpy(unique_classes.astype(np.float32)).to(dev)
    # detections of label class c occupy [lo_c, hi_c) of the sorted arrays; classes without labels are skipped like the reference's loop
    lo, hi = torch.searchsorted(cls_s, uc, right=False), torch.searchsorted(cls_s, uc, right=True)
    counts = hi - lo
    segs = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)
    idx = (torch.cat([torch.arange(int(a), int(b), device=dev) for a, b in zip(lo.tolist(), hi.tolist())])
           if nc and n else torch.zeros(0, dtype=torch.long, device=dev))
    tp_c, conf_c = tp_s[idx].contiguous(), conf_s[idx].contiguous()
    nd = int(tp_c.shape[0])
    x101 = torch.from_numpy(np.linspace(0, 1, 101)).to(dev)
    px_np = np.linspace(0, 1, 1000)
    px = torch.from_numpy(px_np).to(dev)
    ap = torch.zeros(nc, T, dtype=torch.float64, device=dev)
    p = torch.zeros(nc, 1000, dtype=torch.float64, device=dev)
    r = torch.zeros(nc, 1000, dtype=torch.float64, device=dev)
    if nc and nd:
        ws = torch.empty(L.lib().mgdt_ap_workspace_bytes(nd, nc), dtype=torch.uint8, device=dev)
        nlab = torch.from_numpy(nt.astype(np.int32)).to(dev)
        L.check(L.lib().mgdt_ap_per_class(hip.ptr(tp_c), hip.ptr(conf_c), hip.ptr(segs), hip.ptr(nlab), nd, nc, T, hip.ptr(x101), hip.ptr(px), float(eps),
                                          hip.ptr(ws), hip.ptr(ap), hip.ptr(p), hip.ptr(r), hip.stream()), 'ap_per_class')
    ap, p, r = ap.cpu().numpy(), p.cpu().numpy(), r.cpu().numpy()
    # the tail of the reference function, verbatim numpy on (nc, 1000) arrays (metrics.py:476-497)
    f1 = 2 * p * r / (p + r + eps)
    i = smooth(f1.mean(0), 0.1).argmax() if nc else 0
    p, r, f1 = p[:, i], r[:, i], f1[:, i]
    tp_out = (r * nt).round()
    fp_out = (tp_out / (p + eps) - tp_out).round()
    return tp_out, fp_out, p, r, f1, ap, unique_classes.astype(int)


class ClassifyMetrics:
    """Top-1 / top-5 accuracy of the classification task (reference metrics.py:934-977).  `process(targets, pred)`: lists of per-batch targets
    (n,) and predicted class indices (n, min(nc, 5)), best first - the rows mgdt_cls_topk_fwd writes.  The comparison is a few integers per image
    and runs wherever the tensors live (host tensors after the validator's one read)."""

    def __init__(self):
        self.top1 = 0
        self.top5 = 0
        self.speed = {'preprocess': 0.0, 'inference': 0.0, 'loss': 0.0, 'postprocess': 0.0}

    def process(self, targets, pred):
        pred, targets = torch.cat(list(pred)), torch.cat(list(targets))
        correct = (targets.reshape(-1)[:, None] == pred).float()
        acc = torch.stack((correct[:, 0], correct.max(1).values), dim=1)          # (top1, top5) accuracy
        self.top1, self.top5 = acc.mean(0).tolist()

    @property
    def fitness(self):
        return self.top5

    @property
    def results_dict(self):
        return dict(zip(self.keys + ['fitness'], [self.top1, self.top5, self.fitness]))

    @property
    def keys(self):
        return ['metrics/accuracy_top1', 'metrics/accuracy_top5']


def _one_image(detections, labels, dev):
    """The per-image arguments of the reference in the batch layout of `ops.nms`: -> det (1, max(n, 1), 6), ndet, labels (1, max(m, 1), 5), nlab."""
    cnt = lambda k: torch.full((1,), k, dtype=torch.int32, device=dev)
    if labels.dim() == 1:                                   # the class vector of the `detections is None` call (val.py:88)
        labels = torch.cat((labels.float().view(-1, 1), torch.zeros(labels.shape[0], 4, device=dev)), 1)
    if labels.dim() != 2 or labels.shape[1] != 5:
        raise RuntimeError(f'process_batch: labels are (M, 5) [cls, x1, y1, x2, y2] or, without detections, (M,) classes, got {tuple(labels.shape)}')
    if detections is None:
        detections = torch.zeros(0, 6, device=dev)
    if detections.dim() != 2 or detections.shape[1] != 6:
        raise RuntimeError(f'process_batch: detections are (N, 6) [x1, y1, x2, y2, conf, cls], got {tuple(detections.shape)}')
    n, m = detections.shape[0], labels.shape[0]
    det = detections.float().contiguous() if n else torch.zeros(1, 6, device=dev)
    lab = labels.float().contiguous() if m else torch.zeros(1, 5, device=dev)
    return det[None], cnt(n), lab[None], cnt(m)


class ConfusionMatrix:
    """The detection confusion matrix (reference metrics.py:176-264) accumulated on the device by mgdt_val_confusion_fwd: int32 counts,
    row = predicted class, column = true class, index nc = background.  `process_batch(detections, labels)` has the reference's per-image
    signature; `process_batch_dev` takes a whole batch as `ops.nms` returns it.  Reading `matrix` is the only synchronisation."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45, task='detect'):
        if task != 'detect':
            raise RuntimeError(f"ConfusionMatrix: task='{task}': the classification counts are kept by ClassificationValidator (confusion_matrix); "
                               "this class is the detection matrix")
        self.task, self.nc, self.conf, self.iou_thres = task, int(nc), conf, iou_thres
        self._dev = None

    def _buffer(self, dev):
        if self._dev is None:
            self._dev = torch.zeros(self.nc + 1, self.nc + 1, dtype=torch.int32, device=dev)
        return self._dev

    def process_batch_dev(self, det, ndet, labels, nlab):
        """det (B, max_det, 6) + ndet (B,) int32, labels (B, max_lab, 5) + nlab (B,) int32, one pixel frame per image: one launch, no sync."""
        hip._need_gpu(det)
        hip.val_confusion(det, ndet, labels, nlab, self.nc, matrix=self._buffer(det.device), cm_conf=self.conf, cm_iou=self.iou_thres)

    def process_batch(self, detections, labels):
        """detections (N, 6) [x1, y1, x2, y2, conf, cls] or None, labels (M, 5) [cls, x1, y1, x2, y2] (with detections=None also (M,) classes)."""
        hip._need_gpu(labels)
        if detections is not None:
            hip._need_gpu(detections)
        self.process_batch_dev(*_one_image(detections, labels, labels.device))

    @property
    def matrix(self):
        if self._dev is None:
            return np.zeros((self.nc + 1, self.nc + 1))
        return self._dev.cpu().numpy().astype(np.float64)

    def tp_fp(self):
        """True and false positives per class, background dropped (metrics.py:259-264)."""
        m = self.matrix
        tp = m.diagonal()
        fp = m.sum(1) - tp
        return tp[:-1], fp[:-1]

    def plot(self, *args, **kwargs):
        raise RuntimeError('ConfusionMatrix: plotting and printing the matrix are host-side tooling outside the validation path (read `matrix`)')

    print = plot


class CountMetrics:
    """Counting metrics of a detection model (reference nn/cal_counting_metrics.py and nn/cal_model_count_error.py, for nc classes): per class TP /
    FP / FN at IoU `iou`, true and predicted counts per image, MAE, RMSE and R^2, from int64 sums accumulated on the device by
    mgdt_val_confusion_fwd.  Reading `slots` / `results_dict` is the only synchronisation."""

    def __init__(self, nc, conf=0.25, iou=0.5, trunc_labels=True):
        self.nc, self.conf, self.iou, self.trunc_labels = int(nc), conf, iou, bool(trunc_labels)
        self._dev = None

    def _buffer(self, dev):
        if self._dev is None:
            self._dev = torch.zeros(self.nc, hip.COUNT_SLOTS, dtype=torch.int64, device=dev)
        return self._dev

    def process_batch_dev(self, det, ndet, labels, nlab):
        hip._need_gpu(det)
        hip.val_confusion(det, ndet, labels, nlab, self.nc, counts=self._buffer(det.device), cnt_conf=self.conf, cnt_iou=self.iou, trunc_labels=self.trunc_labels)

    def process_batch(self, detections, labels):
        """One image, the arguments of ConfusionMatrix.process_batch (an image without detections or without labels still counts as an image)."""
        hip._need_gpu(labels)
        if detections is not None:
            hip._need_gpu(detections)
        self.process_batch_dev(*_one_image(detections, labels, labels.device))

    @property
    def slots(self):
        """(nc, COUNT_SLOTS) int64: images, sum t, sum p, sum t^2, sum t*p, sum (t-p)^2, sum |t-p|, TP, FP, FN."""
        if self._dev is None:
            return np.zeros((self.nc, hip.COUNT_SLOTS), np.int64)
        return self._dev.cpu().numpy()

    @staticmethod
    def from_slots(slots):
        """Integer slots -> dict of (nc,) arrays, float64.  R^2 is sklearn.metrics.r2_score behind the script's guard: 0 with fewer than two
        images; with SS_tot = 0, 1 where SS_res = 0 and 0 elsewhere.  n * SS_tot = n * sum t^2 - (sum t)^2 is formed in integers."""
        s = np.asarray(slots, dtype=np.int64)
        n, st, stt, d2 = s[:, 0], s[:, 1], s[:, 3], s[:, 5]
        nf = np.maximum(n, 1).astype(np.float64)
        n_ss_tot = n * stt - st * st
        with np.errstate(divide='ignore', invalid='ignore'):
            r2 = 1.0 - (d2.astype(np.float64) * nf) / n_ss_tot.astype(np.float64)
        r2 = np.where(n_ss_tot == 0, np.where(d2 == 0, 1.0, 0.0), r2)
        r2 = np.where(n < 2, 0.0, r2)
        return dict(tp=s[:, 7].astype(np.float64), fp=s[:, 8].astype(np.float64), fn=s[:, 9].astype(np.float64), gt=st.astype(np.float64),
                    pred=s[:, 2].astype(np.float64), mae=np.where(n > 0, s[:, 6] / nf, 0.0), rmse=np.where(n > 0, np.sqrt(d2 / nf), 0.0), r2=r2)

    @property
    def keys(self):
        return [f'metrics/count_{k}({c})' for c in range(self.nc) for k in ('tp', 'fp', 'fn', 'gt', 'pred', 'mae', 'rmse', 'r2')]

    @property
    def results_dict(self):
        """Flat: 'metrics/count_<tp|fp|fn|gt|pred|mae|rmse|r2>(<class>)' -> float."""
        r = self.from_slots(self.slots)
        return {f'metrics/count_{k}({c})': float(r[k][c]) for c in range(self.nc) for k in ('tp', 'fp', 'fn', 'gt', 'pred', 'mae', 'rmse', 'r2')}
