"""Validator-side hot step (reference: yolo/v8/detect/val.py): matching predictions to labels on the device.

Only the per-batch compute of the reference's DetectionValidator is mirrored here - `_process_batch` (val.py:152-175) with the same
signature and return, plus a batched form that consumes the NMS kernel's output directly.  Dataset handling, plotting, JSON export and the
final `ap_per_class` reduction (numpy, once per validation run) are host glue outside the hot path.

The class is also the batch core of the segmentation and pose validators: the padded detection rows, the label census, the native-space boxes,
the per-image stats rows and the summary dict exist here once; a task adds its own similarity (mask IoU, OKS) and its second match.
"""
from types import SimpleNamespace

import numpy as np
import torch

from .... import ops as hip
from ...utils import ops
from ...utils.metrics import ConfusionMatrix, CountMetrics, _one_image, ap_per_class

__all__ = ('DetectionValidator',)

_KEYS = ('metrics/precision', 'metrics/recall', 'metrics/mAP50', 'metrics/mAP50-95')


class DetectionValidator:
    _REFUSAL = None                          # None: `args` is not looked at; a task's validator sets the tail of its refusal text ('' for none)
    _STATS = (('(B)', 0, 'ap'),)             # (key suffix, column of a stats row, attribute that keeps the AP matrix)

    def __init__(self, device='cuda:0', args=None):
        self.device = torch.device(device)
        self.iouv = torch.linspace(0.5, 0.95, 10, device=self.device)     # val.py:60: IoU vector for mAP@0.5:0.95
        self.niou = self.iouv.numel()
        self.confusion_matrix = self.count_metrics = None      # init_metrics(confusion=True, counting=True)
        self._nms = None                                       # (per, rows, counts_dev, counts) of a task's `postprocess`
        for k in ('plots', 'save_json', 'single_cls', 'save_hybrid'):
            if self._REFUSAL is not None and (args or {}).get(k):
                raise RuntimeError(f'{type(self).__name__}: {k}=True is host-side tooling (plots, confusion matrix, COCO JSON / pycocotools, class merging) '
                                   f'outside the validation path{self._REFUSAL}')

    def _process_batch(self, detections, labels):
        """detections (N, 6) [x1, y1, x2, y2, conf, cls], labels (M, 5) [cls, x1, y1, x2, y2] -> correct (N, 10) bool on detections.device."""
        n, m = detections.shape[0], labels.shape[0]
        if n == 0 or m == 0:
            return torch.zeros(n, self.niou, dtype=torch.bool, device=detections.device)
        return hip.val_match(*_one_image(detections, labels, detections.device), self.iouv.to(detections.device))[0]

    # ---- the per-batch metric update and the final reduction (val.py:73-117, :123-131; metrics.py:410-497) -------------------------------
    def init_metrics(self, nc=80, conf=0.001, iou=0.7, max_det=300, confusion=False, counting=False):
        """confusion / counting (both off by default): also accumulate the reference's ConfusionMatrix (val.py:54, fed as val.py:88 and :109 do) /
        the counting metrics of nn/cal_counting_metrics.py on the device; `get_stats` then adds `confusion_matrix` and the `metrics/count_*` keys."""
        self.nc, self.conf, self.iou, self.max_det = nc, conf, iou, max_det     # validator.py:85-86 / default.yaml
        self.seen, self.stats = 0, []
        self.confusion_matrix = ConfusionMatrix(nc=nc) if confusion else None
        self.count_metrics = CountMetrics(nc=nc) if counting else None

    def preprocess(self, batch):
        """Tensors of the dataloader dict go to the device.  The host copy of batch_idx is kept so that the label counts cost no device read."""
        batch = dict(batch)
        batch['batch_idx_host'] = batch['batch_idx'].detach().cpu()
        for k in ('img', 'cls', 'bboxes', 'batch_idx'):
            batch[k] = batch[k].to(self.device, non_blocking=True)
        return batch

    def postprocess(self, preds):
        """val.py:63-71: NMS with the validator's settings (multi_label)."""
        return ops.non_max_suppression(preds, self.conf, self.iou, multi_label=True, max_det=self.max_det)

    # ---- the batch core -------------------------------------------------------------------------------------------------------------------
    def _padded_rows(self, per, width):
        """per: list of (n_i, width) rows -> (rows (B, max_det, width) zero-padded, counts_dev (B,) int32, counts list): the batch form `postprocess`
        kept when `per` is its list, else a padded copy (the sizes are known: no device read)."""
        if self._nms is not None and self._nms[0] is per:
            return self._nms[1:]
        counts = [int(p.shape[0]) for p in per]
        rows = torch.zeros(len(per), max(max(counts), 1), width, dtype=torch.float32, device=self.device)
        for i, p in enumerate(per):
            rows[i, :counts[i]] = p
        return rows, torch.tensor(counts, dtype=torch.int32).to(self.device), counts

    def _label_census(self, batch, b):
        """The labels of a batch of b images, grouped by image in their given order: nl (labels per image) and off (their exclusive offsets) as host
        lists from the host copy of batch_idx, bidx (n,) long, cls (n, 1), bbox (n, 4) on the device, and `order`: the stable re-sort that was applied
        (the caller applies it to its own per-label tensor), None when the labels came grouped."""
        dev = self.device
        bidx_host = batch.get('batch_idx_host')
        if bidx_host is None:
            bidx_host = batch['batch_idx'].detach().cpu()
        bidx_host = bidx_host.long().view(-1)
        nl = torch.bincount(bidx_host, minlength=b)[:b].tolist()
        bidx = batch['batch_idx'].to(dev).long().view(-1)
        cls = batch['cls'].to(dev).float().view(-1, 1)
        bbox = batch['bboxes'].to(dev).float().view(-1, 4)
        order = None
        if bidx_host.numel() > 1 and not bool((bidx_host[1:] >= bidx_host[:-1]).all()):
            order = torch.sort(bidx_host, stable=True).indices.to(dev)
            bidx, cls, bbox = bidx[order], cls[order], bbox[order]
        off = [sum(nl[:i]) for i in range(b)]
        return SimpleNamespace(nl=nl, off=off, bidx=bidx, cls=cls, bbox=bbox, order=order)

    def _native_space(self, batch, rows, counts, lab):
        """Boxes of predictions and labels in each image's native space (`scale_boxes`, one launch per image and side) -> predn (B, max_det, 6).  Added
        to `lab`: native (n, 5) [cls, x1, y1, x2, y2] and, when there is anything to match, the same rows as labels (B, max_lab, 5) zero-padded, nlab
        and lab_off (B,) int32 and the scatter index (bidx, pos) of label rows into (B, max_lab, ...); else labels = None."""
        dev = self.device
        in_shape = tuple(batch['img'].shape[2:])
        height, width = in_shape
        predn = rows[:, :, :6].clone()
        max_lab = max(lab.nl) if lab.nl else 0
        if max_lab:
            tbox = ops.xywh2xyxy(lab.bbox.contiguous()) * torch.tensor((width, height, width, height), dtype=torch.float32, device=dev)
        for si, (npr, nl, off) in enumerate(zip(counts, lab.nl, lab.off)):
            shape, rp = batch['ori_shape'][si], batch['ratio_pad'][si]
            if npr:
                ops.scale_boxes(in_shape, predn[si, :npr], shape, ratio_pad=rp)                       # native-space pred
            if nl:
                ops.scale_boxes(in_shape, tbox[off:off + nl], shape, ratio_pad=rp)                    # native-space labels
        lab.native = torch.cat((lab.cls, tbox), 1) if max_lab else torch.zeros(0, 5, device=dev)
        lab.labels = None
        if max_lab and max(counts):
            lab.nlab = torch.tensor(lab.nl, dtype=torch.int32).to(dev)
            lab.lab_off = torch.tensor(lab.off, dtype=torch.int32).to(dev)
            lab.pos = torch.arange(lab.bidx.numel(), device=dev) - lab.lab_off.long()[lab.bidx]
            lab.labels = torch.zeros(len(counts), max_lab, 5, dtype=torch.float32, device=dev)
            lab.labels[lab.bidx, lab.pos] = lab.native
        return predn

    def _append_stats(self, rows, counts, lab, *correct):
        """One stats row per image: (correct_* ..., conf, pcls, tcls).  correct: (B, max_det, 10) bool each, or None each when nothing was matched.
        An image without detections adds a row only if it has labels."""
        dev = self.device
        for si, (npr, nl, off) in enumerate(zip(counts, lab.nl, lab.off)):
            tcls = lab.cls[off:off + nl, 0]
            self.seen += 1
            if npr == 0:
                if nl:
                    empty = torch.zeros(0, self.niou, dtype=torch.bool, device=dev)
                    self.stats.append((*(empty,) * len(correct), *torch.zeros((2, 0), device=dev), tcls))
                continue
            if correct[0] is None:
                c = (torch.zeros(npr, self.niou, dtype=torch.bool, device=dev),) * len(correct)
            else:
                c = tuple(x[si, :npr] for x in correct)
            self.stats.append((*c, rows[si, :npr, 4], rows[si, :npr, 5], tcls))

    def _update_extras(self, predn, labelsn):
        """One image in native space: predn (n, 6) or None, labelsn (m, 5) (without detections also (m,) classes).  The confusion matrix skips an image without labels like val.py:84-109;
        the counting metrics count every image, as the script does."""
        cm, ct, dev = self.confusion_matrix, self.count_metrics, labelsn.device
        matrix = cm._buffer(dev) if cm is not None and labelsn.shape[0] else None
        counts = ct._buffer(dev) if ct is not None else None
        if matrix is None and counts is None:
            return
        kw = dict(cm_conf=cm.conf, cm_iou=cm.iou_thres) if cm is not None else {}
        if ct is not None:
            kw.update(cnt_conf=ct.conf, cnt_iou=ct.iou, trunc_labels=ct.trunc_labels)
        hip.val_confusion(*_one_image(predn, labelsn, dev), self.nc, matrix=matrix, counts=counts, **kw)      # both parts in one launch

    def update_metrics(self, preds, batch):
        """preds: list of (n_i, 6) tensors from `postprocess`; batch: the dataloader dict (img, cls, bboxes, batch_idx, ori_shape, ratio_pad).
        Everything stays on the device: boxes are rescaled to native space by mgdt_scale_boxes, the whole batch is matched by one mgdt_val_match_fwd."""
        rows, counts_dev, counts = self._padded_rows(preds, 6)
        lab = self._label_census(batch, len(preds))
        predn = self._native_space(batch, rows, counts, lab)
        self._append_stats(rows, counts, lab, None if lab.labels is None else self.match_batch(predn, counts_dev, lab.labels, lab.nlab))
        if self.confusion_matrix is None and self.count_metrics is None:
            return
        for si, (npr, nl, off) in enumerate(zip(counts, lab.nl, lab.off)):
            labelsn = lab.native[off:off + nl]
            if npr == 0 and self.count_metrics is None:
                labelsn = labelsn[:, 0]                         # the matrix reads the classes alone (val.py:88): zero boxes; the counters compare boxes
            self._update_extras(predn[si, :npr] if npr else None, labelsn)

    def get_stats(self):
        """val.py:123-131 + DetMetrics.process: `ap_per_class` once per entry of `_STATS` (boxes; a task adds its masks or keypoints) -> the summary
        dict; keeps ap_class_index, nt_per_class and the AP matrices.  With init_metrics(confusion=True / counting=True) also `confusion_matrix` (the
        object) and the flat `metrics/count_*` keys."""
        out = self._map_stats()
        if self.confusion_matrix is not None:
            out['confusion_matrix'] = self.confusion_matrix
        if self.count_metrics is not None:
            out.update(self.count_metrics.results_dict)
        return out

    def _map_stats(self):
        if not self.stats:
            return {}
        *tps, conf, pcls, tcls = [torch.cat(x, 0) for x in zip(*self.stats)]
        self.nt_per_class = np.bincount(tcls.cpu().numpy().astype(int), minlength=self.nc)
        out = {}
        for suffix, col, attr in self._STATS:
            if not (len(tps[col]) and bool(tps[0].any())):        # val.py:126: the gate is the box matrix, for every entry
                out.update({k + suffix: 0.0 for k in _KEYS})
                continue
            _, _, p, r, _, ap, ap_class = ap_per_class(tps[col], conf, pcls, tcls, device=self.device)
            self.ap_class_index = ap_class
            setattr(self, attr, ap)
            out.update({_KEYS[0] + suffix: float(p.mean()), _KEYS[1] + suffix: float(r.mean()), _KEYS[2] + suffix: float(ap[:, 0].mean()),
                        _KEYS[3] + suffix: float(ap.mean())})
        return out

    def match_batch(self, det, ndet, labels, nlab):
        """Whole batch in one launch: det (B, max_det, 6) + ndet (B,) int32 exactly as `mgdt_yolo_amd.ops.nms` returns them, labels
        (B, max_lab, 5) zero-padded + nlab (B,) int32 -> correct (B, max_det, 10) bool (rows past ndet are False)."""
        return hip.val_match(det, ndet, labels, nlab, self.iouv.to(det.device))

    # ---- host tooling that stays out ---------------------------------------------------------------------------------------------------
    def _host_tooling(self, *a, **k):
        raise RuntimeError(f'{type(self).__name__}: plots, the confusion matrix and COCO JSON / pycocotools export are host-side tooling outside the '
                           'validation path')

    pred_to_json = eval_json = plot_val_samples = plot_predictions = _host_tooling
