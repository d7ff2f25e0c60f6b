"""reference: yolo/v8/segment/val.py:17-166 - the segmentation task's validator: box AND mask matching on the device.

Per batch: one NMS launch with the mask coefficients (`nms_masks_batch`, whose read of the counts is the only host sync), one mask launch
(`process_mask_batch`, uint8 masks of the whole batch), one mask-IoU launch (mgdt_mask_iou_fwd: the index-map ground truth of
`overlap_mask=True` is expanded inside the kernel, never as the reference's (nl, H, W) repeat) and two match launches (boxes:
mgdt_val_match_fwd, masks: mgdt_val_match_iou_fwd).  Boxes are compared in native image space (`scale_boxes`, one launch per image as in
DetectionValidator), masks at the mask routine's resolution, as in the reference.  `single_cls`, plots, the confusion matrix and
`pred_to_json` / pycocotools are host tooling outside this package: they raise."""
import torch

from .... import ops as hip
from ..detect.val import DetectionValidator

__all__ = ('SegmentationValidator',)

_KEYS = ('metrics/precision', 'metrics/recall', 'metrics/mAP50', 'metrics/mAP50-95')


class SegmentationValidator(DetectionValidator):
    MASK_MODES = ('process_mask', 'process_mask_upsample')       # val.py:35-39: `save_json` selects the second in the reference

    def __init__(self, device='cuda:0', args=None):
        super().__init__(device)
        for k in ('plots', 'save_json', 'single_cls', 'save_hybrid'):
            if (args or {}).get(k):
                raise RuntimeError(f'SegmentationValidator: {k}=True is host-side tooling (plots, confusion matrix, COCO JSON / pycocotools, class merging) '
                                   f"outside the validation path; for the masks of the reference's save_json route use init_metrics(mask_mode='process_mask_upsample')")
        self._nms = None

    # ---- val.py:25-57 ---------------------------------------------------------------------------------------------------------------------
    def init_metrics(self, nc=80, conf=0.001, iou=0.7, max_det=300, overlap_mask=True, mask_mode='process_mask'):
        if mask_mode not in self.MASK_MODES:
            raise RuntimeError(f'SegmentationValidator: mask_mode {mask_mode!r} is not one of {self.MASK_MODES}')
        super().init_metrics(nc, conf, iou, max_det)
        self.overlap_mask, self.mask_mode = bool(overlap_mask), mask_mode

    def preprocess(self, batch):
        """Tensors of the dataloader dict go to the device; masks stay 8-bit (index maps 0 .. 255 or 0 / 1 instance masks: the reference's
        `.float()` holds the same integers).  The host copy of batch_idx is kept so that the label counts cost no device read."""
        batch = dict(batch)
        batch['batch_idx_host'] = batch['batch_idx'].detach().cpu()
        for k in ('img', 'cls', 'bboxes', 'batch_idx'):
            batch[k] = batch[k].to(self.device, non_blocking=True)
        batch['masks'] = batch['masks'].to(self.device, non_blocking=True).to(torch.uint8)
        return batch

    def postprocess(self, preds):
        """val.py:46-57: NMS with the validator's settings -> (list of (n_i, 6 + nm) rows, protos).  The padded batch form of the same rows is kept
        for `update_metrics`."""
        from ...utils import ops
        proto = preds[1][-1] if len(preds[1]) == 3 else preds[1]        # (feats, mc, p) of the model, p alone of an exported one
        per, rows, counts_dev, counts = ops.nms_masks_batch(preds[0], proto.shape[1], self.conf, self.iou, multi_label=True, max_det=self.max_det)
        self._nms = (per, rows, counts_dev, counts)
        return per, proto

    # ---- val.py:131-166 -------------------------------------------------------------------------------------------------------------------
    def match_masks(self, rows, counts, masks, labels, nlab, gt, overlap=True, offsets=None, lab_offsets=None, n_labels=None):
        """The mask half of `match_batch`: one IoU launch and one match launch (plus the resampling launch when the ground truth has another
        size than the masks) -> correct_masks (B, max_det, 10) bool.  Only column 5 (the class) of `rows` is read, in place, whatever the row
        width.  n_labels: sum(nlab) when the caller knows it on the host (sizes the resampled ground truth; else B * max_lab, an upper bound that
        needs no device read)."""
        iouv = self.iouv.to(rows.device)
        b, max_det, max_lab = rows.shape[0], rows.shape[1], labels.shape[1]
        if offsets is None:
            offsets = hip.exclusive_offsets(counts)
        if lab_offsets is None:
            lab_offsets = hip.exclusive_offsets(nlab)
        if tuple(gt.shape[1:]) != tuple(masks.shape[1:]):
            total = gt.shape[0] if not overlap else (b * max_lab if n_labels is None else int(n_labels))
            gt = hip.gt_masks_resample(gt, nlab, lab_offsets, total, max_lab, masks.shape[1:], index_map=overlap)
            overlap = False
        iou = hip.mask_iou_batch(masks, counts, offsets, max_det, gt, nlab, max_lab, index_map=overlap, lab_offsets=lab_offsets)
        return hip.val_match_iou(iou, rows, counts, labels, nlab, iouv)

    def match_batch(self, rows, counts, masks, labels, nlab, gt, overlap=True, offsets=None, lab_offsets=None, n_labels=None):
        """The batch form: rows (B, max_det, >= 6) fp32 detection rows in the labels' box frame + counts (B,) int32 as `nms_masks_batch` returns
        them, masks (sum(counts), H, W) uint8 as `process_mask_batch` returns them, labels (B, max_lab, 5) [cls, x1, y1, x2, y2] zero-padded +
        nlab (B,) int32, gt the (B, h, w) uint8 index maps (overlap=True) or (sum(nlab), h, w) uint8 instance masks -> (correct_bboxes,
        correct_masks), each (B, max_det, 10) bool.  One IoU launch and two match launches (plus the resampling launch when h, w differ from
        H, W); nothing is read back.  The box matcher takes 6-float rows, so wider rows are copied to (B, max_det, 6) for it; the mask matcher
        reads the classes from `rows` as given.  NOTE: this replaces DetectionValidator.match_batch(det, ndet, labels, nlab), which returns the box
        matrix alone; the positional signatures are not compatible."""
        det6 = rows if rows.shape[2] == 6 else rows[:, :, :6].contiguous()
        correct_b = hip.val_match(det6, counts, labels, nlab, self.iouv.to(rows.device))
        return correct_b, self.match_masks(rows, counts, masks, labels, nlab, gt, overlap, offsets, lab_offsets, n_labels)

    def _process_batch(self, detections, labels, pred_masks=None, gt_masks=None, overlap=False, masks=False):
        """One image, the reference's signature and return: detections (N, 6), labels (M, 5) -> correct (N, 10) bool; with masks=True from the mask
        IoU of pred_masks (N, H, W) against gt_masks ((1, h, w) index map when `overlap`, else (M, h, w)); the boxes are not looked at then."""
        if not masks:
            return super()._process_batch(detections, labels)
        n, m = detections.shape[0], labels.shape[0]
        dev = detections.device
        if n == 0 or m == 0:
            return torch.zeros(n, self.niou, dtype=torch.bool, device=dev)
        one = lambda k: torch.full((1,), k, dtype=torch.int32, device=dev)
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        det = detections.float().contiguous()[None]
        lab = labels.float().contiguous()[None]
        pm = pred_masks.to(torch.uint8).contiguous()
        gt = gt_masks.to(torch.uint8).contiguous()
        return self.match_masks(det, one(n), pm, lab, one(m), gt, overlap=overlap, offsets=zero, lab_offsets=zero, n_labels=m)[0]

    # ---- val.py:59-111 --------------------------------------------------------------------------------------------------------------------
    def update_metrics(self, preds, batch):
        """preds: `postprocess`'s (rows per image, protos); batch: the dataloader dict after `preprocess` (img, cls, bboxes, batch_idx, masks,
        ori_shape, ratio_pad).  Appends (correct_bboxes, correct_masks, conf, pcls, tcls) per image."""
        from ...utils import ops
        dev = self.device
        per, proto = preds
        b = len(per)
        if self._nms is not None and self._nms[0] is per:
            _, rows, counts_dev, counts = self._nms
        else:                                                     # rows that did not come from `postprocess`: pad them (sizes are known, no read)
            counts = [int(p.shape[0]) for p in per]
            rows = torch.zeros(b, max(max(counts), 1), 6 + proto.shape[1], dtype=torch.float32, device=dev)
            for i, p in enumerate(per):
                rows[i, :counts[i]] = p
            counts_dev = torch.tensor(counts, dtype=torch.int32).to(dev)
        in_shape = tuple(batch['img'].shape[2:])
        height, width = in_shape
        masks = ops.process_mask_batch(proto, rows, counts_dev, in_shape, self.mask_mode, torch.uint8, counts_host=counts)
        # labels: counts from the host copy of batch_idx; grouped by image in their given order
        bidx_host = batch.get('batch_idx_host')
        if bidx_host is None:
            bidx_host = batch['batch_idx'].detach().cpu()
        bidx_host = bidx_host.long().view(-1)
        nl_host = torch.bincount(bidx_host, minlength=b)[:b].tolist()
        sorted_idx = bool((bidx_host[1:] >= bidx_host[:-1]).all()) if bidx_host.numel() > 1 else True
        bidx = batch['batch_idx'].to(dev).long().view(-1)
        cls = batch['cls'].to(dev).float().view(-1, 1)
        bbox = batch['bboxes'].to(dev).float().view(-1, 4)
        gt = batch['masks'].to(dev)
        if gt.dtype != torch.uint8:
            gt = gt.to(torch.uint8)
        if not sorted_idx:
            order = torch.sort(bidx_host, stable=True).indices.to(dev)
            bidx, cls, bbox = bidx[order], cls[order], bbox[order]
            if not self.overlap_mask:
                gt = gt[order]
        gt = gt.contiguous()
        max_lab = max(nl_host) if nl_host else 0
        predn = rows[:, :, :6].clone()
        loff, acc = [], 0
        for n in nl_host:
            loff.append(acc)
            acc += n
        if max_lab:
            whwh = torch.tensor((width, height, width, height), dtype=torch.float32, device=dev)
            tbox = ops.xywh2xyxy(bbox.contiguous()) * whwh
        for si in range(b):
            shape, rp = batch['ori_shape'][si], batch['ratio_pad'][si]
            if counts[si]:
                ops.scale_boxes(in_shape, predn[si, :counts[si]], shape, ratio_pad=rp)                       # native-space pred
            if nl_host[si]:
                ops.scale_boxes(in_shape, tbox[loff[si]:loff[si] + nl_host[si]], shape, ratio_pad=rp)       # native-space labels
        correct_b = correct_m = None
        if max_lab and max(counts):
            nlab = torch.tensor(nl_host, dtype=torch.int32).to(dev)
            lab_off = torch.tensor(loff, dtype=torch.int32).to(dev)
            labels = torch.zeros(b, max_lab, 5, dtype=torch.float32, device=dev)
            pos = torch.arange(bidx.numel(), device=dev) - lab_off.long()[bidx]
            labels[bidx, pos] = torch.cat((cls, tbox), 1)
            correct_b, correct_m = self.match_batch(predn, counts_dev, masks, labels, nlab, gt, overlap=self.overlap_mask, lab_offsets=lab_off,
                                                    n_labels=sum(nl_host))
        for si in range(b):
            npr, nl = counts[si], nl_host[si]
            tcls = cls[loff[si]:loff[si] + nl, 0]
            self.seen += 1
            if npr == 0:
                if nl:
                    empty = torch.zeros(0, self.niou, dtype=torch.bool, device=dev)
                    self.stats.append((empty, empty, *torch.zeros((2, 0), device=dev), tcls))
                continue
            if correct_b is None:
                cb = cm = torch.zeros(npr, self.niou, dtype=torch.bool, device=dev)
            else:
                cb, cm = correct_b[si, :npr], correct_m[si, :npr]
            self.stats.append((cb, cm, rows[si, :npr, 4], rows[si, :npr, 5], tcls))

    def get_stats(self):
        """val.py / SegmentMetrics.process: ap_per_class once with the box matches and once with the mask matches -> the eight summary numbers.
        Keeps ap_class_index, nt_per_class, ap (boxes) and ap_mask."""
        import numpy as np
        from ...utils.metrics import ap_per_class
        if not self.stats:
            return {}
        tp, tpm, conf, pcls, tcls = [torch.cat(x, 0) for x in zip(*self.stats)]
        self.nt_per_class = np.bincount(tcls.cpu().numpy().astype(int), minlength=self.nc)
        out = {}
        for suffix, t, attr in (('(B)', tp, 'ap'), ('(M)', tpm, 'ap_mask')):
            if not (len(t) and bool(tp.any())):                   # val.py:126 of the detection validator: the gate is the box matrix
                out.update({k + suffix: 0.0 for k in _KEYS})
                continue
            _, _, p, r, _, ap, ap_class = ap_per_class(t, conf, pcls, tcls, device=self.device)
            self.ap_class_index = ap_class
            setattr(self, attr, ap)
            out.update({_KEYS[0] + suffix: float(p.mean()), _KEYS[1] + suffix: float(r.mean()), _KEYS[2] + suffix: float(ap[:, 0].mean()),
                        _KEYS[3] + suffix: float(ap.mean())})
        return out

    # ---- host tooling that stays out ---------------------------------------------------------------------------------------------------
    def _host_tooling(self, *a, **k):
        raise RuntimeError('SegmentationValidator: plots, the confusion matrix and COCO JSON / pycocotools export are host-side tooling outside the '
                           'validation path')

    pred_to_json = eval_json = plot_val_samples = plot_predictions = _host_tooling
