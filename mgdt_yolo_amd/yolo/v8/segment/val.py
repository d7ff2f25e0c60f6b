"""reference: yolo/v8/segment/val.py:17-166 - the segmentation task's validator: box AND mask matching on the device.

Per batch: one NMS launch with the mask coefficients (`nms_masks_batch`, whose read of the counts is the only host sync), one mask launch
(`process_mask_batch`, uint8 masks of the whole batch), one mask-IoU launch (mgdt_mask_iou_fwd: the index-map ground truth of
`overlap_mask=True` is expanded inside the kernel, never as the reference's (nl, H, W) repeat) and two match launches (boxes:
mgdt_val_match_fwd, masks: mgdt_val_match_iou_fwd).  Boxes are compared in native image space (`scale_boxes`, one launch per image as in
DetectionValidator, whose batch core `update_metrics` is built from), masks at the mask routine's resolution, as in the reference.  `get_stats`
is the detection validator's with the `(M)` entry of `_STATS` (ap_mask).  `single_cls`, plots, the confusion matrix and `pred_to_json` /
pycocotools are host tooling outside this package: they raise."""
import torch

from .... import ops as hip
from ...utils import ops
from ...utils.metrics import _one_image
from ..detect.val import DetectionValidator

__all__ = ('SegmentationValidator',)


class SegmentationValidator(DetectionValidator):
    MASK_MODES = ('process_mask', 'process_mask_upsample')       # val.py:35-39: `save_json` selects the second in the reference
    _REFUSAL = "; for the masks of the reference's save_json route use init_metrics(mask_mode='process_mask_upsample')"
    _STATS = (('(B)', 0, 'ap'), ('(M)', 1, 'ap_mask'))

    # ---- val.py:25-57 ---------------------------------------------------------------------------------------------------------------------
    def init_metrics(self, nc=80, conf=0.001, iou=0.7, max_det=300, overlap_mask=True, mask_mode='process_mask'):
        if mask_mode not in self.MASK_MODES:
            raise RuntimeError(f'SegmentationValidator: mask_mode {mask_mode!r} is not one of {self.MASK_MODES}')
        super().init_metrics(nc, conf, iou, max_det)
        self.overlap_mask, self.mask_mode = bool(overlap_mask), mask_mode

    def preprocess(self, batch):
        """The detection validator's, and the masks, which stay 8-bit (index maps 0 .. 255 or 0 / 1 instance masks: the reference's `.float()` holds
        the same integers)."""
        batch = super().preprocess(batch)
        batch['masks'] = batch['masks'].to(self.device, non_blocking=True).to(torch.uint8)
        return batch

    def postprocess(self, preds):
        """val.py:46-57: NMS with the validator's settings -> (list of (n_i, 6 + nm) rows, protos).  The padded batch form of the same rows is kept
        for `update_metrics`."""
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
        det, cnt_n, lab, cnt_m = _one_image(detections, labels, dev)
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        pm = pred_masks.to(torch.uint8).contiguous()
        gt = gt_masks.to(torch.uint8).contiguous()
        return self.match_masks(det, cnt_n, pm, lab, cnt_m, gt, overlap=overlap, offsets=zero, lab_offsets=zero, n_labels=m)[0]

    # ---- val.py:59-111 --------------------------------------------------------------------------------------------------------------------
    def update_metrics(self, preds, batch):
        """preds: `postprocess`'s (rows per image, protos); batch: the dataloader dict after `preprocess` (img, cls, bboxes, batch_idx, masks,
        ori_shape, ratio_pad).  Appends (correct_bboxes, correct_masks, conf, pcls, tcls) per image."""
        per, proto = preds
        rows, counts_dev, counts = self._padded_rows(per, 6 + proto.shape[1])
        masks = ops.process_mask_batch(proto, rows, counts_dev, tuple(batch['img'].shape[2:]), self.mask_mode, torch.uint8, counts_host=counts)
        lab = self._label_census(batch, len(per))
        gt = batch['masks'].to(self.device, torch.uint8)
        if lab.order is not None and not self.overlap_mask:        # instance masks follow their labels; an index map numbers them per image
            gt = gt[lab.order]
        predn = self._native_space(batch, rows, counts, lab)
        correct = None, None
        if lab.labels is not None:
            correct = self.match_batch(predn, counts_dev, masks, lab.labels, lab.nlab, gt.contiguous(), overlap=self.overlap_mask, lab_offsets=lab.lab_off,
                                       n_labels=sum(lab.nl))
        self._append_stats(rows, counts, lab, *correct)
