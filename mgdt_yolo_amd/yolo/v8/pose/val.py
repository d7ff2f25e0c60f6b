"""reference: yolo/v8/pose/val.py:15-141 - the pose task's validator: box AND keypoint matching on the device.

Per batch: one NMS launch with the keypoints behind the detection columns (`nms_masks_batch` with nm = nk, whose read of the counts is the only
host sync), one mgdt_pose_scale_fwd launch each for the predicted and the label keypoints (`scale_coords` with clipping, lead = 0), one OKS
launch (mgdt_kpt_iou_fwd: the reference's `kpt_iou` for every (label, detection) pair of the batch) and two match launches (boxes:
mgdt_val_match_fwd, keypoints: mgdt_val_match_iou_fwd).  Boxes and keypoints are compared in native image space (`scale_boxes`, one launch per
image as in DetectionValidator).  `single_cls`, plots, the confusion matrix and `pred_to_json` / pycocotools are host tooling outside this
package: they raise."""
import numpy as np
import torch

from .... import ops as hip
from ...utils import ops
from ...utils.metrics import OKS_SIGMA, _one_image
from ..detect.val import DetectionValidator

__all__ = ('PoseValidator',)


class PoseValidator(DetectionValidator):
    _REFUSAL = ''
    _STATS = (('(B)', 0, 'ap'), ('(P)', 1, 'ap_pose'))
    _sigma_dev = None

    # ---- val.py:45-51 ---------------------------------------------------------------------------------------------------------------------
    def init_metrics(self, nc=1, conf=0.001, iou=0.7, max_det=300, kpt_shape=(17, 3)):
        kpt_shape = tuple(int(k) for k in kpt_shape)
        if len(kpt_shape) != 2 or kpt_shape[0] < 1 or kpt_shape[1] not in (2, 3):
            raise RuntimeError(f'PoseValidator: kpt_shape {kpt_shape} is not (nkpt, 2 | 3)')
        super().init_metrics(nc, conf, iou, max_det)
        self.kpt_shape = kpt_shape
        nkpt = kpt_shape[0]
        self.sigma = OKS_SIGMA if kpt_shape == (17, 3) else np.ones(nkpt) / nkpt
        self._sigma_dev = None

    def _sigma(self, dev):
        """sigma as the float32 device tensor the kernel reads (cached: `match_batch` uploads nothing)."""
        if self._sigma_dev is None or self._sigma_dev.device != dev:
            self._sigma_dev = torch.from_numpy(np.asarray(self.sigma, dtype=np.float32)).to(dev)
        return self._sigma_dev

    def preprocess(self, batch):
        """val.py:23-27: the detection validator's, and the keypoints as float."""
        batch = super().preprocess(batch)
        batch['keypoints'] = batch['keypoints'].to(self.device, non_blocking=True).float()
        return batch

    def postprocess(self, preds):
        """val.py:34-43: NMS with the validator's settings -> list of (n_i, 6 + nk) rows.  The padded batch form of the same rows is kept for
        `update_metrics`."""
        nk = self.kpt_shape[0] * self.kpt_shape[1]
        per, rows, counts_dev, counts = ops.nms_masks_batch(preds, nk, self.conf, self.iou, multi_label=True, max_det=self.max_det)
        self._nms = (per, rows, counts_dev, counts)
        return per

    # ---- val.py:110-141 -------------------------------------------------------------------------------------------------------------------
    def match_kpts(self, rows, counts, pred_kpts, labels, nlab, gt_kpts):
        """The keypoint half of `match_batch`: area = w * h * 0.53 of the label boxes (val.py:123) on the device, one OKS launch and one match
        launch -> correct_kpts (B, max_det, 10) bool.  Only column 5 (the class) of `rows` is read, in place, whatever the row width."""
        dev = rows.device
        area = ((labels[:, :, 3] - labels[:, :, 1]) * (labels[:, :, 4] - labels[:, :, 2]) * 0.53).contiguous()
        oks = hip.kpt_iou_batch(pred_kpts, counts, rows.shape[1], gt_kpts, area, nlab, self._sigma(dev))
        return hip.val_match_iou(oks, rows, counts, labels, nlab, self.iouv.to(dev))

    def match_batch(self, rows, counts, pred_kpts, labels, nlab, gt_kpts):
        """The batch form: rows (B, max_det, >= 6) fp32 detection rows in the labels' box frame + counts (B,) int32 as `nms_masks_batch` returns
        them; pred_kpts the keypoints in the labels' frame, a dense (B, max_det, nkpt, 2 | 3) fp32 tensor or (B, max_det, 6 + nk) rows read in
        place (`rows` itself when its keypoint columns are already in that frame); labels (B, max_lab, 5) [cls, x1, y1, x2, y2] zero-padded +
        nlab (B,) int32; gt_kpts (B, max_lab, nkpt, 3) fp32 [x, y, visibility] zero-padded -> (correct_bboxes, correct_kpts), each
        (B, max_det, 10) bool.  One box-match launch, one OKS launch and one match launch on the OKS matrix; nothing is read back.  The box
        matcher takes 6-float rows, so wider rows are copied to (B, max_det, 6) for it.  NOTE: this replaces
        DetectionValidator.match_batch(det, ndet, labels, nlab), which returns the box matrix alone; the positional signatures are not compatible."""
        det6 = rows if rows.shape[2] == 6 else rows[:, :, :6].contiguous()
        correct_b = hip.val_match(det6, counts, labels, nlab, self.iouv.to(rows.device))
        return correct_b, self.match_kpts(rows, counts, pred_kpts, labels, nlab, gt_kpts)

    def _process_batch(self, detections, labels, pred_kpts=None, gt_kpts=None):
        """One image, the reference's signature and return: detections (N, 6), labels (M, 5) -> correct (N, 10) bool; with pred_kpts (N, nkpt, 2 | 3)
        and gt_kpts (M, nkpt, 3) from their OKS (the boxes give the area only)."""
        if pred_kpts is None or gt_kpts is None:
            return super()._process_batch(detections, labels)
        n, m = detections.shape[0], labels.shape[0]
        dev = detections.device
        if n == 0 or m == 0:
            return torch.zeros(n, self.niou, dtype=torch.bool, device=dev)
        det, cnt_n, lab, cnt_m = _one_image(detections, labels, dev)
        pk = pred_kpts.float().contiguous().view(1, n, gt_kpts.shape[1], -1)
        return self.match_kpts(det, cnt_n, pk, lab, cnt_m, gt_kpts.float().contiguous()[None])[0]

    # ---- val.py:53-102 --------------------------------------------------------------------------------------------------------------------
    def update_metrics(self, preds, batch):
        """preds: `postprocess`'s rows per image; batch: the dataloader dict after `preprocess` (img, cls, bboxes, batch_idx, keypoints
        (n, nkpt, 3) normalised - (n, nkpt, 2) gets the visibility column the reference's dataset appends - ori_shape, ratio_pad).  Appends
        (correct_bboxes, correct_kpts, conf, pcls, tcls) per image."""
        dev = self.device
        b = len(preds)
        nkpt, ndim = self.kpt_shape
        nk = nkpt * ndim
        rows, counts_dev, counts = self._padded_rows(preds, 6 + nk)
        if rows.shape[2] != 6 + nk:
            raise RuntimeError(f'PoseValidator: rows of {rows.shape[2]} columns do not hold 6 + {nkpt} x {ndim} values')
        in_shape = tuple(batch['img'].shape[2:])
        lab = self._label_census(batch, b)
        kpts = batch['keypoints'].to(dev).float()
        if kpts.dim() != 3 or kpts.shape[0] != lab.bidx.numel() or kpts.shape[1] != nkpt or kpts.shape[2] not in (2, 3):
            raise RuntimeError(f'PoseValidator: keypoints {tuple(kpts.shape)} for {lab.bidx.numel()} labels of {nkpt} keypoints')
        if kpts.shape[2] == 2:                                    # yolo/data/utils.py:124-128: visible unless a coordinate is negative
            kpts = torch.cat((kpts, ((kpts[..., 0] >= 0) & (kpts[..., 1] >= 0)).float()[..., None]), 2)
        if lab.order is not None:
            kpts = kpts[lab.order]
        predn = self._native_space(batch, rows, counts, lab)
        correct = None, None
        if lab.labels is not None:
            meta = []
            for si in range(b):
                m, rp = hip.pose_scale_meta(in_shape, batch['ori_shape'][si]), batch['ratio_pad'][si]
                if rp is not None:
                    m[0], m[1], m[2] = float(rp[0][0]), float(rp[1][0]), float(rp[1][1])
                meta.append(m)
            meta = torch.tensor(meta, dtype=torch.float32).to(dev)
            max_lab = lab.labels.shape[1]
            tk = torch.zeros(b, max_lab, nkpt, 3, dtype=torch.float32, device=dev)
            tk[lab.bidx, lab.pos] = kpts * torch.tensor((in_shape[1], in_shape[0], 1), dtype=torch.float32, device=dev)      # val.py:91-93
            hip.pose_scale(tk.view(b, max_lab, nkpt * 3), lab.nlab, meta, nkpt * 3, 3, lead=0)                # native-space label keypoints
            pk = rows[:, :, 6:].contiguous()
            hip.pose_scale(pk, counts_dev, meta, nk, ndim, lead=0)                                            # native-space predicted keypoints
            correct = self.match_batch(predn, counts_dev, pk.view(b, rows.shape[1], nkpt, ndim), lab.labels, lab.nlab, tk)
        self._append_stats(rows, counts, lab, *correct)
