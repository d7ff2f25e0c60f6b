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
from ..detect.val import DetectionValidator

__all__ = ('PoseValidator',)

_KEYS = ('metrics/precision', 'metrics/recall', 'metrics/mAP50', 'metrics/mAP50-95')


class PoseValidator(DetectionValidator):
    def __init__(self, device='cuda:0', args=None):
        super().__init__(device)
        for k in ('plots', 'save_json', 'single_cls', 'save_hybrid'):
            if (args or {}).get(k):
                raise RuntimeError(f'PoseValidator: {k}=True is host-side tooling (plots, confusion matrix, COCO JSON / pycocotools, class merging) '
                                   f'outside the validation path')
        self._nms = None
        self._sigma_dev = None

    # ---- val.py:45-51 ---------------------------------------------------------------------------------------------------------------------
    def init_metrics(self, nc=1, conf=0.001, iou=0.7, max_det=300, kpt_shape=(17, 3)):
        from ...utils.metrics import OKS_SIGMA
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
        """val.py:23-27: tensors of the dataloader dict go to the device, keypoints as float.  The host copy of batch_idx is kept so that the label
        counts cost no device read."""
        batch = dict(batch)
        batch['batch_idx_host'] = batch['batch_idx'].detach().cpu()
        for k in ('img', 'cls', 'bboxes', 'batch_idx'):
            batch[k] = batch[k].to(self.device, non_blocking=True)
        batch['keypoints'] = batch['keypoints'].to(self.device, non_blocking=True).float()
        return batch

    def postprocess(self, preds):
        """val.py:34-43: NMS with the validator's settings -> list of (n_i, 6 + nk) rows.  The padded batch form of the same rows is kept for
        `update_metrics`."""
        from ...utils import ops
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
        one = lambda k: torch.full((1,), k, dtype=torch.int32, device=dev)
        det = detections.float().contiguous()[None]
        lab = labels.float().contiguous()[None]
        pk = pred_kpts.float().contiguous().view(1, n, gt_kpts.shape[1], -1)
        return self.match_kpts(det, one(n), pk, lab, one(m), gt_kpts.float().contiguous()[None])[0]

    # ---- val.py:53-102 --------------------------------------------------------------------------------------------------------------------
    def update_metrics(self, preds, batch):
        """preds: `postprocess`'s rows per image; batch: the dataloader dict after `preprocess` (img, cls, bboxes, batch_idx, keypoints
        (n, nkpt, 3) normalised - (n, nkpt, 2) gets the visibility column the reference's dataset appends - ori_shape, ratio_pad).  Appends
        (correct_bboxes, correct_kpts, conf, pcls, tcls) per image."""
        from ...utils import ops
        dev = self.device
        per = preds
        b = len(per)
        nkpt, ndim = self.kpt_shape
        nk = nkpt * ndim
        if self._nms is not None and self._nms[0] is per:
            _, rows, counts_dev, counts = self._nms
        else:                                                     # rows that did not come from `postprocess`: pad them (sizes are known, no read)
            counts = [int(p.shape[0]) for p in per]
            rows = torch.zeros(b, max(max(counts), 1), 6 + nk, dtype=torch.float32, device=dev)
            for i, p in enumerate(per):
                rows[i, :counts[i]] = p
            counts_dev = torch.tensor(counts, dtype=torch.int32).to(dev)
        if rows.shape[2] != 6 + nk:
            raise RuntimeError(f'PoseValidator: rows of {rows.shape[2]} columns do not hold 6 + {nkpt} x {ndim} values')
        in_shape = tuple(batch['img'].shape[2:])
        height, width = in_shape
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
        kpts = batch['keypoints'].to(dev).float()
        if kpts.dim() != 3 or kpts.shape[0] != bidx.numel() or kpts.shape[1] != nkpt or kpts.shape[2] not in (2, 3):
            raise RuntimeError(f'PoseValidator: keypoints {tuple(kpts.shape)} for {bidx.numel()} labels of {nkpt} keypoints')
        if kpts.shape[2] == 2:                                    # yolo/data/utils.py:124-128: visible unless a coordinate is negative
            kpts = torch.cat((kpts, ((kpts[..., 0] >= 0) & (kpts[..., 1] >= 0)).float()[..., None]), 2)
        if not sorted_idx:
            order = torch.sort(bidx_host, stable=True).indices.to(dev)
            bidx, cls, bbox, kpts = bidx[order], cls[order], bbox[order], kpts[order]
        max_lab = max(nl_host) if nl_host else 0
        predn = rows[:, :, :6].clone()
        loff, acc = [], 0
        for n in nl_host:
            loff.append(acc)
            acc += n
        if max_lab:
            whwh = torch.tensor((width, height, width, height), dtype=torch.float32, device=dev)
            tbox = ops.xywh2xyxy(bbox.contiguous()) * whwh
        meta = []
        for si in range(b):
            shape, rp = batch['ori_shape'][si], batch['ratio_pad'][si]
            if counts[si]:
                ops.scale_boxes(in_shape, predn[si, :counts[si]], shape, ratio_pad=rp)                       # native-space pred
            if nl_host[si]:
                ops.scale_boxes(in_shape, tbox[loff[si]:loff[si] + nl_host[si]], shape, ratio_pad=rp)       # native-space labels
            m = hip.pose_scale_meta(in_shape, shape)
            if rp is not None:
                m[0], m[1], m[2] = float(rp[0][0]), float(rp[1][0]), float(rp[1][1])
            meta.append(m)
        correct_b = correct_k = None
        if max_lab and max(counts):
            meta = torch.tensor(meta, dtype=torch.float32).to(dev)
            nlab = torch.tensor(nl_host, dtype=torch.int32).to(dev)
            lab_off = torch.tensor(loff, dtype=torch.int32).to(dev)
            pos = torch.arange(bidx.numel(), device=dev) - lab_off.long()[bidx]
            labels = torch.zeros(b, max_lab, 5, dtype=torch.float32, device=dev)
            labels[bidx, pos] = torch.cat((cls, tbox), 1)
            tk = torch.zeros(b, max_lab, nkpt, 3, dtype=torch.float32, device=dev)
            tk[bidx, pos] = kpts * torch.tensor((width, height, 1), dtype=torch.float32, device=dev)          # val.py:91-93
            hip.pose_scale(tk.view(b, max_lab, nkpt * 3), nlab, meta, nkpt * 3, 3, lead=0)                    # native-space label keypoints
            pk = rows[:, :, 6:].contiguous()
            hip.pose_scale(pk, counts_dev, meta, nk, ndim, lead=0)                                            # native-space predicted keypoints
            correct_b, correct_k = self.match_batch(predn, counts_dev, pk.view(b, rows.shape[1], nkpt, ndim), labels, nlab, tk)
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
                cb = ck = torch.zeros(npr, self.niou, dtype=torch.bool, device=dev)
            else:
                cb, ck = correct_b[si, :npr], correct_k[si, :npr]
            self.stats.append((cb, ck, rows[si, :npr, 4], rows[si, :npr, 5], tcls))

    def get_stats(self):
        """val.py / PoseMetrics.process: ap_per_class once with the box matches and once with the keypoint matches -> the eight summary numbers.
        Keeps ap_class_index, nt_per_class, ap (boxes) and ap_pose."""
        from ...utils.metrics import ap_per_class
        if not self.stats:
            return {}
        tp, tpk, conf, pcls, tcls = [torch.cat(x, 0) for x in zip(*self.stats)]
        self.nt_per_class = np.bincount(tcls.cpu().numpy().astype(int), minlength=self.nc)
        out = {}
        for suffix, t, attr in (('(B)', tp, 'ap'), ('(P)', tpk, 'ap_pose')):
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
        raise RuntimeError('PoseValidator: plots, the confusion matrix and COCO JSON / pycocotools export are host-side tooling outside the '
                           'validation path')

    pred_to_json = eval_json = plot_val_samples = plot_predictions = _host_tooling
