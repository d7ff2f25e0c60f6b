"""reference: vit/rtdetr/val.py:69-152 - RTDETRValidator.  `postprocess` is one launch (mgdt_rtdetr_val_post_fwd): all nq rows of every image, no
threshold, sorted by confidence; boxes and labels are compared in each image's native space = normalised coordinates times `ori_shape`, with no
letterbox arithmetic.  Matching, the stats rows, `get_stats` and the confusion / counting extras are the detection validator's."""
import torch

from ... import ops as hip
from ...yolo.utils import ops
from ...yolo.v8.detect.val import DetectionValidator

__all__ = ('RTDETRValidator',)


class RTDETRValidator(DetectionValidator):
    _REFUSAL = ''

    def __init__(self, device='cuda:0', args=None):
        super().__init__(device=device, args=args)
        if (args or {}).get('save_txt'):
            raise RuntimeError(f'{type(self).__name__}: save_txt=True is host-side tooling (plots, confusion matrix, COCO JSON / pycocotools, class merging) '
                               f'outside the validation path{self._REFUSAL}')

    def postprocess(self, preds):
        """val.py:90-106: preds = the model's eval tuple (dec_bboxes (1, B, nq, 4) xywh in [0, 1], dec_scores (1, B, nq, nc), ...) -> list of (nq, 6)
        rows (x1, y1, x2, y2, conf, cls) per image in descending confidence (equal confidences by ascending query index; the reference's argsort
        leaves them unspecified).  The padded batch form is kept for `update_metrics`."""
        bboxes, scores = preds[:2]
        if bboxes.dim() == 4:
            bboxes, scores = bboxes[0], scores[0]
        rows, counts_dev = hip.rtdetr_val_post(bboxes.float().contiguous(), scores.float().contiguous())
        b, nq = rows.shape[:2]
        per = [rows[i] for i in range(b)]
        self._nms = (per, rows, counts_dev, [nq] * b)
        return per

    def _native_space(self, batch, rows, counts, lab):
        """val.py:129-137: predictions and labels (xywh -> xyxy first) times ori_shape (w, h); no ratio_pad."""
        dev = self.device
        wh = torch.tensor([[float(s[1]), float(s[0])] for s in batch['ori_shape']], dtype=torch.float32).to(dev)      # (B, 2) = (w, h)
        scale = torch.cat((wh, wh), 1)                                                                                 # (B, 4)
        predn = rows[:, :, :6].clone()
        predn[:, :, :4] *= scale[:, None, :]
        max_lab = max(lab.nl) if lab.nl else 0
        if max_lab:
            tbox = ops.xywh2xyxy(lab.bbox.contiguous()) * scale[lab.bidx]
        lab.native = torch.cat((lab.cls, tbox), 1) if max_lab else torch.zeros(0, 5, device=dev)
        lab.labels = None
        if max_lab and max(counts):
            lab.nlab = torch.tensor(lab.nl, dtype=torch.int32).to(dev)
            lab.lab_off = torch.tensor(lab.off, dtype=torch.int32).to(dev)
            lab.pos = torch.arange(lab.bidx.numel(), device=dev) - lab.lab_off.long()[lab.bidx]
            lab.labels = torch.zeros(len(counts), max_lab, 5, dtype=torch.float32, device=dev)
            lab.labels[lab.bidx, lab.pos] = lab.native
        return predn

    build_dataset = save_one_txt = DetectionValidator._host_tooling
