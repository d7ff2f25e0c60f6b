"""reference: vit/rtdetr/predict.py - the RT-DETR predictor.  The head is NMS-free: postprocess is one mgdt_rtdetr_post_fwd launch for the batch
(xywh -> xyxy, class maximum, conf threshold, class filter, scaling to each original image) plus one read of the per-image row counts."""
import numpy as np
import torch

from ... import ops
from ...yolo.data.augment import LetterBox
from ...yolo.engine.predictor import BasePredictor

__all__ = ('RTDETRPredictor',)


class RTDETRPredictor(BasePredictor):
    """Results are the per-image (n, 6) [x1, y1, x2, y2, conf, cls] tensors in query order: original-image pixels for a list source, normalised
    to [0, 1] for a tensor source (predict.py:27-29; the reference wraps the same tensor in a `Results` container)."""

    def __init__(self, model=None, overrides=None, **kwargs):
        super().__init__({**(overrides or {}), **kwargs})
        if model is not None:
            self.setup_model(model)

    def pre_transform(self, im):
        """predict.py:35-44: stretched to the (square) input size, no border.  The interpolation is this library's resampling kernel, not cv2's."""
        lb = LetterBox(self.imgsz, auto=False, scaleFill=True)
        dev = lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        return [lb(image=dev(x)) for x in im]

    def postprocess(self, preds, img, orig_imgs):
        bboxes, scores = preds[0][0], preds[1][0]              # (1, B, nq, 4), (1, B, nq, nc)
        b, nq, nc = scores.shape
        wh = None
        if not isinstance(orig_imgs, torch.Tensor):
            wh = torch.tensor([[float(o.shape[1]), float(o.shape[0])] for o in orig_imgs], dtype=torch.float32).to(bboxes.device)
        keep = None
        if self.args.classes is not None:
            keep = torch.zeros(nc, dtype=torch.uint8)
            keep[[int(c) for c in self.args.classes if 0 <= int(c) < nc]] = 1
            keep = keep.to(bboxes.device)
        rows, counts = ops.rtdetr_post(bboxes.contiguous(), scores.contiguous(), self.args.conf, keep, wh)
        return [rows[i, :n] for i, n in enumerate(counts.tolist())]
