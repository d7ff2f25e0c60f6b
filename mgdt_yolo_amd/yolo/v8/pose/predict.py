"""reference: yolo/v8/pose/predict.py:8-41 - the pose task's predictor plug-in."""
import torch

from ...engine.predictor import DetectionPredictor

__all__ = ('PosePredictor',)


class PosePredictor(DetectionPredictor):
    """Results are, per image, `(boxes (n, 6) [x1, y1, x2, y2, conf, cls], keypoints (n, *kpt_shape))` in ORIGINAL image coordinates, boxes rounded
    to whole pixels as the reference does (predict.py:30; it wraps the same two tensors in a `Results` container).  For an already prepared
    (N, 3, h, w) tensor source the original shape is the tensor's own (gain 1, no padding: clip and round only).  Device work of postprocess: one
    NMS launch, one host read of the counts, one mgdt_pose_scale_fwd launch for the batch."""

    def __init__(self, overrides=None):
        super().__init__(overrides)
        self.args.task = 'pose'

    def postprocess(self, preds, img, orig_imgs):
        from .... import ops as hip
        from ...utils import ops
        pred = preds[0] if isinstance(preds, (list, tuple)) else preds
        head = self.model.model.model[-1]
        kpt_shape = tuple(head.kpt_shape)
        nk, nc = head.nk, len(self.model.names)
        if pred.shape[1] != 4 + nc + nk:
            raise RuntimeError(f'PosePredictor: the prediction has {pred.shape[1]} rows, expected 4 + nc={nc} + nk={nk}')
        b = pred.shape[0]
        if self.args.classes is not None and len(self.args.classes) == 0:
            return [(torch.zeros((0, 6), device=pred.device), torch.zeros((0, *kpt_shape), device=pred.device))] * b
        per, rows, counts_dev, counts = ops.nms_masks_batch(pred, nk, self.args.conf, self.args.iou, classes=self.args.classes,
                                                            agnostic=self.args.agnostic_nms, max_det=self.args.max_det)
        in_shape = tuple(img.shape[2:])
        tensor_src = isinstance(orig_imgs, torch.Tensor)
        meta = [hip.pose_scale_meta(in_shape, in_shape if tensor_src else tuple(orig_imgs[i].shape[:2])) for i in range(b)]
        hip.pose_scale(rows, counts_dev, torch.tensor(meta, dtype=torch.float32).to(pred.device), nk, kpt_shape[1])
        return [(per[i][:, :6], per[i][:, 6:].reshape(counts[i], *kpt_shape)) for i in range(b)]
