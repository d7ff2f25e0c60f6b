"""reference: yolo/v8/segment/predict.py:10-44 - the segmentation task's predictor plug-in."""
import torch

from ...engine.predictor import DetectionPredictor

__all__ = ('SegmentationPredictor',)


class SegmentationPredictor(DetectionPredictor):
    """Results are, per image, `(boxes (n, 6) [x1, y1, x2, y2, conf, cls] in ORIGINAL image coordinates, masks (n, H, W) uint8 0 / 1)` (the
    reference wraps the same two tensors in a `Results` container).  `retina_masks=False` (default): process_mask(upsample=True) at the
    letter-boxed input size, boxes scaled to the original image AFTER the masks; `retina_masks=True`: boxes scaled first, then
    process_mask_native at the original image size (predict.py:34-41).  Device work of postprocess: one NMS launch, one host read of the
    counts, the box scaling launches and one mask launch for the batch (retina masks of images with different original shapes have different
    mask sizes and take one launch per image)."""

    def __init__(self, overrides=None):
        o = dict(retina_masks=False)
        o.update(overrides or {})
        super().__init__(o)
        self.args.task = 'segment'

    def postprocess(self, preds, img, orig_imgs):
        from .... import ops as hip
        from ...utils import ops
        proto = preds[1][-1] if len(preds[1]) == 3 else preds[1]        # (feats, mc, p) of the model, p alone of an exported one
        pred = preds[0]
        nm = proto.shape[1]
        if self.args.classes is not None and len(self.args.classes) == 0:
            return [(torch.zeros((0, 6), device=pred.device), torch.zeros((0, *img.shape[2:]), dtype=torch.uint8, device=pred.device))] * pred.shape[0]
        per, rows, counts_dev, counts = ops.nms_masks_batch(pred, nm, self.args.conf, self.args.iou, classes=self.args.classes,
                                                            agnostic=self.args.agnostic_nms, max_det=self.args.max_det)
        b = len(per)
        in_shape = tuple(img.shape[2:])
        tensor_src = isinstance(orig_imgs, torch.Tensor)
        shapes = [in_shape if tensor_src else tuple(orig_imgs[i].shape[:2]) for i in range(b)]

        def scale(i):
            if not tensor_src and counts[i]:
                ops.scale_boxes(in_shape, per[i], shapes[i])                # in place on rows[i, :n, :4] (rows of 6+nm floats)

        if self.args.retina_masks:
            for i in range(b):
                scale(i)
            if all(s == shapes[0] for s in shapes):
                flat = ops.process_mask_batch(proto, rows, counts_dev, shapes[0], 'process_mask_native', torch.uint8, counts_host=counts)
                masks = self._split(flat, counts)
            else:
                p = ops._protos_nhwc(proto)
                masks = [hip.seg_masks(p[i:i + 1], rows[i:i + 1], counts_dev[i:i + 1], counts[i:i + 1], shapes[i], 'process_mask_native', torch.uint8)
                         for i in range(b)]
        else:
            flat = ops.process_mask_batch(proto, rows, counts_dev, in_shape, 'process_mask_up', torch.uint8, counts_host=counts)
            masks = self._split(flat, counts)
            for i in range(b):
                scale(i)
        return [(per[i][:, :6], masks[i]) for i in range(b)]

    @staticmethod
    def _split(flat, counts):
        out, off = [], 0
        for c in counts:
            out.append(flat[off:off + c])
            off += c
        return out
