"""reference: yolo/v8/classify/predict.py:9-37 + yolo/data/augment.py:794-801, :873-899 - the classification task's predictor plug-in."""
import numpy as np
import torch

from .... import _lib as L
from .... import ops as hip
from ...engine.predictor import BasePredictor

__all__ = ('ClassificationPredictor', 'classify_transforms', 'classify_crop')


def classify_crop(shape):
    """(top, left, m) of the reference's CenterCrop (augment.py:880-884): the centred square of side m = min(h, w)."""
    h, w = int(shape[0]), int(shape[1])
    m = min(h, w)
    return (h - m) // 2, (w - m) // 2, m


class classify_transforms:
    """`classify_transforms(size)` of the reference with its default mean 0 / std 1: CenterCrop(size) + ToTensor.  image: uint8 (h, w, 3) BGR on
    the device (or a numpy array, copied once) -> uint8 (3, size, size) RGB planes; the division by 255 is the first convolution's loader, as in
    the detection predictor.  The crop geometry is the reference's exactly; the resize is the letter-box kernel's (the cv2.INTER_LINEAR rule for
    8-bit images, a copy when the crop already is size x size) - cv2 is absent where the fixtures are made, so the interpolation is unpinned,
    exactly as LetterBox's."""

    def __init__(self, size=224):
        if not isinstance(size, int):
            raise TypeError(f'classify_transforms() size {size} must be integer, not (list, tuple)')
        self.size = size

    def __call__(self, image, out=None):
        img = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image)).to('cuda:0')
        hip._need_gpu(img)
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or img.stride(2) != 1 or img.stride(1) != 3:
            raise RuntimeError('classify_transforms: expected a uint8 (h, w, 3) image with packed pixels')
        top, left, m = classify_crop(img.shape)
        s = self.size
        if out is None:
            out = torch.empty(3, s, s, dtype=torch.uint8, device=img.device)
        elif tuple(out.shape) != (3, s, s) or not out.is_contiguous():
            raise RuntimeError(f'classify_transforms: out must be a contiguous (3, {s}, {s}) uint8 tensor')
        crop = img[top:top + m, left:left + m]                  # a view: the kernel reads it through the source pitch
        L.check(L.lib().mgdt_letterbox_fwd(hip.ptr(crop), m, m, img.stride(0), hip.ptr(out), s, s, s, s, 0, 0, hip.stream()), 'classify_transforms')
        return out


class ClassificationPredictor(BasePredictor):
    """Results are the per-image probability rows (nc,) fp32 on the device (the reference wraps the same row in `Results(probs=...)`).  Sources: a
    list of uint8 (h, w, 3) BGR images, or an already prepared (N, 3, h, w) device tensor."""

    def __init__(self, overrides=None):
        overrides = dict(overrides or {})
        overrides.setdefault('imgsz', 224)
        super().__init__(overrides)
        self.args.task = 'classify'

    def pre_transform(self, im):
        size = self.imgsz if isinstance(self.imgsz, int) else int(self.imgsz[0])
        tf = classify_transforms(size)
        dev = lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        return [tf(dev(x)) for x in im]

    def postprocess(self, preds, img, orig_imgs):
        preds = preds[0] if isinstance(preds, (list, tuple)) else preds
        return [preds[i] for i in range(preds.shape[0])]
