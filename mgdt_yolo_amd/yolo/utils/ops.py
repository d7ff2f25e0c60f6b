"""Detection, segmentation and pose post-processing with the reference's names (reference: yolo/utils/ops.py)."""
import torch

from ... import _lib as L
from ... import ops as hip


def _rows(x):
    """(..., k >= 4) cuda fp32 tensor -> contiguous 2-D view + row width (the reference's helpers index the last axis)."""
    hip._need_gpu(x)
    if x.dtype != torch.float32:
        raise RuntimeError('box helpers compute in float32')
    if x.shape[-1] < 4:
        raise RuntimeError(f'expected boxes with >= 4 columns, got {tuple(x.shape)}')
    return x.contiguous().view(-1, x.shape[-1]), x.shape[-1]


def _convert(x, mode):
    rows, k = _rows(x)
    out = torch.empty_like(rows)
    L.check(L.lib().mgdt_box_convert(hip.ptr(rows), hip.ptr(out), rows.shape[0], k, mode, hip.stream()), 'box_convert')
    return out.view(x.shape)


def xywh2xyxy(x):
    """(x, y, w, h) -> (x1, y1, x2, y2) on the last axis, other columns copied (ops.py:362-377)."""
    return _convert(x, 0)


def xyxy2xywh(x):
    """(x1, y1, x2, y2) -> (x, y, w, h) (ops.py:345-359)."""
    return _convert(x, 1)


def clip_boxes(boxes, shape):
    """In-place clip to the image (h, w) (ops.py:269-285)."""
    return scale_boxes(shape, boxes, shape, ratio_pad=((1.0, 1.0), (0.0, 0.0)))


def scale_boxes(img1_shape, boxes, img0_shape, ratio_pad=None):
    """Rescale xyxy boxes (in place, like the reference) from the letter-boxed shape img1_shape (h, w) to the original img0_shape and clip
    them (ops.py:90-117).  `boxes` must be a contiguous view whose rows are >= 4 floats apart (a (n, 4) tensor or pred[:, :4] of (n, 6))."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1), round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1)
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    hip._need_gpu(boxes)
    if boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] < 4 or boxes.stride(1) != 1:
        raise RuntimeError('scale_boxes: expected a 2-D float32 view with unit column stride')
    if boxes.shape[0]:
        L.check(L.lib().mgdt_scale_boxes(hip.ptr(boxes), boxes.shape[0], boxes.stride(0), float(gain), float(pad[0]), float(pad[1]), float(img0_shape[0]),
                                         float(img0_shape[1]), hip.stream()), 'scale_boxes')
    return boxes


def _coords_inplace(coords, meta):
    """One mgdt_pose_scale_fwd launch (lead = 0) on coords (..., 2 | 3) fp32 cuda, in place like the reference's helpers."""
    hip._need_gpu(coords)
    if coords.dtype != torch.float32 or coords.dim() < 1 or coords.shape[-1] not in (2, 3):
        raise RuntimeError(f'keypoint helpers take float32 (..., 2) or (..., 3) coordinates, got {tuple(coords.shape)} {coords.dtype}')
    n = coords.numel() // coords.shape[-1]
    if n == 0:
        return coords
    flat = coords if coords.is_contiguous() else coords.contiguous()
    dev = coords.device
    hip.pose_scale(flat.view(1, n, coords.shape[-1]), torch.tensor([n], dtype=torch.int32).to(dev), torch.tensor([meta], dtype=torch.float32).to(dev),
                   coords.shape[-1], coords.shape[-1], lead=0)
    if flat is not coords:
        coords.copy_(flat)
    return coords


def clip_coords(coords, shape):
    """In-place clip of (..., 2 | 3) keypoint coordinates to the image (h, w): x to [0, w], y to [0, h] (ops.py:288-300)."""
    return _coords_inplace(coords, [1.0, 0.0, 0.0, float(shape[0]), float(shape[1]), 0.0, 0.0, 0.0])


def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None, normalize=False):
    """Rescale keypoint coordinates (in place, like the reference) from the letter-boxed shape img1_shape (h, w) to the original img0_shape and
    clip them (ops.py:636-666): the padding is NOT rounded here, unlike scale_boxes.  coords: float32 (..., 2) or (..., 3) [x, y(, visibility)]."""
    meta = hip.pose_scale_meta(img1_shape, img0_shape, normalize)
    if ratio_pad is not None:
        meta[0], meta[1], meta[2] = ratio_pad[0][0], ratio_pad[1][0], ratio_pad[1][1]
    return _coords_inplace(coords, meta)


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, labels=(),
                        max_det=300, nc=0, max_time_img=0.05, max_nms=30000, max_wh=7680):
    """Batched NMS, same signature and return type as the reference (ops.py:136-266): list of (n_i, 6) tensors
    [x1, y1, x2, y2, conf, cls] on prediction.device.  One fused HIP launch for the whole batch + one D2H of the counts.

    With mask channels (nm = prediction rows - 4 - nc > 0, a Segment head's output) the rows are (n_i, 6 + nm): the kept anchors' mask
    coefficients behind the six detection columns (mgdt_nms_masks_fwd; the nm == 0 call is unchanged).  A Pose prediction is the same call with
    nm = nk decoded keypoint values.

    Differences, all documented in DESIGN.md: `max_time_img` is accepted and ignored (no wall-clock truncation);
    score ties are ordered by candidate index; `labels` (autolabelling a-priori boxes) are not on the hot path and raise.
    """
    assert 0 <= conf_thres <= 1, f'Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0'
    assert 0 <= iou_thres <= 1, f'Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0'
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    bs = prediction.shape[0]
    nc = nc or (prediction.shape[1] - 4)
    nm = prediction.shape[1] - nc - 4
    if nm < 0:
        raise RuntimeError(f'non_max_suppression: nc={nc} does not fit a prediction with {prediction.shape[1]} rows')
    if labels and any(len(l) for l in labels):
        raise RuntimeError('non_max_suppression: autolabelling `labels` are out of scope of the detection path')
    if classes is not None and len(classes) == 0:
        return [torch.zeros((0, 6 + nm), device=prediction.device)] * bs
    if nm:
        return nms_masks_batch(prediction, nm, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, max_nms, max_wh)[0]
    pred = prediction if (prediction.dtype == torch.float32 and prediction.is_contiguous()) else prediction.float().contiguous()
    out, _, counts = hip.nms(pred, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, max_nms, max_wh)
    counts = counts.tolist()   # the one host sync: result sizes
    return [out[i, :counts[i]] for i in range(bs)]


def nms_with_index(prediction, **kw):
    """Like non_max_suppression but also returns the kept anchor indices (int32) per image - used by the parity tests."""
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    kw.setdefault('conf_thres', 0.25); kw.setdefault('iou_thres', 0.45)
    out, kept, counts = hip.nms(prediction.float().contiguous(), kw['conf_thres'], kw['iou_thres'], kw.get('classes'), kw.get('agnostic', False),
                                kw.get('multi_label', False), kw.get('max_det', 300), kw.get('max_nms', 30000), kw.get('max_wh', 7680))
    counts = counts.tolist()
    return [out[i, :c] for i, c in enumerate(counts)], [kept[i, :c] for i, c in enumerate(counts)]


def nms_masks_batch(prediction, nm, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300, max_nms=30000,
                    max_wh=7680):
    """NMS on a Segment prediction (B, 4+nc+nm, A) -> (list of (n_i, 6+nm) rows, the padded (B, max_det, 6+nm) rows, counts on the device, counts
    on the host): the batch form `process_mask_batch` takes.  One launch, one host sync (the counts)."""
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    pred = prediction if (prediction.dtype == torch.float32 and prediction.is_contiguous()) else prediction.float().contiguous()
    rows, _, counts_dev = hip.nms_masks(pred, nm, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, max_nms, max_wh)
    counts = counts_dev.tolist()   # the one host sync: result sizes
    return [rows[i, :counts[i]] for i in range(pred.shape[0])], rows, counts_dev, counts


def crop_mask(masks, boxes):
    """Zero the (n, h, w) masks outside their xyxy `boxes` (n, 4) given in mask pixels: pixel (row y, column x) survives when x1 <= x < x2 and
    y1 <= y < y2 on float indices (ops.py:541-557).  A plain-tensor helper for callers that hold masks already; the mask routines below apply
    the same half-open test inside their kernel and never call it."""
    _, h, w = masks.shape
    b = boxes.to(masks.dtype if masks.is_floating_point() else torch.float32)[:, :, None, None]
    xs = torch.arange(w, device=masks.device, dtype=b.dtype)[None, None, :]
    ys = torch.arange(h, device=masks.device, dtype=b.dtype)[None, :, None]
    keep = (xs >= b[:, 0]) & (xs < b[:, 2]) & (ys >= b[:, 1]) & (ys < b[:, 3])
    return masks * keep


def _protos_nhwc(protos):
    """(nm, mh, mw) or (B, nm, mh, mw) protos -> the (B, nm, mh, mw) NHWC-backed tensor the kernel reads (a slice of the Proto output is one
    already; anything else is copied by the layout kernel)."""
    p = protos[None] if protos.dim() == 3 else protos
    if p.dim() != 4:
        raise RuntimeError(f'protos must be (nm, mh, mw) or (B, nm, mh, mw), got {tuple(protos.shape)}')
    if p.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f'protos are float32 or bfloat16, not {p.dtype}')
    hip._need_gpu(p)
    b, c, h, w = p.shape
    es = 8 if p.dtype == torch.bfloat16 else 4
    if hip.is_nhwc(p) and p.stride(3) == c and p.stride(2) == w * c and p.stride(0) % es == 0 and p.data_ptr() % 16 == 0:
        return p
    return hip.copy(p, hip.new_act(b, c, h, w, p.dtype, p.device))


def _one_image(protos, masks_in, bboxes, shape, mode, out_dtype):
    if protos.dim() != 3:
        raise RuntimeError(f'protos of one image are (nm, mh, mw), got {tuple(protos.shape)}')
    if masks_in.dim() != 2 or bboxes.dim() != 2 or masks_in.shape[0] != bboxes.shape[0] or bboxes.shape[1] != 4:
        raise RuntimeError(f'masks_in (n, nm) and bboxes (n, 4) expected, got {tuple(masks_in.shape)} and {tuple(bboxes.shape)}')
    if masks_in.shape[1] != protos.shape[0]:
        raise RuntimeError(f'masks_in has nm={masks_in.shape[1]} coefficients, the protos {protos.shape[0]} channels')
    p = _protos_nhwc(protos)
    n, nm = masks_in.shape
    rows = torch.zeros(1, max(n, 1), 6 + nm, dtype=torch.float32, device=p.device)
    if n:
        rows[0, :n, :4] = bboxes
        rows[0, :n, 6:] = masks_in
    counts_dev = torch.tensor([n], dtype=torch.int32).to(p.device)
    return hip.seg_masks(p, rows, counts_dev, [n], shape, mode, out_dtype)


def process_mask(protos, masks_in, bboxes, shape, upsample=False, out_dtype=torch.float32):
    """Masks of one image (ops.py:581-610): sigmoid(masks_in @ protos) cropped by the boxes scaled to proto resolution, optionally resampled to
    `shape` (the crop is applied BEFORE the resampling), > 0.5.  protos (nm, mh, mw), masks_in (n, nm), bboxes (n, 4) xyxy in `shape` pixels ->
    (n, mh, mw) or (n, *shape) 0 / 1 masks, float32 like the reference or uint8."""
    return _one_image(protos, masks_in, bboxes, shape, 'process_mask_up' if upsample else 'process_mask', out_dtype)


def process_mask_upsample(protos, masks_in, bboxes, shape, out_dtype=torch.float32):
    """ops.py:560-578: resample to `shape` first, crop with the unscaled boxes afterwards."""
    return _one_image(protos, masks_in, bboxes, shape, 'process_mask_upsample', out_dtype)


def process_mask_native(protos, masks_in, bboxes, shape, out_dtype=torch.float32):
    """ops.py:613-636: the letter-box window of the protos resampled to the original image `shape`, cropped with boxes in original pixels."""
    return _one_image(protos, masks_in, bboxes, shape, 'process_mask_native', out_dtype)


def process_mask_batch(protos, rows, counts, shape, mode='process_mask', out_dtype=torch.uint8, counts_host=None):
    """The masks of a whole batch in one launch: protos (B, nm, mh, mw) as the Segment head returns them, rows (B, max_det, 6+nm) + counts (B,)
    int32 on the device as `nms_masks_batch` returns them (counts_host: their host copy when the caller already has it - no second sync), mode one
    of 'process_mask', 'process_mask_up' (upsample=True), 'process_mask_upsample', 'process_mask_native' -> (sum(counts), H, W) masks, image
    after image."""
    if protos.dim() != 4 or rows.dim() != 3 or rows.shape[2] != 6 + protos.shape[1]:
        raise RuntimeError(f'process_mask_batch: protos (B, nm, mh, mw) and rows (B, max_det, 6+nm) expected, got {tuple(protos.shape)} and {tuple(rows.shape)}')
    p = _protos_nhwc(protos)
    if counts_host is None:
        counts_host = counts.tolist()
    return hip.seg_masks(p, rows, counts, counts_host, shape, mode, out_dtype)
