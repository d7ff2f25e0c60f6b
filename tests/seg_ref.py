"""Restatement of the reference's mask routines (yolo/utils/ops.py:541-636) in float64, for the undecided band of the mask tests.

`mask_values(protos, masks_in, bboxes, shape, mode)` returns the PRE-THRESHOLD values of the routine `mode` (what the reference compares with 0.5)
with every product, sum, sigmoid and interpolation weight evaluated in float64 on the inputs as given (so bf16-rounded inputs give the exact
target of the bf16 kernel).  The crop tests are NOT restated in float64: they are the reference's float32 comparisons, bit for bit (the box
scaled by the Python double `mw / iw` rounded into the float32 tensor), because a crop edge is a decision, not a rounding error.
Used by tests/golden/gen_seg.py (to record which pixels lie within 1e-3 of the threshold) and by tests/test_segment.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

MODES = ('process_mask', 'process_mask_up', 'process_mask_upsample', 'process_mask_native')
BAND = 1e-3


def crop_keep(boxes, h, w):
    """(n, h, w) bool: pixel (y, x) is kept when x1 <= x < x2 and y1 <= y < y2, compared in float32 as the reference does (ops.py:552-557)."""
    b = boxes.float()[:, :, None, None]
    xs = torch.arange(w, dtype=torch.float32)[None, None, :]
    ys = torch.arange(h, dtype=torch.float32)[None, :, None]
    return (xs >= b[:, 0]) & (xs < b[:, 2]) & (ys >= b[:, 1]) & (ys < b[:, 3])


def native_window(mh, mw, shape):
    gain = min(mh / shape[0], mw / shape[1])
    pad = (mw - shape[1] * gain) / 2, (mh - shape[0] * gain) / 2
    top, left = int(pad[1]), int(pad[0])
    bottom, right = int(mh - pad[1]), int(mw - pad[0])
    return top, bottom, left, right


def mask_values(protos, masks_in, bboxes, shape, mode):
    """protos (nm, mh, mw), masks_in (n, nm), bboxes (n, 4) float32 CPU tensors -> (n, H, W) float64 pre-threshold values."""
    assert mode in MODES
    c, mh, mw = protos.shape
    ih, iw = shape
    m = (masks_in.double() @ protos.double().reshape(c, -1)).sigmoid().view(-1, mh, mw)
    if mode in ('process_mask', 'process_mask_up'):
        d = bboxes.clone().float()
        d[:, 0] *= mw / iw
        d[:, 2] *= mw / iw
        d[:, 3] *= mh / ih
        d[:, 1] *= mh / ih
        m = m * crop_keep(d, mh, mw)
        if mode == 'process_mask_up':
            m = F.interpolate(m[None], shape, mode='bilinear', align_corners=False)[0]
        return m
    if mode == 'process_mask_native':
        top, bottom, left, right = native_window(mh, mw, shape)
        m = m[:, top:bottom, left:right]
    m = F.interpolate(m[None], shape, mode='bilinear', align_corners=False)[0]
    return m * crop_keep(bboxes, shape[0], shape[1])


def undecided(values):
    """bool mask of the pixels whose float64 value lies within BAND of the 0.5 threshold."""
    return (values - 0.5).abs() <= BAND


def pack(mask_bool):
    return np.packbits(np.asarray(mask_bool, dtype=bool).reshape(-1))


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape).astype(bool)


def bf16_round(t):
    return t.to(torch.bfloat16).float()


def load_fixture():
    """All arrays of tests/golden/seg_NN.npz (tests/golden/gen_seg.py spreads them over several files) as one dict-like."""
    import glob
    import os
    out = {}
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'seg_[0-9][0-9].npz'))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    assert out, 'tests/golden/seg_NN.npz are missing'
    return out


def lb_images(shape=(134, 224)):
    """The two seeded BGR uint8 images of the predictor case (re-created, not stored)."""
    r = np.random.default_rng([41, 9])
    return [r.integers(0, 256, (*shape, 3), dtype=np.uint8) for _ in range(2)]
