"""LetterBox (reference: yolo/data/augment.py:538-593) for the predictor: geometry on the host exactly as the reference computes it, pixels
on the device - resize (cv2.INTER_LINEAR rule for 8-bit images), 114 border, BGR->RGB and HWC->CHW in one kernel per image, written
straight into the batch tensor (yolo/engine/predictor.py:115-130).

ImagePool / TrainAugment: the detection training pipeline of the reference's v8_transforms (augment.py:762-790, stretch=False) - Mosaic(4) or
LetterBox, RandomPerspective without perspective, RandomHSV, the two RandomFlips, Format - for a whole batch.  The random draws are made on the host
in the reference's order (`sample`); the pixels and the labels are made on the device in two launches (`apply`, csrc/augment.hip)."""
import math
import random

import numpy as np
import torch

from ... import _lib as L
from ... import ops as hip


class LetterBox:
    """Resize image and padding for detection (same constructor as the reference)."""

    def __init__(self, new_shape=(640, 640), auto=False, scaleFill=False, scaleup=True, stride=32):
        self.new_shape = new_shape
        self.auto = auto
        self.scaleFill = scaleFill
        self.scaleup = scaleup
        self.stride = stride

    def geometry(self, shape):
        """Source (h, w) -> (out_h, out_w, resized_h, resized_w, top, left, ratio, (pad_w / 2, pad_h / 2)).  The rule is the reference's
        (augment.py:554-583) and its rounding is part of the contract (fixtures tests/golden/letterbox.npz): one scale for both axes unless
        scaleFill, resized side = round(side * scale), the leftover split in halves with the odd pixel going to the bottom / right edge
        (round(half - 0.1) before, round(half + 0.1) after)."""
        src_h, src_w = shape[0], shape[1]
        dst_h, dst_w = (self.new_shape, self.new_shape) if isinstance(self.new_shape, int) else self.new_shape[:2]
        scale = min(dst_h / src_h, dst_w / src_w)
        if not self.scaleup:
            scale = min(scale, 1.0)
        ratio = (scale, scale)
        res_w, res_h = int(round(src_w * scale)), int(round(src_h * scale))
        pad_w, pad_h = dst_w - res_w, dst_h - res_h
        if self.auto:                                  # minimal rectangle: pad only up to the next multiple of the stride
            pad_w, pad_h = np.mod(pad_w, self.stride), np.mod(pad_h, self.stride)
        elif self.scaleFill:                           # stretch to the target, no border
            pad_w, pad_h, res_w, res_h = 0.0, 0.0, dst_w, dst_h
            ratio = (dst_w / src_w, dst_h / src_h)
        half_w, half_h = pad_w / 2, pad_h / 2
        before = lambda half: int(round(half - 0.1))
        after = lambda half: int(round(half + 0.1))
        top, left = before(half_h), before(half_w)
        return res_h + top + after(half_h), res_w + left + after(half_w), res_h, res_w, top, left, ratio, (half_w, half_h)

    def __call__(self, labels=None, image=None, out=None):
        """image: uint8 (h, w, 3) BGR tensor on the device (or numpy array, copied once).  Returns the letter-boxed image as uint8 (3, H, W) RGB
        planes (written into `out` when given) - the reference's LetterBox followed by predictor.py:123-125."""
        if labels:
            raise RuntimeError('LetterBox: label transformation belongs to the training data pipeline (out of scope)')
        img = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image)).to('cuda:0')
        hip._need_gpu(img)
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or img.stride(2) != 1 or img.stride(1) != 3:
            raise RuntimeError('LetterBox: expected a uint8 (h, w, 3) image with packed pixels')
        oh, ow, nh, nw, top, left, _, _ = self.geometry(tuple(img.shape[:2]))
        if out is None:
            out = torch.empty(3, oh, ow, dtype=torch.uint8, device=img.device)
        elif tuple(out.shape) != (3, oh, ow) or not out.is_contiguous():
            raise RuntimeError(f'LetterBox: out must be a contiguous (3, {oh}, {ow}) uint8 tensor')
        L.check(L.lib().mgdt_letterbox_fwd(hip.ptr(img), img.shape[0], img.shape[1], img.stride(0), hip.ptr(out), oh, ow, nh, nw, top, left, hip.stream()), 'letterbox')
        return out


DEFAULT_HYP = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, flipud=0.0, fliplr=0.0,
                   mosaic=1.0, mixup=0.0, copy_paste=0.0)          # yolo/cfg/default.yaml:97-109 of this fork (fliplr is 0.0 here)


def rotation_matrix_2d(angle, scale, center=(0.0, 0.0)):
    """cv2.getRotationMatrix2D by its documented closed form (float64, 2 x 3): alpha = scale cos(angle), beta = scale sin(angle), angle in degrees."""
    a = angle * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = center
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)


class ImagePool:
    """A device-resident pool of training images: uint8 (h, w, 3) BGR arrays whose long side equals imgsz (what the reference's load_image hands
    to the transforms: no resize is left to do) and their labels (n, 5) [cls, x, y, w, h] normalised, uploaded once.  device=None keeps the pool on
    the host: enough for TrainAugment.sample.  `buffer` is the list Mosaic draws its three other images from (the reference's dataset.buffer)."""

    def __init__(self, images, labels, imgsz, device='cuda:0'):
        if len(images) != len(labels) or not len(images):
            raise ValueError(f'ImagePool: {len(images)} images, {len(labels)} label arrays')
        self.imgsz = int(imgsz)
        table = np.zeros(len(images), hip.AUG_IMAGE)
        flat, rows, off, start = [], [], 0, 0
        for i, (im, lb) in enumerate(zip(images, labels)):
            im = np.asarray(im)
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError(f'ImagePool: image {i} must be a uint8 (h, w, 3) BGR array, got {im.dtype} {im.shape}')
            if max(im.shape[:2]) != self.imgsz:
                raise ValueError(f'ImagePool: image {i} is {im.shape[0]} x {im.shape[1]}: its long side must equal imgsz = {self.imgsz} (pool images are not resized)')
            lb = np.asarray(lb, np.float32)
            lb = lb.reshape(0, 5) if lb.size == 0 else lb
            if lb.ndim != 2 or lb.shape[1] != 5:
                raise ValueError(f'ImagePool: labels of image {i} must be (n, 5) [cls, x, y, w, h] (boxes only: no segments, no keypoints), got {lb.shape}')
            table[i] = (off, im.shape[0], im.shape[1], start, len(lb))
            flat.append(np.ascontiguousarray(im).reshape(-1))
            rows.append(lb)
            off += im.shape[0] * im.shape[1] * 3
            start += len(lb)
        self.table, self.pool_bytes, self.n_labels = table, off, start
        self.buffer = list(range(len(images)))
        self.device = None if device is None else torch.device(device)
        if self.device is not None:
            if self.device.type != 'cuda':
                raise RuntimeError('mgdt_yolo_amd runs on MI355X (HIP) only: the image pool lives on the device and there is no CPU/PyTorch fallback')
            self.pixels = torch.from_numpy(np.concatenate(flat)).to(self.device)
            self.labels = torch.from_numpy(np.concatenate(rows).reshape(-1, 5) if start else np.zeros((1, 5), np.float32)).to(self.device)
            self.table_dev = torch.from_numpy(table.view(np.uint8).copy()).to(self.device)

    def __len__(self):
        return len(self.table)


class AugParams:
    """What `sample` drew for a batch: `records` (hip.AUG_RECORD, one per output image) and `luts` (B, 3, 256) uint8 are what the kernels read; the
    rest is the same in readable form: mosaic (B,) bool, indices (B, 4) (-1 past a letter-boxed image), yc / xc (B,), M (B, 3, 3) float32,
    scale (B,) float64, flipud / fliplr (B,) bool."""

    def __init__(self, b):
        self.records = np.zeros(b, hip.AUG_RECORD)
        self.luts = np.zeros((b, 3, 256), np.uint8)
        self.mosaic, self.flipud, self.fliplr = np.zeros(b, bool), np.zeros(b, bool), np.zeros(b, bool)
        self.indices = np.full((b, 4), -1, np.int64)
        self.yc, self.xc = np.zeros(b, np.int64), np.zeros(b, np.int64)
        self.M = np.zeros((b, 3, 3), np.float32)
        self.scale = np.zeros(b, np.float64)

    def __len__(self):
        return len(self.records)


def mosaic4_rects(s, yc, xc, shapes):
    """Placement of Mosaic._mosaic4 (augment.py:154-188) for four images of the given (h, w): image 0 lies with its lower right corner on the centre
    (xc, yc) of the 2s x 2s canvas, image 1 with its lower left, image 2 with its upper right, image 3 with its upper left one; whatever falls
    outside the canvas is cut off.  -> per image (x1, y1, x2, y2 on the canvas, x, y of the first source pixel shown)."""
    out = []
    for k, (h, w) in enumerate(shapes):
        ox, oy = (xc if k & 1 else xc - w), (yc if k & 2 else yc - h)           # where the image's own (0, 0) falls on the canvas
        x1, y1, x2, y2 = max(ox, 0), max(oy, 0), min(ox + w, 2 * s), min(oy + h, 2 * s)
        out.append((x1, y1, x2, y2, x1 - ox, y1 - oy))
    return out


def fill_record(rec, rects, pads, canvas, M, scale, flipud, fliplr, mosaic, lut):
    """One hip.AUG_RECORD from placement rectangles [(src, dx1, dy1, dx2, dy2, sx1, sy1)], label pads [(x, y)], the float32 3 x 3 matrix M and s.
    The inverse is taken in float64 and stored as six float32 words."""
    rec['nrect'], rec['canvas'], rec['lut'] = len(rects), canvas, lut
    rec['flags'] = int(bool(flipud)) | int(bool(fliplr)) << 1 | int(bool(mosaic)) << 2
    for k, (r, p) in enumerate(zip(rects, pads)):
        rec['rect'][k] = r
        rec['pad'][k] = p
    rec['inv'] = np.linalg.inv(np.asarray(M, np.float64))[:2].astype(np.float32).reshape(-1)
    rec['m'] = np.asarray(M, np.float32)[:2].reshape(-1)
    rec['scale'] = np.float32(scale)


class TrainAugment:
    """v8_transforms(dataset, imgsz, hyp) + Format(bbox_format='xywh', normalize=True) of the reference for detection, on an ImagePool.

    sample(indices) -> AugParams on the host: Python's `random` and `numpy.random` are consumed in the reference's order (the draws of transforms
                       whose probability is 0 included), so equal seeds, pool and indices give the reference's parameters.  Needs no GPU.
    apply(params)   -> {'img' (B, 3, S, S) uint8 RGB, dense NCHW planes (the stem's uint8 loader walks a plane row by row: unit stride along x
                       is what it reads fastest), 'gt' (B, N, 5) [cls, x1, y1, x2, y2] px, 'labels' (B, N, 5) [cls, x, y, w, h] normalised,
                       'nlabels' (B,) int32, 'flags' (B,) int32} on the device: one copy of the records and tables from pinned host memory into a
                       static device buffer, then two launches.  No host read, so it can be captured; `load(params)` then puts new records where
                       a replay's copy reads them.
    to_dict(batch)  -> the reference's wire format ('img', 'batch_idx', 'cls', 'bboxes') with one host read; raises when a flag is set.
    Not built (each raises when asked for): mixup, copy_paste, perspective, mosaic9, segments / keypoints, Albumentations."""

    def __init__(self, pool, hyp=None, imgsz=None, max_labels=None):
        h = dict(DEFAULT_HYP)
        if hyp is not None:
            h.update(hyp if isinstance(hyp, dict) else {k: v for k, v in vars(hyp).items()})
        for k in ('mixup', 'copy_paste'):
            if h.get(k):
                raise NotImplementedError(f'TrainAugment: {k}={h[k]} is not built (only {k}=0.0)')
        if h.get('perspective'):
            raise NotImplementedError(f"TrainAugment: perspective={h['perspective']} is not built (affine warps only)")
        if h.get('mosaic_n', 4) != 4:
            raise NotImplementedError(f"TrainAugment: a mosaic of {h['mosaic_n']} images is not built (mosaic9), only 4")
        for k in ('segments', 'keypoints', 'use_segments', 'use_keypoints', 'albumentations'):
            if h.get(k):
                raise NotImplementedError(f'TrainAugment: {k} is not built (detection boxes only, no Albumentations)')
        for k in ('mosaic', 'flipud', 'fliplr'):
            if not 0 <= h[k] <= 1.0:
                raise ValueError(f'TrainAugment: {k}={h[k]} must be a probability')
        self.hyp, self.pool = h, pool
        self.imgsz = int(pool.imgsz if imgsz is None else imgsz)
        if self.imgsz != pool.imgsz:
            raise ValueError(f'TrainAugment: imgsz={self.imgsz} but the pool holds images of long side {pool.imgsz} (pool images are not resized)')
        if self.imgsz % 4:
            raise ValueError(f'TrainAugment: imgsz={self.imgsz} must be a multiple of 4')
        if max_labels is None:
            max_labels = 4 * int(pool.table['label_count'].max())
        self.max_labels = max(16, -(-int(max_labels) // 16) * 16)
        self._dev = self._host = self._copied = None

    # ---- host: the draws ------------------------------------------------------------------------------------------------------------
    def _affine(self, canvas_w, canvas_h, size):
        """M = T @ S @ R @ P @ C of RandomPerspective.affine_transform (augment.py:308-346) and its scale: the eight draws in the reference's order,
        every factor a float32 3 x 3 matrix, the product taken left to right in float32 numpy as the reference takes it."""
        h = self.hyp
        draw = lambda lo, hi: random.uniform(lo, hi)
        px, py = draw(-h['perspective'], h['perspective']), draw(-h['perspective'], h['perspective'])
        angle, scale = draw(-h['degrees'], h['degrees']), draw(1 - h['scale'], 1 + h['scale'])
        shx, shy = draw(-h['shear'], h['shear']), draw(-h['shear'], h['shear'])
        tx, ty = draw(0.5 - h['translate'], 0.5 + h['translate']), draw(0.5 - h['translate'], 0.5 + h['translate'])

        def m3(entries):
            m = np.eye(3, dtype=np.float32)
            for (i, j), v in entries.items():
                m[i, j] = v
            return m
        centre = m3({(0, 2): -canvas_w / 2, (1, 2): -canvas_h / 2})
        persp = m3({(2, 0): px, (2, 1): py})
        rot = m3({})
        rot[:2] = rotation_matrix_2d(angle, scale)
        shear = m3({(0, 1): math.tan(shx * math.pi / 180), (1, 0): math.tan(shy * math.pi / 180)})
        shift = m3({(0, 2): tx * size[0], (1, 2): ty * size[1]})
        return shift @ shear @ rot @ persp @ centre, scale

    def sample(self, indices):
        h, s, tab = self.hyp, self.imgsz, self.pool.table
        indices = [int(i) for i in indices]
        if any(not 0 <= i < len(tab) for i in indices):
            raise ValueError(f'TrainAugment.sample: indices must lie in 0..{len(tab) - 1}')
        P = AugParams(len(indices))
        shape = lambda i: (int(tab['h'][i]), int(tab['w'][i]))
        for b, index in enumerate(indices):
            if random.uniform(0, 1) > h['mosaic']:                                  # BaseMixTransform.__call__ of Mosaic (augment.py:87)
                lb = LetterBox(new_shape=(s, s))                                    # RandomPerspective's pre_transform (:428-430)
                hh, ww = shape(index)
                _, _, _, _, top, left, _, (dw, dh) = lb.geometry((hh, ww))
                rects, pads = [(index, left, top, left + ww, top + hh, 0, 0)], [(dw, dh)]
                canvas, border = s, (0, 0)
                P.indices[b, 0] = index
            else:
                idx = [index] + random.choices(list(self.pool.buffer), k=3)         # Mosaic.get_indexes (:141-144)
                border = (-s // 2, -s // 2)
                yc, xc = (int(random.uniform(-x, 2 * s + x)) for x in border)       # :158
                quads = mosaic4_rects(s, yc, xc, [shape(i) for i in idx])
                rects = [(i,) + q for i, q in zip(idx, quads)]
                pads = [(q[0] - q[4], q[1] - q[5]) for q in quads]          # where each image's own (0, 0) falls: what its boxes move by
                canvas = 2 * s
                P.mosaic[b], P.indices[b], P.yc[b], P.xc[b] = True, idx, yc, xc
            size = (canvas + border[1] * 2, canvas + border[0] * 2)               # (w, h) of the warp's output (:440)
            if size != (s, s):
                raise ValueError(f'TrainAugment: imgsz={s} gives a warp output of {size}')
            M, sc = self._affine(canvas, canvas, size)
            random.uniform(0, 1)                                                    # BaseMixTransform.__call__ of MixUp, p = 0
            lut = -1
            if h['hsv_h'] or h['hsv_s'] or h['hsv_v']:                              # RandomHSV (:489-497)
                r = np.random.uniform(-1, 1, 3) * [h['hsv_h'], h['hsv_s'], h['hsv_v']] + 1
                x = np.arange(0, 256, dtype=r.dtype)
                P.luts[b, 0] = ((x * r[0]) % 180).astype(np.uint8)
                P.luts[b, 1] = np.clip(x * r[1], 0, 255).astype(np.uint8)
                P.luts[b, 2] = np.clip(x * r[2], 0, 255).astype(np.uint8)
                lut = b * 768
            P.flipud[b] = random.random() < h['flipud']                             # RandomFlip('vertical') then ('horizontal') (:524-527)
            P.fliplr[b] = random.random() < h['fliplr']
            P.M[b], P.scale[b] = M, sc
            fill_record(P.records[b], rects, pads, canvas, M, sc, P.flipud[b], P.fliplr[b], P.mosaic[b], lut)
        return P

    # ---- device ---------------------------------------------------------------------------------------------------------------------
    def _buffers(self, b):
        n = b * (hip.AUG_RECORD.itemsize + 768)
        if self._dev is None or self._dev.numel() != n:
            if self.pool.device is None:
                raise RuntimeError('TrainAugment.apply: the pool was built with device=None (host only)')
            self._dev = torch.zeros(n, dtype=torch.uint8, device=self.pool.device)
            self._host = torch.zeros(n, dtype=torch.uint8).pin_memory()
            self._copied = None
        return self._dev, self._host

    def load(self, params):
        """Check the records against the pool (mgdt_aug_check) and put them, with the LUTs, into the pinned host buffer that `apply`'s copy reads."""
        b = len(params)
        dev, host = self._buffers(b)
        hip.aug_check(params.records, self.pool.table, self.pool.pool_bytes, self.pool.n_labels, b * 768, self.imgsz)
        if self._copied is not None and not torch.cuda.is_current_stream_capturing():
            self._copied.synchronize()                  # an earlier eager copy may still be reading the buffer (host-side wait, no device read)
        rb = b * hip.AUG_RECORD.itemsize
        host[:rb].numpy()[:] = params.records.view(np.uint8).reshape(-1)
        host[rb:].numpy()[:] = params.luts.reshape(-1)
        return b, rb

    def apply(self, params):
        b, rb = self.load(params)
        dev, host, p, s = self._dev, self._host, self.pool, self.imgsz
        dev.copy_(host, non_blocking=True)
        if not torch.cuda.is_current_stream_capturing():
            self._copied = torch.cuda.Event()
            self._copied.record()
        img = hip.aug_warp(p.pixels, p.table_dev, p.table, dev[:rb], params.records, dev[rb:], b, s)
        gt, labels, nlabels, flags = hip.aug_labels(p.labels, p.n_labels, p.table_dev, p.table, dev[:rb], params.records, b, s, self.max_labels)
        return {'img': img, 'gt': gt, 'labels': labels, 'nlabels': nlabels, 'flags': flags}

    def __call__(self, indices):
        return self.apply(self.sample(indices))

    @staticmethod
    def to_dict(batch):
        """The device batch as the reference's collated dict: img stays where it is; batch_idx (n,), cls (n, 1), bboxes (n, 4) on the host."""
        b, n = batch['labels'].shape[:2]
        flat = torch.cat([batch['flags'].float(), batch['nlabels'].float(), batch['labels'].reshape(-1)]).cpu().numpy()      # the one host read
        flags, counts, rows = flat[:b].astype(np.int64), flat[b:2 * b].astype(np.int64), flat[2 * b:].reshape(b, n, 5)
        if flags.any():
            raise RuntimeError(f'TrainAugment.to_dict: images {np.nonzero(flags)[0].tolist()} have more than {n} boxes (raise max_labels)')
        idx = np.concatenate([np.full(c, i, np.float32) for i, c in enumerate(counts)]) if b else np.zeros(0, np.float32)
        kept = np.concatenate([rows[i, :c] for i, c in enumerate(counts)]).reshape(-1, 5)
        return {'img': batch['img'], 'batch_idx': torch.from_numpy(idx), 'cls': torch.from_numpy(kept[:, :1].copy()),
                'bboxes': torch.from_numpy(kept[:, 1:].copy())}
