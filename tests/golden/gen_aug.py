"""Generate tests/golden/aug_NN.npz from the reference's own v8_transforms + Format (build container only; cv2 is not installed).

The reference's yolo/data/augment.py runs as it is.  What it asks of cv2 is stood in for WITHOUT emulating any pixel arithmetic:
  getRotationMatrix2D  its documented closed form;
  warpAffine           records its input (the mosaic / letter-box canvas), M and dsize, returns a 114 image of dsize;
  cvtColor, split, merge, LUT   pass the image through; LUT records the table;
  copyMakeBorder       constant border (LetterBox places the image with it); resize must not be called (pool images have their final size).
The `random` module the reference sees is a logging proxy, so Mosaic's indices and centre and the flip draws are recorded as drawn.

Run:  python tests/golden/gen_aug.py          (asserts that every case ends on the seed of tests/aug_ref.py CASES)
      python tests/golden/gen_aug.py --find   (prints the seeds instead)
"""
import importlib
import json
import math
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import aug_ref as AR  # noqa: E402
import ref_import  # noqa: E402

DEFAULT_HYP = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, flipud=0.0, fliplr=0.0,
                   mosaic=1.0, mixup=0.0, copy_paste=0.0)
REC = {}


class RandomLog:
    """`random` as the reference's module sees it: the real generator, every draw logged."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        fn = getattr(random, name)

        def call(*a, **k):
            v = fn(*a, **k)
            self.log.append((name, v))
            return v
        return call


def install():
    ref_import.install()
    m = types.ModuleType('ultralytics.yolo.data')                # shell package: its __init__ pulls in the dataset classes
    m.__path__ = [os.path.join(ref_import.REF, 'yolo', 'data')]
    sys.modules['ultralytics.yolo.data'] = m
    import cv2
    cv2.BORDER_CONSTANT, cv2.INTER_LINEAR, cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = 0, 1, 40, 54

    def rot(angle, center, scale):
        a = angle * math.pi / 180
        al, be = math.cos(a) * scale, math.sin(a) * scale
        cx, cy = center
        return np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]], np.float64)

    def warp_affine(img, M, dsize, borderValue=None):
        REC['canvas'], REC['M2'], REC['dsize'] = img.copy(), np.array(M), tuple(dsize)
        return np.full((dsize[1], dsize[0], 3), 114, np.uint8)

    def lut(ch, table):
        REC.setdefault('luts', []).append(np.array(table))
        return ch

    def border(img, top, bottom, left, right, kind, value=None):
        out = np.full((img.shape[0] + top + bottom, img.shape[1] + left + right, 3), value[0], np.uint8)
        out[top:top + img.shape[0], left:left + img.shape[1]] = img
        return out

    def no_resize(*a, **k):
        raise AssertionError('cv2.resize must not be reached: pool images have their final size')

    cv2.getRotationMatrix2D, cv2.warpAffine, cv2.LUT, cv2.copyMakeBorder, cv2.resize = rot, warp_affine, lut, border, no_resize
    cv2.cvtColor = lambda img, code, dst=None: img
    cv2.split = lambda img: (img[..., 0], img[..., 1], img[..., 2])
    cv2.merge = lambda chans: np.stack(chans, -1)
    aug = importlib.import_module('ultralytics.yolo.data.augment')
    inst = importlib.import_module('ultralytics.yolo.utils.instance')
    return aug, inst


class Dataset:
    use_keypoints = False
    data = {}

    def __init__(self, inst, images, labels):
        self.inst, self.images, self.labels = inst, images, labels
        self.buffer = list(range(len(images)))

    def __len__(self):
        return len(self.images)

    def get_image_and_label(self, i):
        im = self.images[i].copy()
        l = self.labels[i]
        return dict(img=im, im_file=f'{i}.jpg', ori_shape=im.shape[:2], resized_shape=im.shape[:2], ratio_pad=(1.0, 1.0), cls=l[:, :1].copy(),
                    instances=self.inst.Instances(l[:, 1:].copy(), segments=[], keypoints=None, bbox_format='xywh', normalized=True))


def run_case(aug, inst, case, seed):
    S = case['S']
    hyp = types.SimpleNamespace(**dict(DEFAULT_HYP, **case['hyp']))
    images, labels = AR.make_pool(S)
    shapes = [im.shape[:2] for im in images]
    ds = Dataset(inst, images, labels)
    tf = aug.Compose([aug.v8_transforms(ds, S, hyp), aug.Format(bbox_format='xywh', normalize=True, return_mask=False, return_keypoint=False, batch_idx=True)])
    random.seed(seed)
    np.random.seed(seed)
    log = aug.random = RandomLog()
    B = len(AR.INDICES)
    d = dict(seed=np.int64(seed), S=np.int64(S), indices=np.array(AR.INDICES), mosaic=np.zeros(B, bool), mix=np.full((B, 4), -1, np.int64),
             yc=np.zeros(B, np.int64), xc=np.zeros(B, np.int64), M=np.zeros((B, 3, 3), np.float32), s=np.zeros(B), luts=np.zeros((B, 3, 256), np.uint8),
             flipud=np.zeros(B, bool), fliplr=np.zeros(B, bool), n=np.zeros(B, np.int64), hyp=np.array(json.dumps(vars(hyp), sort_keys=True)))
    canv, cls, box, margin = [], [], [], np.inf
    try:
        for b, i in enumerate(AR.INDICES):
            REC.clear()
            del log.log[:]
            out = tf(ds.get_image_and_label(i))
            draws = list(log.log)
            assert tuple(out['img'].shape) == (3, S, S) and REC['dsize'] == (S, S)
            mosaic = draws[1][0] == 'choices'
            d['mosaic'][b] = mosaic
            if mosaic:
                d['mix'][b] = [i] + list(draws[1][1])
                d['yc'][b], d['xc'][b] = int(draws[2][1]), int(draws[3][1])
                draws = draws[4:]
            else:
                d['mix'][b, 0] = i
                draws = draws[1:]
            # two perspective draws, angle, scale, two shears, two translations, MixUp's uniform, the two flips
            assert [n for n, _ in draws] == ['uniform'] * 9 + ['random'] * 2, draws
            d['s'][b] = draws[3][1]
            d['flipud'][b], d['fliplr'][b] = draws[9][1] < hyp.flipud, draws[10][1] < hyp.fliplr
            M = np.eye(3, dtype=np.float32)
            M[:2] = REC['M2']
            assert REC['M2'].dtype == np.float32
            d['M'][b] = M
            d['luts'][b] = np.stack(REC['luts'])
            canv.append(REC['canvas'])
            nb = len(out['cls'])
            d['n'][b] = nb
            cls.append(out['cls'].numpy().reshape(-1).astype(np.float32))
            box.append(out['bboxes'].numpy().reshape(-1, 4).astype(np.float32))
            assert out['bboxes'].dtype.is_floating_point and (nb == 0 or out['bboxes'].numpy().dtype == np.float32)
            # the restatement on the recorded parameters: how far every keep/drop quantity is from its threshold
            if mosaic:
                rects, pads = AR.mosaic_rects(S, int(d['yc'][b]), int(d['xc'][b]), d['mix'][b].tolist(), [shapes[j] for j in d['mix'][b]])
            else:
                rects, pads = AR.letterbox_rect(S, i, shapes[i])
            r = AR.boxes(labels, shapes, rects, pads, canv[-1].shape[0], M, d['s'][b], S, mosaic, d['flipud'][b], d['fliplr'][b])
            margin = min(margin, r['margin'])
            if int(r['keep'].sum()) != nb:
                margin = 0.0
        d['next_random'] = np.float64(random.random())
    finally:
        aug.random = random
    nmax = max(1, int(d['n'].max()))
    d['cls'], d['bboxes'] = np.zeros((B, nmax), np.float32), np.zeros((B, nmax, 4), np.float32)
    for b in range(B):
        d['cls'][b, :d['n'][b]], d['bboxes'][b, :d['n'][b]] = cls[b], box[b]
    d['canvas'] = np.stack(canv)
    rot = bool(case['hyp'].get('flipud'))
    covered = d['n'].sum() > 0 and (not rot or (d['flipud'].any() and d['fliplr'].any() and not d['flipud'].all() and not d['fliplr'].all()))
    return d, margin, covered


def main(find):
    aug, inst = install()
    for case in AR.CASES:
        for seed in range(case['start'], case['start'] + 200):
            d, margin, covered = run_case(aug, inst, case, seed)
            if margin >= AR.MARGIN and covered:
                break
            print(f"{case['name']}: seed {seed}: margin {margin:.2e}, covered {covered} - next seed")
        else:
            raise SystemExit(f"{case['name']}: no seed passed")
        if not find:
            assert seed == case['seed'], f"{case['name']}: ended on seed {seed}, the case table says {case['seed']}"
        path = os.path.join(HERE, case['name'] + '.npz')
        np.savez_compressed(path, **d)
        print(f"{path}: seed {seed}, margin {margin:.2e}, boxes {d['n'].tolist()}, mosaic {d['mosaic'].tolist()}, flipud {d['flipud'].tolist()}, "
              f"fliplr {d['fliplr'].tolist()}, {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main('--find' in sys.argv)
