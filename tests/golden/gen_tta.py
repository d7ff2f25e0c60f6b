"""Generate tests/golden/tta.npz: test-time augmentation fixtures from the reference's own Python modules (BUILD CONTAINER ONLY).

    python tests/golden/gen_tta.py

Same recipe as gen_golden.py (ref_import, seeded weights and images, CPU fp32).  Records
  - `scale_img` (yolo/utils/torch_utils.py:261-270) on fp32 and uint8-derived inputs, with and without the left-right flip;
  - `DetectionModel._predict_augment` (nn/tasks.py:256-287) of yolov8 n and mspa_c2f_gd_yolov8 n, with the per-pass geometry
    (pass sizes, per-level anchor counts, the anchor range each pass keeps after `_clip_augmented`);
  - NMS kept rows on the augmented output at the predictor's and the validator's settings (oracle NMS standing in for torchvision).
The GPU box never runs this file.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_import  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images  # noqa: E402
from oracle import nms as onms  # noqa: E402  (only to stand in for the absent torchvision.ops.nms)
from inputs import E2E_MODELS, IMG_SEED  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()
REFY = '/root/reference/models/v8/'

# (name, (b, h, w), ratio, flip, gs, uint8 input)
SCALE_CASES = [
    ('f32_083_g32', (1, 40, 72), 0.83, False, 32, False),
    ('f32_083_g32_flip', (1, 40, 72), 0.83, True, 32, False),
    ('f32_067_g8_odd', (1, 37, 53), 0.67, False, 8, False),
    ('f32_083_g8_odd_flip', (1, 37, 53), 0.83, True, 8, False),
    ('f32_067_g32_flip', (1, 72, 120), 0.67, True, 32, False),
    ('u8_083_g8_flip', (2, 45, 31), 0.83, True, 8, True),
    ('u8_067_g32', (1, 64, 80), 0.67, False, 32, True),
]
# shapes whose augmented outputs are recorded, every SUB-th anchor (the committed file stays small)
TTA_SHAPES = {(2, 160, 224): 10, (1, 192, 160): 5, (1, 640, 480): 50}
# the shape whose whole augmented output is recorded with its NMS kept rows
NMS_SHAPE = (1, 128, 96)
# shapes whose geometry alone is recorded (the table of the feature's issue)
GEOM_SHAPES = [(1, 640, 640), (1, 640, 480), (1, 160, 224), (2, 160, 224), (1, 192, 160), (1, 128, 96)]
NMS_TTA_CASES = (('pred', dict(conf_thres=0.25, iou_thres=0.7)), ('val', dict(conf_thres=0.001, iou_thres=0.7, multi_label=True)))


def save(name, **arrs):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print(f'{name}: {os.path.getsize(path) / 1024:.1f} KiB')


def build(yaml_name, nc=80, seed=0):
    m = ns.tasks.DetectionModel(REFY + yaml_name, nc=nc, verbose=False)
    seed_state_dict_(m, seed)
    m.args = types.SimpleNamespace(box=7.5, cls=0.5, dfl=1.5)
    return m.eval()


def u8_image(b, h, w, seed):
    r = np.random.default_rng([seed, 777])
    return r.integers(0, 256, (b, 3, h, w), dtype=np.uint8)


def scale_cases(arrs):
    for i, (name, (b, h, w), ratio, flip, gs, u8) in enumerate(SCALE_CASES):
        if u8:
            xu = u8_image(b, h, w, 100 + i)
            arrs[f'scale_{name}_u8'] = xu
            x = torch.from_numpy(xu).float() / 255
        else:
            x = seeded_images(b, h, w, seed=100 + i)            # re-created from the seed by the test
        out = ns.torch_utils.scale_img(x.flip(3) if flip else x, ratio, gs=gs)
        arrs[f'scale_{name}_y'] = out.numpy()
        arrs[f'scale_{name}_p'] = np.array([ratio, float(flip), gs], np.float64)
        print('scale_img', name, tuple(x.shape), '->', tuple(out.shape))


def geometry(m, x):
    """The reference's three passes, step by step: pass sizes, per-level anchor counts and the kept anchor range of each pass."""
    img_size = x.shape[-2:]
    gs = int(m.stride.max())
    sizes, levels, ys = [], [], []
    for si, fi in zip([1, 0.83, 0.67], [None, 3, None]):
        xi = ns.torch_utils.scale_img(x.flip(fi) if fi else x, si, gs=gs)
        yi, feats = ns.tasks.BaseModel.predict(m, xi)
        sizes.append(list(xi.shape[-2:]))
        levels.append([int(f.shape[2] * f.shape[3]) for f in feats])
        ys.append(m._descale_pred(yi, fi, si, img_size))
    full = [int(y.shape[-1]) for y in ys]
    clipped = m._clip_augmented(list(ys))
    keep = [(0, int(clipped[0].shape[-1])), (0, int(clipped[1].shape[-1])), (full[2] - int(clipped[2].shape[-1]), full[2])]
    return np.array(sizes, np.int64), np.array(levels, np.int64), np.array(keep, np.int64), torch.cat(clipped, -1)


def tta(arrs, tag, yaml_name):
    m = build(yaml_name)
    arrs[f'{tag}_stride'] = m.stride.numpy()
    for (b, h, w) in sorted(set(GEOM_SHAPES) | set(TTA_SHAPES) | {NMS_SHAPE}):
        key = f'{tag}_{b}x{h}x{w}'
        x = seeded_images(b, h, w, seed=IMG_SEED)
        with torch.no_grad():
            sizes, levels, keep, ystep = geometry(m, x)
            y, none = m._predict_augment(x)
        assert none is None and torch.equal(y, ystep)
        arrs[f'{key}_sizes'], arrs[f'{key}_levels'], arrs[f'{key}_keep'] = sizes, levels, keep
        arrs[f'{key}_anchors'] = np.array(y.shape[-1], np.int64)
        if (b, h, w) in TTA_SHAPES:
            arrs[f'{key}_ysub'] = y[:, :, ::TTA_SHAPES[(b, h, w)]].numpy()
        if (b, h, w) == NMS_SHAPE:
            arrs[f'{key}_y'] = y.numpy()
            for cname, kw in NMS_TTA_CASES:
                out = ns.ops.non_max_suppression((y.clone(), None), max_time_img=1e9, **kw)       # the (y, None) tuple as the model returns it
                for i, o in enumerate(out):
                    arrs[f'{key}_nms_{cname}_{i}'] = o.numpy()
                print('nms', key, cname, [int(o.shape[0]) for o in out])
        print('tta', key, sizes.tolist(), 'anchors', int(y.shape[-1]), 'keep', keep.tolist())


def main():
    import torchvision  # the stand-in module from ref_import

    def nms_standin(boxes, scores, thr):
        assert bool((scores[:-1] >= scores[1:]).all()), 'reference hands nms() descending scores'
        return torch.from_numpy(onms.greedy_nms(boxes.numpy(), thr))

    torchvision.ops.nms = nms_standin
    arrs = {}
    scale_cases(arrs)
    for tag, yname in E2E_MODELS.items():
        tta(arrs, tag, yname + '.yaml')
    save('tta', **arrs)


if __name__ == '__main__':
    main()
