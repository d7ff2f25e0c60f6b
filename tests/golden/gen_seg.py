"""Generate tests/golden/seg_NN.npz: instance-segmentation fixtures from the reference's own Python modules (BUILD CONTAINER ONLY).

    python tests/golden/gen_seg.py

Same recipe as gen_tta.py (ref_import, seeded weights and images, CPU fp32, the oracle's greedy NMS standing in for torchvision).  The arrays
are spread over several files (tests/seg_ref.py:load_fixture merges them) so that each stays under 1 MiB.  Recorded:
  - nn.ConvTranspose2d(c, c, 2, 2, 0) alone (1x16x9x13, 1x64x20x28: the 2-image form of the latter would be 1.1 MiB by itself) and `Proto`
    alone (1x16x9x13, 2x64x20x28) (nn/modules/block.py:57-69), inputs re-created from seeds;
  - SegmentationModel('yolov8-seg') and the MSPA-GD graph with its Detect row replaced by Segment [nc, 32, 256] (written to a temporary YAML and
    parsed by the reference), scale n, nc = 80: state-dict keys / shapes, parameter count, stride; cat(y, mc) and the protos IN FULL at 2x160x224
    and 1x192x160, every 25th anchor and every 4th proto pixel at 1x640x640;
  - for yolov8-seg at 2x160x224: NMS rows (n, 38) at the predictor's and the validator's settings, with a class filter, class-agnostic, and one
    setting that leaves an image with fewer detections than max_det; for the predictor-settings rows the masks of process_mask (both `upsample`
    values), process_mask_upsample and process_mask_native (two letter-boxed original shapes), bit-packed, each with the bit-packed set of
    pixels whose float64 pre-threshold value (tests/seg_ref.py) lies within 1e-3 of 0.5 - the undecided band of the mask tests;
  - the predictor chain (yolo/v8/segment/predict.py:17-41) on two seeded 134x224 uint8 images that letter-box into 160x224 by padding alone
    (cv2 is absent here, so a resizing letter-box cannot be pinned): boxes and masks with retina_masks off and on.
The GPU box never runs this file.
"""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_import  # noqa: E402
import seg_ref as SR  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images, seeded_tensor  # noqa: E402
from oracle import nms as onms  # noqa: E402  (only to stand in for the absent torchvision.ops.nms)

torch.set_num_threads(8)
ns = ref_import.load()
REFY = '/root/reference/models/v8/'

DECONV_CASES = {'c16': (1, 16, 9, 13), 'c64': (1, 64, 20, 28)}
PROTO_CASES = {'p16': ((16, 32, 32), (1, 16, 9, 13)), 'p64': ((64, 64, 32), (2, 64, 20, 28))}      # (c1, c_, c2), input shape
FULL_SHAPE = (2, 160, 224)
SHAPES = {(2, 160, 224): (1, 1), (1, 192, 160): (1, 1), (1, 640, 640): (25, 4)}          # (every SUB-th anchor, every PSUB-th proto pixel) recorded
LB_SHAPE = (134, 224)            # original images of the predictor case: letter-box into 160 x 224 by padding 13 rows of 114 above and below
IMG_SEED = 3
NMS_SEG_CASES = (('pred', dict(conf_thres=0.25, iou_thres=0.7, max_det=50)),
                 ('val', dict(conf_thres=0.001, iou_thres=0.7, multi_label=True, max_det=100)),
                 ('cls', dict(conf_thres=0.25, iou_thres=0.7, max_det=50, classes=[0, 3, 7])),
                 ('agn', dict(conf_thres=0.25, iou_thres=0.7, max_det=50, agnostic=True)),
                 ('few', dict(conf_thres=0.38, iou_thres=0.5, max_det=50)))
NATIVE_SHAPES = {'land': (120, 200), 'port': (200, 120)}    # original shapes that letter-box into 160 x 224
BAND_CAP = 0.01


def save(arrs, limit=900 * 1024):
    """Greedy shards seg_00.npz, seg_01.npz, ... of at most `limit` raw bytes, each checked against the 1 MiB limit of a committed file."""
    import glob
    for old in glob.glob(os.path.join(HERE, 'seg_*.npz')) + [os.path.join(HERE, 'seg.npz')]:
        if os.path.exists(old):
            os.remove(old)
    shards, cur, size = [], {}, 0
    for k, v in arrs.items():
        v = np.asarray(v)
        assert v.nbytes <= limit, (k, v.nbytes)
        if size + v.nbytes > limit:
            shards.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    shards.append(cur)
    for n, sh in enumerate(shards):
        path = os.path.join(HERE, f'seg_{n:02d}.npz')
        np.savez_compressed(path, **sh)
        sz = os.path.getsize(path)
        print(f'seg_{n:02d}: {len(sh)} arrays, {sz / 1024:.1f} KiB')
        assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def modules(arrs):
    for name, shape in DECONV_CASES.items():
        c = shape[1]
        m = nn.ConvTranspose2d(c, c, 2, 2, 0, bias=True)
        seed_state_dict_(m, 21)
        x = seeded_tensor(f'deconv_{name}.x', shape, seed=22)
        with torch.no_grad():
            arrs[f'deconv_{name}_y'] = m(x).numpy()
    for name, (args, shape) in PROTO_CASES.items():
        m = ns.modules.Proto(*args)
        seed_state_dict_(m, 23)
        x = seeded_tensor(f'proto_{name}.x', shape, seed=24)
        with torch.no_grad():
            arrs[f'proto_{name}_y'] = m.eval()(x).numpy()


def mspa_seg_yaml(tmp):
    """The fork's MSPA-GD graph with its Detect row replaced by the Segment row of yolov8-seg.yaml."""
    src = open(REFY + 'mspa_c2f_gd_yolov8.yaml').read().splitlines()
    out, done = [], False
    for line in src:
        if 'Detect' in line and line.lstrip().startswith('- [['):
            line = line[:line.index('- [[')] + '- [[15], 1, Segment, [nc, 32, 256]]'
            done = True
        out.append(line)
    assert done
    path = os.path.join(tmp, 'mspa_c2f_gd_yolov8n-seg.yaml')
    open(path, 'w').write('\n'.join(out) + '\n')
    return path


def build(path):
    m = ns.tasks.SegmentationModel(path, nc=80, verbose=False)
    seed_state_dict_(m, 0)
    return m.eval()


def models(arrs, tmp):
    for tag, path in (('yolov8_seg_n', REFY + 'yolov8n-seg.yaml'), ('mspa_c2f_gd_seg_n', mspa_seg_yaml(tmp))):
        m = build(path)
        sd = m.state_dict()
        arrs[f'{tag}_keys'] = np.array(list(sd.keys()))
        arrs[f'{tag}_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
        arrs[f'{tag}_nparams'] = np.array(sum(p.numel() for p in m.parameters()), np.int64)
        arrs[f'{tag}_stride'] = m.stride.numpy()
        assert ns.tasks.guess_model_task(m) == 'segment'
        for shape, (sub, psub) in SHAPES.items():
            key = f'{tag}_{shape[0]}x{shape[1]}x{shape[2]}'
            x = seeded_images(*shape, seed=IMG_SEED)
            with torch.no_grad():
                cat, (feats, mc, p) = m(x)
            assert torch.equal(cat[:, -32:], mc)
            arrs[f'{key}_cat'] = cat[:, :, ::sub].numpy()
            arrs[f'{key}_p'] = p[:, :, ::psub, ::psub].numpy()
            arrs[f'{key}_anchors'] = np.array(cat.shape[-1], np.int64)
            print(key, tuple(cat.shape), tuple(p.shape), 'max |mc|', float(mc.abs().max()), 'max |p|', float(p.abs().max()))
            if tag == 'yolov8_seg_n' and shape == FULL_SHAPE:
                nms_and_masks(arrs, arrs, key, cat, p, shape)
                predictor_case(arrs, m)


def lb_images():
    r = np.random.default_rng([41, 9])
    return [r.integers(0, 256, (*LB_SHAPE, 3), dtype=np.uint8) for _ in range(2)]


def predictor_case(arrs, m):
    """predict.py:17-41 on the padded (no resize) letter-box of two BGR uint8 images: NMS at the predictor's settings, then either
    process_mask(upsample=True) + scale_boxes, or scale_boxes + process_mask_native."""
    imgs = lb_images()
    x = np.full((2, 160, 224, 3), 114, np.uint8)
    for i, im in enumerate(imgs):
        x[i, 13:13 + LB_SHAPE[0]] = im
    x = torch.from_numpy(np.ascontiguousarray(x[..., ::-1].transpose(0, 3, 1, 2))).float() / 255      # BGR -> RGB, HWC -> CHW, /255
    with torch.no_grad():
        cat, (_, _, p) = m(x)
    rows = ns.ops.non_max_suppression(cat.clone(), 0.25, 0.7, nc=80, max_det=50, max_time_img=1e9)
    oshape = (*LB_SHAPE, 3)
    for i, r in enumerate(rows):
        r0 = r.clone()
        masks = ns.ops.process_mask(p[i], r0[:, 6:], r0[:, :4], (160, 224), upsample=True)
        r0[:, :4] = ns.ops.scale_boxes((160, 224), r0[:, :4], oshape)
        arrs[f'lb_off_{i}_boxes'] = r0[:, :6].numpy()
        arrs[f'lb_off_{i}_m'] = SR.pack(masks.bool().numpy())
        arrs[f'lb_off_{i}_shape'] = np.array(masks.shape, np.int64)
        r1 = r.clone()
        r1[:, :4] = ns.ops.scale_boxes((160, 224), r1[:, :4], oshape)
        masks = ns.ops.process_mask_native(p[i], r1[:, 6:], r1[:, :4], oshape[:2])
        arrs[f'lb_on_{i}_boxes'] = r1[:, :6].numpy()
        arrs[f'lb_on_{i}_m'] = SR.pack(masks.bool().numpy())
        arrs[f'lb_on_{i}_shape'] = np.array(masks.shape, np.int64)
        print('predictor case', i, tuple(r.shape), tuple(masks.shape))


def nms_and_masks(arrs, marrs, key, cat, p, shape):
    for cname, kw in NMS_SEG_CASES:
        out = ns.ops.non_max_suppression(cat.clone(), nc=80, max_time_img=1e9, **kw)
        for i, o in enumerate(out):
            assert o.shape[1] == 38
            arrs[f'{key}_nms_{cname}_{i}'] = o.numpy()
        print('nms', cname, [int(o.shape[0]) for o in out])
        if cname == 'few':
            n = [int(o.shape[0]) for o in out]
            assert min(n) < kw['max_det'] and max(n) > 0, n
    rows = ns.ops.non_max_suppression(cat.clone(), nc=80, max_time_img=1e9, **dict(NMS_SEG_CASES)['pred'])
    ishape = shape[1:]
    mh, mw = p.shape[2:]

    def record(name, ref_masks, values):
        und = SR.undecided(values)
        share = float(und.double().mean())
        got = values > 0.5
        bad = int(((got != ref_masks.bool()) & ~und).sum())
        print(f'  {name}: {tuple(ref_masks.shape)} ones {float(ref_masks.mean()):.4f} undecided {share:.5f} fp64-vs-reference outside the band {bad}')
        assert share <= BAND_CAP, (name, share)
        assert bad == 0, (name, bad)
        marrs[f'{name}_m'] = SR.pack(ref_masks.bool().numpy())
        marrs[f'{name}_u'] = SR.pack(und.numpy())
        marrs[f'{name}_shape'] = np.array(ref_masks.shape, np.int64)

    for i, r in enumerate(rows):
        boxes, mc = r[:, :4], r[:, 6:]
        # tile geometry facts the tests rely on: a box crossing a 32 x 128 output-tile border and a tile wholly outside some box
        if i == 0:
            assert bool(((boxes[:, 0] < 128) & (boxes[:, 2] > 128)).any()) and bool((boxes[:, 2] < 128).any() or (boxes[:, 0] >= 128).any())
        record(f'pm_{i}', ns.ops.process_mask(p[i], mc, boxes, ishape, upsample=False), SR.mask_values(p[i], mc, boxes, ishape, 'process_mask'))
        record(f'pmup_{i}', ns.ops.process_mask(p[i], mc, boxes, ishape, upsample=True), SR.mask_values(p[i], mc, boxes, ishape, 'process_mask_up'))
        record(f'pmu_{i}', ns.ops.process_mask_upsample(p[i], mc, boxes, ishape), SR.mask_values(p[i], mc, boxes, ishape, 'process_mask_upsample'))
    r = rows[0]
    for nname, oshape in NATIVE_SHAPES.items():
        boxes = ns.ops.scale_boxes(ishape, r[:, :4].clone(), oshape)
        marrs[f'native_{nname}_boxes'] = boxes.numpy()
        record(f'native_{nname}', ns.ops.process_mask_native(p[0], r[:, 6:], boxes, oshape),
               SR.mask_values(p[0], r[:, 6:], boxes, oshape, 'process_mask_native'))


def main():
    import torchvision  # the stand-in module from ref_import

    def nms_standin(boxes, scores, thr):
        assert bool((scores[:-1] >= scores[1:]).all()), 'reference hands nms() descending scores'
        return torch.from_numpy(onms.greedy_nms(boxes.numpy(), thr))

    torchvision.ops.nms = nms_standin
    arrs = {}
    modules(arrs)
    with tempfile.TemporaryDirectory() as tmp:
        models(arrs, tmp)
    save(arrs)


if __name__ == '__main__':
    main()
