"""Generate tests/golden/segval_NN.npz: segmentation-validation fixtures from the reference's own Python modules.

    python tests/golden/gen_segval.py

Same recipe as gen_golden.py:val_match: `SegmentationValidator._process_batch` (yolo/v8/segment/val.py:131-166) is taken out of its class with
`ast` (importing the file pulls in the dataset / plotting stack) and executed as is, bound to the reference's own `mask_iou` and `box_iou`;
`ap_per_class` is the reference's.  Inputs come from seeds (tests/segval_ref.py), so only results are stored:
  - per image of every synthetic case: the mask IoU matrix (float32, both ground-truth forms give the same one: the instance masks are the index
    map's own), `correct` for boxes and for masks; per case the eight summary numbers of two `ap_per_class` calls;
  - the asymmetric cases (distinct areas, pairwise distinct intersections - checked here): the IoU matrix;
  - ground truth at another resolution: the reference's resampled, thresholded masks (captured at its `mask_iou` call), bit-packed, and the
    bit-packed set of pixels whose float64 value lies within 1e-5 of 0.5 (empty for the ratio 4);
  - the whole chain: the `val` NMS rows and protos of seg_NN.npz (yolov8_seg_n_2x160x224) through the reference's `process_mask` (masks and the
    pixels within 1e-3 of the threshold, bit-packed; band capped at 1 %), seeded labels made from the detections' own reference masks, both
    `correct` matrices, the eight summary numbers, and the detections that own a band pixel and have a candidate IoU within band_pixels / union of
    a level (capped at 2 % here): the only ones whose mask matching may differ on a device whose masks differ inside the band.
Conditions asserted here: no two equal IoU values among the candidate pairs (iou >= 0.5, same class) of an image, for masks and for boxes; at
least 5 true positives at level 0.5 and fewer at 0.95 in every matching case; at most 0.1 % of the pixels in a resampling band; float32 restatement
(tests/segval_ref.py) equal to the reference bit for bit.
"""
import ast
import glob
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_import  # noqa: E402
import segval_ref as R  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()


def reference_process_batch():
    src = open(os.path.join(ref_import.REF, 'yolo/v8/segment/val.py')).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == 'SegmentationValidator')
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == '_process_batch')
    env = {'np': np, 'torch': torch, 'F': F, 'box_iou': ns.metrics.box_iou, 'mask_iou': ns.metrics.mask_iou}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), 'ref:_process_batch', 'exec'), env)
    return env


def no_ties(iou, lab, det, what):
    cand = iou[(iou >= 0.5) & (lab[:, 0:1] == det[None, :, 5])]
    assert len(np.unique(cand)) == len(cand), f'{what}: {len(cand) - len(np.unique(cand))} equal IoU values among {len(cand)} candidate pairs'
    return len(cand)


def summary(tp, conf, pcls, tcls):
    if not tp.any():
        return np.zeros(4)
    _, _, p, r, _, ap, _ = ns.metrics.ap_per_class(tp, conf, pcls, tcls, names={})
    return np.array([p.mean(), r.mean(), ap[:, 0].mean(), ap.mean()])


def synthetic(arrs, env):
    me = types.SimpleNamespace(iouv=torch.linspace(0.5, 0.95, 10))
    assert np.array_equal(me.iouv.numpy(), R.IOUV)
    pb = env['_process_batch']
    for name in R.CASES:
        stats = []
        for k, (idx, pred, det, lab) in enumerate(R.case_inputs(name)):
            nd, nl = det.shape[0], lab.shape[0]
            gt = R.instances(idx, nl)
            key = f'{name}_{k}'
            iou = ns.metrics.mask_iou(torch.from_numpy(gt).float().view(nl, -1), torch.from_numpy(pred).float().view(nd, -1)).numpy() if nd and nl \
                else np.zeros((nl, nd), np.float32)
            assert not (nd and nl) or np.array_equal(iou, R.mask_iou_exact(gt, pred)), key
            cb = cm = np.zeros((nd, 10), bool)
            if nd and nl:       # val.py:71-111: the caller never reaches _process_batch with an empty side
                d, l = torch.from_numpy(det), torch.from_numpy(lab)
                cb = pb(me, d, l).numpy()
                cm = pb(me, d, l, torch.from_numpy(pred).float(), torch.from_numpy(idx)[None].float(), overlap=True, masks=True).numpy()
                cm2 = pb(me, d, l, torch.from_numpy(pred).float(), torch.from_numpy(gt).float(), overlap=False, masks=True).numpy()
                assert np.array_equal(cm, cm2), key
                nc_m = no_ties(iou, lab, det, key + ' masks')
                biou = ns.metrics.box_iou(l[:, 1:], d[:, :4]).numpy()
                nc_b = no_ties(biou, lab, det, key + ' boxes')
                assert np.array_equal(biou, R.box_iou_f32(lab[:, 1:], det[:, :4])), key
                assert np.array_equal(cm, R.match(iou, lab[:, 0], det[:, 5])), key
                assert np.array_equal(cb, R.match(biou, lab[:, 0], det[:, 5])), key
                print(f'{key}: nd {nd} nl {nl} candidates masks {nc_m} boxes {nc_b} tp masks {cm.sum(0).tolist()} boxes {cb.sum(0).tolist()}')
            arrs[key + '_iou'], arrs[key + '_cb'], arrs[key + '_cm'] = iou, cb, cm
            if nd or nl:
                stats.append((cb, cm, det[:, 4], det[:, 5], lab[:, 0]))
        cb, cm, conf, pcls, tcls = [np.concatenate(x, 0) for x in zip(*stats)]
        assert cm[:, 0].sum() >= 5 and cm[:, 9].sum() < cm[:, 0].sum(), (name, cm.sum(0))
        assert cb[:, 0].sum() >= 5 and cb[:, 9].sum() < cb[:, 0].sum(), (name, cb.sum(0))
        arrs[name + '_summary'] = np.concatenate([summary(cb, conf, pcls, tcls), summary(cm, conf, pcls, tcls)])
        print(name, 'summary', arrs[name + '_summary'].round(4).tolist())
    for name in R.ASYM_CASES:
        gt, pred, _ = R.asym_inputs(name)
        nl, nd = gt.shape[0], pred.shape[0]
        g, p = gt.reshape(nl, -1).astype(np.int64), pred.reshape(nd, -1).astype(np.int64)
        inter = g @ p.T
        assert len(np.unique(g.sum(1))) == nl and len(np.unique(p.sum(1))) == nd and len(np.unique(inter)) == inter.size, name
        iou = ns.metrics.mask_iou(torch.from_numpy(gt).float().view(nl, -1), torch.from_numpy(pred).float().view(nd, -1)).numpy()
        assert np.array_equal(iou, R.mask_iou_exact(gt, pred)), name
        arrs[name + '_iou'] = iou
        print(name, 'distinct areas and intersections; iou', float(iou.min()), float(iou.max()))


def resample(arrs, env):
    me = types.SimpleNamespace(iouv=torch.linspace(0.5, 0.95, 10))
    for name in R.RESAMPLE_CASES:
        idx, nl, out = R.resample_inputs(name)
        seen = []

        def capture(m1, m2, eps=1e-7):
            seen.append(m1.clone())
            return ns.metrics.mask_iou(m1, m2, eps)
        env['mask_iou'] = capture
        det = np.zeros((2, 6), np.float32)
        lab = np.zeros((nl, 5), np.float32)
        env['_process_batch'](me, torch.from_numpy(det), torch.from_numpy(lab), torch.zeros(2, *out), torch.from_numpy(idx)[None].float(), overlap=True,
                              masks=True)
        env['mask_iou'] = ns.metrics.mask_iou
        ref = seen[0].view(nl, *out).numpy() > 0
        vals = np.stack([R.resample_values(idx == j + 1, out) for j in range(nl)])
        band = np.abs(vals - 0.5) <= R.RESAMPLE_BAND
        bad = int((((vals > 0.5) != ref) & ~band).sum())
        share = float(band.mean())
        print(f'{name}: {idx.shape} -> {out}, ones {ref.mean():.4f}, band {share:.6f}, float64 vs reference outside the band {bad}')
        assert bad == 0 and share <= 1e-3, (name, bad, share)
        if name == 'r4':
            assert not band.any()
        arrs[name + '_m'], arrs[name + '_u'] = R.pack(ref), R.pack(band)


def whole_chain(arrs, env):
    """The `val` NMS rows and the protos seg_NN.npz holds for yolov8_seg_n_2x160x224 through the reference's process_mask and _process_batch.
    Ground truth (instance form): every other of an image's first 40 detections with its own reference mask shifted / dilated by seeded amounts and
    its box jittered, plus two instances nothing predicts."""
    import seg_ref as SR
    f = SR.load_fixture()
    me = types.SimpleNamespace(iouv=torch.linspace(0.5, 0.95, 10))
    pb = env['_process_batch']
    tag, ishape = R.CHAIN_TAG, R.CHAIN_SHAPE
    p = torch.from_numpy(f[tag + '_p'])
    stats = []
    for i in range(p.shape[0]):
        rows = torch.from_numpy(f[f'{tag}_nms_val_{i}'])
        n = rows.shape[0]
        boxes, mc = rows[:, :4], rows[:, 6:]
        ref = ns.ops.process_mask(p[i], mc, boxes, ishape, upsample=False)
        values = SR.mask_values(p[i], mc, boxes, ishape, 'process_mask')
        und = SR.undecided(values)
        share = float(und.double().mean())
        bad = int((((values > 0.5) != ref.bool()) & ~und).sum())
        assert share <= 0.01 and bad == 0, (i, share, bad)
        pm = ref.bool().numpy()
        r = np.random.default_rng([92, i])
        gts, lab = [], []
        for d in range(0, min(n, 40), 2):
            g = R._shift(pm[d], int(r.integers(-1, 2)), int(r.integers(-1, 2)))
            if r.random() < 0.5:
                g = R._dilate(g)
            if g.any():
                gts.append(g)
                lab.append([float(rows[d, 5]), *(rows[d, :4].numpy().astype(np.float64) + r.uniform(-3, 3, 4))])
        for _ in range(2):
            g = R._shape(r, *pm.shape[1:], 0.2)
            gts.append(g)
            lab.append([79.0, *(R._bbox(g, r, 0.0) * 4)])
        gt, lab = np.stack(gts).astype(np.uint8), np.array(lab, np.float32)
        det = rows[:, :6].numpy()
        d_t, l_t = torch.from_numpy(det), torch.from_numpy(lab)
        cb = pb(me, d_t, l_t).numpy()
        cm = pb(me, d_t, l_t, ref, torch.from_numpy(gt).float(), overlap=False, masks=True).numpy()
        iou = R.mask_iou_exact(gt, pm.astype(np.uint8))
        assert np.array_equal(cm, R.match(iou, lab[:, 0], det[:, 5])), i
        nc_m = no_ties(iou, lab, det, f'chain {i} masks')
        nc_b = no_ties(ns.metrics.box_iou(l_t[:, 1:], d_t[:, :4]).numpy(), lab, det, f'chain {i} boxes')
        # detections whose matching may legitimately differ on a device whose masks differ inside the band: they own band pixels and one of their
        # candidate IoUs lies within band_pixels / union of a level
        g64, p64 = gt.reshape(len(gt), -1).astype(np.int64), pm.reshape(n, -1).astype(np.int64)
        inter = g64 @ p64.T
        union = g64.sum(1)[:, None] + p64.sum(1)[None] - inter
        bp = und.reshape(n, -1).sum(1).numpy()
        near = (np.abs(iou[:, :, None].astype(np.float64) - R.IOUV[None, None].astype(np.float64)) <= (bp[None] / np.maximum(union, 1))[:, :, None]).any(2)
        exc = (bp > 0) & (near & (lab[:, 0:1] == det[None, :, 5])).any(0)
        assert exc.mean() <= 0.02, (i, int(exc.sum()), n)
        print(f'chain {i}: {n} detections, {len(gt)} labels, band {share:.5f}, candidates masks {nc_m} boxes {nc_b}, tp masks {cm.sum(0).tolist()} boxes '
              f'{cb.sum(0).tolist()}, excepted {int(exc.sum())}')
        k = f'chain_{i}'
        arrs[k + '_m'], arrs[k + '_u'], arrs[k + '_gt'] = R.pack(pm), R.pack(und.numpy()), R.pack(gt)
        arrs[k + '_lab'], arrs[k + '_cb'], arrs[k + '_cm'], arrs[k + '_exc'] = lab, cb, cm, exc
        stats.append((cb, cm, det[:, 4], det[:, 5], lab[:, 0]))
    cb, cm, conf, pcls, tcls = [np.concatenate(x, 0) for x in zip(*stats)]
    assert cm[:, 0].sum() >= 5 and cm[:, 9].sum() < cm[:, 0].sum() and cb[:, 0].sum() >= 5 and cb[:, 9].sum() < cb[:, 0].sum()
    arrs['chain_summary'] = np.concatenate([summary(cb, conf, pcls, tcls), summary(cm, conf, pcls, tcls)])
    print('chain summary', arrs['chain_summary'].round(4).tolist())


def save(arrs, limit=900 * 1024):
    for old in glob.glob(os.path.join(HERE, 'segval_*.npz')):
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
        path = os.path.join(HERE, f'segval_{n:02d}.npz')
        np.savez_compressed(path, **sh)
        sz = os.path.getsize(path)
        print(f'segval_{n:02d}: {len(sh)} arrays, {sz / 1024:.1f} KiB')
        assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def main():
    env = reference_process_batch()
    arrs = {}
    synthetic(arrs, env)
    resample(arrs, env)
    whole_chain(arrs, env)
    save(arrs)


if __name__ == '__main__':
    main()
