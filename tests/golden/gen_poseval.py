"""Generate tests/golden/poseval_00.npz: pose-validation fixtures from the reference's own Python modules.

    python tests/golden/gen_poseval.py

Same recipe as gen_segval.py: `PoseValidator._process_batch` (yolo/v8/pose/val.py:110-141) is taken out of its class with `ast` (importing the file
pulls in the dataset / plotting stack) and executed as is on a stand-in `self` that carries `iouv` and `sigma`, bound to the reference's own
`kpt_iou`, `box_iou` and `ops`; `scale_boxes`, `scale_coords`, `xywh2xyxy` and `ap_per_class` are the reference's.  Inputs come from seeds
(tests/poseval_ref.py), so only results are stored.  Per image of every case:
  - `<key>_oks`: the reference's float32 OKS matrix (nl, nd); `<key>_oks64`: the same function on the same inputs as float64 tensors;
  - `<key>_cb`, `<key>_ck`: `correct` for boxes and for keypoints;
  - `<key>_exc`: the detections with a same-class candidate whose float64 OKS lies within 1e-5 of a level of iouv;
per case `<case>_d64` = max |fp32 - fp64| over its images and `<case>_summary`, the eight numbers of two `ap_per_class` calls; `oks_sigma`.
Cases: t1, t2, k5 (synthetic, in native space already) and chain_pad / chain_gain: the `val` NMS rows of pose_NN.npz with seeded dataloader-style
labels through val.py:75-97 (scale_boxes, scale_coords on predictions and labels) for a padded letter-box and for one with gain != 1.
Conditions asserted here: the exception list covers at most 2 % of a case's detections; no detection has two same-class candidates (OKS >= 0.5)
within 1e-5 of each other; the float64 restatement (poseval_ref.kpt_iou64) equals the reference's float64 matrix to 1e-12 and the float32
restatements of area and of the letter-box scaling equal the reference bit for bit; `segval_ref.match` reproduces both `correct` matrices; at
least 5 true positives at level 0.5 and fewer at 0.95, for boxes and for keypoints, in every case but t1, whose three images (1 / 0 / 65
detections against 1 / 4 / 0 labels) admit one pair at most: there the single pair must be a true positive at 0.5 for both.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pose_ref as PR  # noqa: E402
import poseval_ref as R  # noqa: E402
import ref_import  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()
EXC_CAP = 0.02


def reference_process_batch():
    src = open(os.path.join(ref_import.REF, 'yolo/v8/pose/val.py')).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == 'PoseValidator')
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == '_process_batch')
    env = {'np': np, 'torch': torch, 'ops': ns.ops, 'box_iou': ns.metrics.box_iou, 'kpt_iou': ns.metrics.kpt_iou}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), 'ref:_process_batch', 'exec'), env)
    return env['_process_batch']


def summary(tp, conf, pcls, tcls):
    if not tp.any():
        return np.zeros(4)
    _, _, p, r, _, ap, _ = ns.metrics.ap_per_class(tp, conf, pcls, tcls, names={})
    return np.array([p.mean(), r.mean(), ap[:, 0].mean(), ap.mean()])


def one_image(arrs, key, pb, me, det, pk, lab, gk):
    """det (nd, 6), pk (nd, nkpt, 2 | 3), lab (nl, 5), gk (nl, nkpt, 3), all native space float32 -> the image's records; returns its stats row."""
    nd, nl = det.shape[0], lab.shape[0]
    oks = np.zeros((nl, nd), np.float32)
    oks64 = np.zeros((nl, nd), np.float64)
    cb = ck = np.zeros((nd, 10), bool)
    exc = np.zeros(nd, bool)
    if nd and nl:       # val.py:67-97: the caller never reaches _process_batch with an empty side
        d_t, l_t, p_t, g_t = (torch.from_numpy(np.ascontiguousarray(a)) for a in (det, lab, pk, gk))
        area = ns.ops.xyxy2xywh(l_t[:, 1:])[:, 2:].prod(1) * 0.53
        assert np.array_equal(area.numpy(), R.area_f32(lab)), key
        oks = ns.metrics.kpt_iou(g_t, p_t, sigma=me.sigma, area=area).numpy()
        oks64 = ns.metrics.kpt_iou(g_t.double(), p_t.double(), sigma=me.sigma, area=area.double()).numpy()
        assert oks.dtype == np.float32 and oks64.dtype == np.float64 and not np.isnan(oks).any()
        assert np.abs(R.kpt_iou64(gk, pk, area.numpy(), me.sigma) - oks64).max() <= 1e-12, key
        cb = pb(me, d_t, l_t).numpy()
        ck = pb(me, d_t, l_t, p_t, g_t).numpy()
        assert np.array_equal(ck, R.match(oks, lab[:, 0], det[:, 5])), key
        assert np.array_equal(cb, R.match(R.box_iou_f32(lab[:, 1:], det[:, :4]), lab[:, 0], det[:, 5])), key
        exc = R.near_level(oks64, lab[:, 0], det[:, 5])
        assert not (R.match(oks64, lab[:, 0], det[:, 5]) != ck)[~exc].any(), key
        cand = np.where((oks64 >= 0.5 - R.NEAR) & (lab[:, 0:1] == det[None, :, 5]), oks64, np.nan)
        for d in range(nd):
            v = np.sort(cand[:, d][~np.isnan(cand[:, d])])
            assert len(v) < 2 or np.diff(v).min() > R.NEAR, (key, d, 'two candidates of one detection within 1e-5')
        print(f'{key}: nd {nd} nl {nl} max|fp32-fp64| {np.abs(oks - oks64).max():.2e} tp kpts {ck.sum(0).tolist()} boxes {cb.sum(0).tolist()} '
              f'excepted {int(exc.sum())}')
    arrs[key + '_oks'], arrs[key + '_oks64'], arrs[key + '_cb'], arrs[key + '_ck'], arrs[key + '_exc'] = oks, oks64, cb, ck, exc
    return (cb, ck, det[:, 4], det[:, 5], lab[:, 0]) if (nd or nl) else None


def close_case(arrs, name, stats, keys, need=5):
    cb, ck, conf, pcls, tcls = [np.concatenate(x, 0) for x in zip(*[s for s in stats if s is not None])]
    d64 = max(float(np.abs(arrs[k + '_oks'] - arrs[k + '_oks64']).max()) if arrs[k + '_oks'].size else 0.0 for k in keys)
    exc = np.concatenate([arrs[k + '_exc'] for k in keys])
    assert exc.mean() <= EXC_CAP, (name, int(exc.sum()), len(exc))
    for what, c in (('boxes', cb), ('keypoints', ck)):
        if need >= 5:
            assert c[:, 0].sum() >= need and c[:, 9].sum() < c[:, 0].sum(), (name, what, c.sum(0))
        else:
            assert c[:, 0].sum() == need, (name, what, c.sum(0))
    arrs[name + '_d64'] = np.array(d64, np.float64)
    arrs[name + '_summary'] = np.concatenate([summary(cb, conf, pcls, tcls), summary(ck, conf, pcls, tcls)])
    print(f'{name}: d64 {d64:.3e} excepted {int(exc.sum())} / {len(exc)} summary {arrs[name + "_summary"].round(4).tolist()}')


def synthetic(arrs, pb):
    for name, (kpt_shape, nc, _) in R.CASES.items():
        me = types.SimpleNamespace(iouv=torch.linspace(0.5, 0.95, 10), sigma=R.sigma_of(kpt_shape))
        assert np.array_equal(me.iouv.numpy(), R.IOUV)
        stats, keys = [], []
        for k, (det, kp, lab, gk) in enumerate(R.case_inputs(name)):
            keys.append(f'{name}_{k}')
            stats.append(one_image(arrs, keys[-1], pb, me, det, kp, lab, gk))
        close_case(arrs, name, stats, keys, need=1 if name == 't1' else 5)
    gk = R.case_inputs('t2')[0][3]
    assert not gk[3, :, 2].any() and not arrs['t2_0_oks'][3].any() and not arrs['t2_0_oks'][5].any(), 'no visible keypoint / zero area must give 0'


def chain(arrs, pb):
    """val.py:75-97 with the reference's own helpers on the fixture rows and the seeded dataloader-style labels."""
    H, W = R.FRAME
    me = types.SimpleNamespace(iouv=torch.linspace(0.5, 0.95, 10), sigma=R.sigma_of((17, 3)))
    rows, batch = R.chain_inputs(PR.load_fixture())
    for tag, (shape, rp) in R.CHAIN_BOXES.items():
        stats, keys = [], []
        for si, pred in enumerate(rows):
            sel = batch['batch_idx'] == si
            cls, bbox, kpts = (torch.from_numpy(batch[k][sel]) for k in ('cls', 'bboxes', 'keypoints'))
            pred = torch.from_numpy(pred)
            npr = pred.shape[0]
            predn = pred.clone()
            ns.ops.scale_boxes((H, W), predn[:, :4], shape, ratio_pad=rp)
            pred_kpts = predn[:, 6:].view(npr, 17, -1)
            ns.ops.scale_coords((H, W), pred_kpts, shape, ratio_pad=rp)
            tbox = ns.ops.xywh2xyxy(bbox) * torch.tensor((W, H, W, H))
            ns.ops.scale_boxes((H, W), tbox, shape, ratio_pad=rp)
            tkpts = kpts.clone()
            tkpts[..., 0] *= W
            tkpts[..., 1] *= H
            tkpts = ns.ops.scale_coords((H, W), tkpts, shape, ratio_pad=rp)
            labelsn = torch.cat((cls, tbox), 1)
            # the float32 restatement of the scaling, bit for bit
            lab_r, tk_r = R.native_labels((H, W), batch['cls'][sel], batch['bboxes'][sel], batch['keypoints'][sel], shape, rp)
            assert np.array_equal(lab_r, labelsn.numpy()) and np.array_equal(tk_r, tkpts.numpy()), (tag, si, 'labels')
            assert np.array_equal(R.scale_boxes_f32((H, W), rows[si], shape, rp), predn[:, :4].numpy()), (tag, si, 'boxes')
            assert np.array_equal(R.scale_coords_f32((H, W), rows[si][:, 6:].reshape(npr, 17, 3), shape, rp), pred_kpts.numpy()), (tag, si, 'keypoints')
            keys.append(f'chain_{tag}_{si}')
            stats.append(one_image(arrs, keys[-1], pb, me, predn[:, :6].numpy(), pred_kpts.numpy(), labelsn.numpy(), tkpts.numpy()))
        close_case(arrs, f'chain_{tag}', stats, keys)


def main():
    pb = reference_process_batch()
    arrs = {'oks_sigma': np.asarray(ns.metrics.OKS_SIGMA)}
    assert arrs['oks_sigma'].dtype == np.float64 and np.array_equal(arrs['oks_sigma'], R.OKS_SIGMA)
    synthetic(arrs, pb)
    chain(arrs, pb)
    path = os.path.join(HERE, 'poseval_00.npz')
    np.savez_compressed(path, **arrs)
    sz = os.path.getsize(path)
    print(f'poseval_00: {len(arrs)} arrays, {sz / 1024:.1f} KiB')
    assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


if __name__ == '__main__':
    main()
