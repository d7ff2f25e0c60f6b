"""Generate tests/golden/pose_NN.npz and tests/golden/pose_yaml.json: pose-estimation fixtures from the reference's own Python modules (BUILD
CONTAINER ONLY).

    python tests/golden/gen_pose.py

Same recipe as gen_seg.py (ref_import, seeded weights (pose_ref.seed_pose_) and images, CPU fp32, the oracle's greedy NMS standing in for torchvision).  Recorded:
  - pose_yaml.json: the reference's models/v8/yolov8-pose.yaml parsed to a dict (a settings fixture);
  - PoseModel('yolov8-pose') at scales n and s and the MSPA-GD graph with its Detect row replaced by Pose [nc, kpt_shape] (written to a temporary
    YAML and parsed by the reference) at scale n, nc = 1: state-dict keys / shapes, parameter count, stride (scale s: these only);
  - for the cases of tests/pose_ref.py:CASES (yolov8-pose n at 2x96x160 and 1x160x224, the same with kpt_shape (5, 2), the MSPA-GD pose graph): the
    eval output cat(y, pred_kpt) and the raw kpt in full; the output of the same model converted with .double() on the same input and the largest
    fp32-vs-fp64 difference per quantity (box px, confidence, keypoint px, keypoint visibility); and the largest difference to a bf16 EMULATION
    of the same model: every parameter and the input rounded to bf16, the output of every Conv (conv + BN + SiLU) and of every bare nn.Conv2d
    (the heads' closing 1x1 convolutions; not the DFL's fixed one) rounded to bf16 by a forward hook, the closing arithmetic in fp32;
  - for yolov8-pose n at 2x96x160: NMS rows (n, 6 + 51) at four settings chosen HERE from the score distribution (seeded weights give low
    confidences), stored with the rows: the predictor's, the validator's (conf 0.001, multi_label, max_det 100), class-agnostic, and one that
    leaves every image with fewer rows than max_det;
  - the predictor chain (yolo/v8/pose/predict.py:16-41) on two seeded 134x224 uint8 images that letter-box into 160x224 by padding alone (cv2 is
    absent here): boxes before and after .round(), keypoints after scale_coords, and the rows whose pre-round coordinate lies within the fp32 box
    tolerance (1e-3 px) of a .5 boundary;
  - scale_coords alone on seeded coordinates (pose_ref.seeded_coords) for two original shapes, one gain-limited by the width and one by the height.
The GPU box never runs this file.
"""
import copy
import json
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

import pose_ref as PR  # noqa: E402
import ref_import  # noqa: E402
from mgdt_yolo_amd.seeding import seeded_images  # noqa: E402
from oracle import nms as onms  # noqa: E402  (only to stand in for the absent torchvision.ops.nms)

torch.set_num_threads(8)
ns = ref_import.load()
REFY = '/root/reference/models/v8/'
MAX_DET = 50
ROUND_BAND = 1e-3            # the fp32 box tolerance: a pre-round coordinate this close to k + 0.5 may round either way
ROUND_CAP = 0.02


def save(arrs, limit=900 * 1024):
    """Greedy shards pose_00.npz, pose_01.npz, ... of at most `limit` raw bytes, each checked against the 1 MiB limit of a committed file."""
    import glob
    for old in glob.glob(os.path.join(HERE, 'pose_[0-9][0-9].npz')):
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
        path = os.path.join(HERE, f'pose_{n:02d}.npz')
        np.savez_compressed(path, **sh)
        sz = os.path.getsize(path)
        print(f'pose_{n:02d}: {len(sh)} arrays, {sz / 1024:.1f} KiB')
        assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def mspa_pose_yaml(tmp):
    """The fork's MSPA-GD graph with its Detect row replaced by the Pose row of yolov8-pose.yaml."""
    src = open(REFY + 'mspa_c2f_gd_yolov8.yaml').read().splitlines()
    out, done, kp = [], False, False
    for line in src:
        if 'Detect' in line and line.lstrip().startswith('- [['):
            line = line[:line.index('- [[')] + '- [[15], 1, Pose, [nc, kpt_shape]]'
            done = True
        out.append(line)
        if line.startswith('nc:') and not kp:
            out.append('kpt_shape: [17, 3]')
            kp = True
    assert done and kp
    path = os.path.join(tmp, 'mspa_c2f_gd_yolov8n-pose.yaml')
    open(path, 'w').write('\n'.join(out) + '\n')
    return path


def build(path, kpt_shape=(None, None)):
    m = ns.tasks.PoseModel(path, nc=1, data_kpt_shape=kpt_shape, verbose=False)
    PR.seed_pose_(m, 0)
    return m.eval()


def structure(arrs, tag, m):
    sd = m.state_dict()
    arrs[f'{tag}_keys'] = np.array(list(sd.keys()))
    arrs[f'{tag}_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
    arrs[f'{tag}_nparams'] = np.array(sum(p.numel() for p in m.parameters()), np.int64)
    arrs[f'{tag}_stride'] = m.stride.numpy()
    assert ns.tasks.guess_model_task(m) == 'pose'


def bf16_emulation(m):
    """A copy of `m` whose parameters are rounded to bf16 and whose Conv / bare nn.Conv2d outputs are rounded to bf16 by forward hooks."""
    e = copy.deepcopy(m)
    r = lambda t: t.to(torch.bfloat16).to(torch.float32)
    with torch.no_grad():
        for p in e.parameters():
            p.copy_(r(p))
    inside = set()
    for mod in e.modules():
        if isinstance(mod, ns.modules.Conv):
            inside.add(id(mod.conv))
            mod.register_forward_hook(lambda _m, _i, o: r(o))
    for name, mod in e.named_modules():
        if isinstance(mod, nn.Conv2d) and id(mod) not in inside and not name.endswith('dfl.conv'):
            mod.register_forward_hook(lambda _m, _i, o: r(o))
    e.model[-1].shape = None
    return e, r


def run_cases(arrs, tmp):
    mspa = mspa_pose_yaml(tmp)
    paths = {'yolov8-pose': REFY + 'yolov8n-pose.yaml', 'mspa_c2f_gd_yolov8-pose': mspa}
    structure(arrs, 'yolov8_pose_n', build(paths['yolov8-pose']))
    structure(arrs, 'yolov8_pose_s', build(REFY + 'yolov8s-pose.yaml'))
    structure(arrs, 'mspa_c2f_gd_pose_n', build(mspa))
    full_model = None
    for tag, (name, kpt_shape, shape) in PR.CASES.items():
        m = build(paths[name], kpt_shape if kpt_shape != (17, 3) else (None, None))
        assert tuple(m.model[-1].kpt_shape) == kpt_shape
        if kpt_shape != (17, 3):
            structure(arrs, 'yolov8_pose_k5x2_n', m)
        x = seeded_images(*shape, seed=PR.IMG_SEED)
        with torch.no_grad():
            pred, (feats, kpt) = m(x)
            m64 = copy.deepcopy(m).double()
            m64.model[-1].shape = None
            pred64, (_, kpt64) = m64(x.double())
            e, r = bf16_emulation(m)
            predb, (_, kptb) = e(r(x))
        nk = kpt_shape[0] * kpt_shape[1]
        assert pred.shape[1] == 5 + nk and tuple(kpt.shape) == (shape[0], nk, pred.shape[2]) and pred64.dtype == torch.float64
        arrs[f'{tag}_pred'] = pred.numpy()
        arrs[f'{tag}_kpt'] = kpt.numpy()
        arrs[f'{tag}_pred64'] = pred64.numpy()
        d64 = PR.max_diffs(pred.numpy(), pred64.numpy(), 1, kpt_shape)
        db = PR.max_diffs(pred.numpy(), predb.numpy(), 1, kpt_shape)
        arrs[f'{tag}_d64'] = np.array([d64[q] for q in PR.QUANTITIES], np.float64)
        arrs[f'{tag}_dbf16'] = np.array([db[q] for q in PR.QUANTITIES], np.float64)
        arrs[f'{tag}_dkpt64'] = np.array(float((kpt.double() - kpt64).abs().max()), np.float64)
        arrs[f'{tag}_dkptbf16'] = np.array(float((kpt - kptb).abs().max()), np.float64)
        arrs[f'{tag}_levels'] = np.array([[f.shape[2], f.shape[3]] for f in feats], np.int64)
        fp32_bounds = {'box': 1e-3, 'conf': 1e-4, 'kxy': max(1e-3, 4 * d64['kxy']), 'kvis': max(1e-4, 4 * d64['kvis'])}
        print(f'{tag}: pred {tuple(pred.shape)} max |kpt raw| {float(kpt.abs().max()):.3f}')
        print('   fp32 vs fp64   ' + '  '.join(f'{q} {d64[q]:.3e}' for q in PR.QUANTITIES) + f'  raw kpt {float(arrs[f"{tag}_dkpt64"]):.3e}')
        print('   fp32 bounds    ' + '  '.join(f'{q} {fp32_bounds[q]:.3e}' for q in PR.QUANTITIES))
        print('   bf16 emulation ' + '  '.join(f'{q} {db[q]:.3e}' for q in PR.QUANTITIES) + f'  raw kpt {float(arrs[f"{tag}_dkptbf16"]):.3e}')
        print('   bf16 bounds    ' + '  '.join(f'{q} {3 * db[q]:.3e}' for q in PR.QUANTITIES))
        assert 3 * db['kxy'] < 4.0, f'{tag}: the bf16 keypoint bound {3 * db["kxy"]} px is not below half the smallest stride: the emulation is wrong'
        if tag == PR.FULL:
            full_model = m
            nms_cases(arrs, tag, pred)
    predictor_case(arrs, full_model)


def nms_cases(arrs, tag, pred):
    sc = pred[:, 4]
    q = lambda p: round(float(torch.quantile(sc.reshape(-1), p)), 4)
    print('scores: min %.4f median %.4f max %.4f' % (float(sc.min()), float(sc.median()), float(sc.max())))
    cases = {'pred': dict(conf_thres=q(0.5), iou_thres=0.7, max_det=MAX_DET),
             'val': dict(conf_thres=0.001, iou_thres=0.7, multi_label=True, max_det=100),
             'agn': dict(conf_thres=q(0.5), iou_thres=0.7, max_det=MAX_DET, agnostic=True),
             'few': dict(conf_thres=q(0.93), iou_thres=0.5, max_det=MAX_DET)}
    assert tuple(cases) == PR.NMS_CASES
    for cname, kw in cases.items():
        out = ns.ops.non_max_suppression(pred.clone(), nc=1, max_time_img=1e9, **kw)
        n = [int(o.shape[0]) for o in out]
        print('nms', cname, kw, n)
        assert max(n) >= 5, (cname, n)
        if cname == 'few':
            assert max(n) < kw['max_det'], n
        arrs[f'{tag}_nms_{cname}_kw'] = np.array(json.dumps(kw))
        for i, o in enumerate(out):
            assert o.shape[1] == 6 + 51
            arrs[f'{tag}_nms_{cname}_{i}'] = o.numpy()
    arrs['predictor_args'] = np.array(json.dumps(dict(conf=cases['pred']['conf_thres'], iou=0.7, max_det=MAX_DET)))


def predictor_case(arrs, m):
    """predict.py:16-41 on the padded (no resize) letter-box of two BGR uint8 images."""
    args = json.loads(str(arrs['predictor_args']))
    imgs = PR.lb_images()
    x = np.full((2, 160, 224, 3), 114, np.uint8)
    for i, im in enumerate(imgs):
        x[i, 13:13 + PR.LB_SHAPE[0]] = im
    x = torch.from_numpy(np.ascontiguousarray(x[..., ::-1].transpose(0, 3, 1, 2))).float() / 255      # BGR -> RGB, HWC -> CHW, /255
    with torch.no_grad():
        pred, _ = m(x)
    rows = ns.ops.non_max_suppression(pred.clone(), args['conf'], args['iou'], agnostic=False, max_det=args['max_det'], classes=None, nc=1,
                                      max_time_img=1e9)
    oshape = (*PR.LB_SHAPE, 3)
    total = near = 0
    for i, r in enumerate(rows):
        r = r.clone()
        pre = ns.ops.scale_boxes((160, 224), r[:, :4].clone(), oshape)
        r[:, :4] = pre.round()
        k = r[:, 6:].view(len(r), 17, 3) if len(r) else r[:, 6:]
        k = ns.ops.scale_coords((160, 224), k.clone(), oshape)
        frac = (pre - torch.floor(pre) - 0.5).abs()
        risky = (frac <= ROUND_BAND).any(1)
        arrs[f'lb_{i}_boxes'] = r[:, :6].numpy()
        arrs[f'lb_{i}_preround'] = pre.numpy()
        arrs[f'lb_{i}_kpts'] = k.numpy()
        arrs[f'lb_{i}_risky'] = risky.numpy()
        total += len(r)
        near += int(risky.sum())
        print('predictor case', i, tuple(r.shape), 'rows near a .5 boundary', int(risky.sum()))
        assert len(r) >= 5
    assert near <= ROUND_CAP * total, (near, total)


def coords_cases(arrs):
    for name, oshape in PR.COORD_CASES.items():
        c = torch.from_numpy(PR.seeded_coords(name))
        out = ns.ops.scale_coords(PR.IN_SHAPE, c.clone(), oshape)
        arrs[f'coords_{name}'] = out.numpy()
        x, y = out[..., 0], out[..., 1]
        hit = int((x == 0).sum() + (x == oshape[1]).sum() + (y == 0).sum() + (y == oshape[0]).sum())
        print('scale_coords', name, oshape, 'clamped values', hit)
        assert hit > 20
        arrs[f'coords_{name}_norm'] = ns.ops.scale_coords(PR.IN_SHAPE, c.clone(), oshape, normalize=True).numpy()


def main():
    import torchvision  # the stand-in module from ref_import
    import yaml

    def nms_standin(boxes, scores, thr):
        assert bool((scores[:-1] >= scores[1:]).all()), 'reference hands nms() descending scores'
        return torch.from_numpy(onms.greedy_nms(boxes.numpy(), thr))

    torchvision.ops.nms = nms_standin
    with open(REFY + 'yolov8-pose.yaml', errors='ignore', encoding='utf-8') as f:
        d = yaml.safe_load(f)
    with open(os.path.join(HERE, 'pose_yaml.json'), 'w') as f:
        json.dump(d, f, indent=1)
        f.write('\n')
    arrs = {}
    with tempfile.TemporaryDirectory() as tmp:
        run_cases(arrs, tmp)
    coords_cases(arrs)
    save(arrs)


if __name__ == '__main__':
    main()
