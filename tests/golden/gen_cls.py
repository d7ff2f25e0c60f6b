"""Generate tests/golden/cls_NN.npz and tests/golden/cls_yaml.json: classification fixtures from the reference's own Python modules (BUILD CONTAINER
ONLY).

    python tests/golden/gen_cls.py

Same recipe as gen_pose.py (ref_import, seeded weights (cls_ref.seed_cls_) and images, CPU fp32).  Recorded:
  - cls_yaml.json: the reference's models/v8/yolov8-cls.yaml parsed to a dict (a settings fixture);
  - ClassificationModel('yolov8-cls') at scales n and s, nc = 10: state-dict keys / shapes and the parameter count;
  - for the cases of tests/cls_ref.py:CASES (scale n): eval probabilities and train-mode logits (batch-statistics BatchNorm, on a copy); the same
    from the .double() model with the largest fp32-vs-fp64 difference per quantity; the largest difference to a bf16 EMULATION (every parameter and
    the input rounded to bf16, the output of every Conv and of the linear rounded to bf16 by forward hooks); the smallest top-1 / top-2 gap;
  - for cls_ref.TRAIN_CASES one reference training step (model.train(), v8ClassificationLoss through model(batch), backward()): loss, BatchNorm
    running statistics, every parameter gradient as (sample, [l2 norm, sum]) - the head's (layer 9) whole, its conv weight in two halves - and the
    per-tensor difference of the same step in float64, relative to the tensor's rms;
  - ClassifyMetrics.process and ConfusionMatrix.process_cls_preds on seeded predictions.
Asserted here (seeds are chosen so that they hold): the top-1 / top-2 gap of every fixture image is at least 2 x the bf16 bound (3 x the emulation
difference); the folded shift of Classify.conv has a mean magnitude in [0.5, 2]; no ties among the best n5 + 1 probabilities.
The GPU box never runs this file.
"""
import copy
import glob
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import cls_ref as CR  # noqa: E402
import ref_import  # noqa: E402
from mgdt_yolo_amd.seeding import seeded_images  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()
REFY = '/root/reference/models/v8/'


def save(arrs, limit=900 * 1024):
    for old in glob.glob(os.path.join(HERE, 'cls_[0-9][0-9].npz')):
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
        path = os.path.join(HERE, f'cls_{n:02d}.npz')
        np.savez_compressed(path, **sh)
        sz = os.path.getsize(path)
        print(f'cls_{n:02d}: {len(sh)} arrays, {sz / 1024:.1f} KiB')
        assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def build(scale, nc):
    m = ns.tasks.ClassificationModel(REFY + f'yolov8{scale}-cls.yaml', nc=nc, verbose=False)
    return CR.seed_cls_(m, CR.WEIGHT_SEED).eval()


def structure(arrs, tag, m):
    sd = m.state_dict()
    arrs[f'{tag}_keys'] = np.array(list(sd.keys()))
    arrs[f'{tag}_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
    arrs[f'{tag}_nparams'] = np.array(sum(p.numel() for p in m.parameters()), np.int64)
    assert ns.tasks.guess_model_task(m) == 'classify'


def bf16_emulation(m):
    e = copy.deepcopy(m)
    with torch.no_grad():
        for p in e.parameters():
            p.copy_(CR.bf16r(p))
    for mod in e.modules():
        if isinstance(mod, (ns.modules.Conv, nn.Linear)):
            mod.register_forward_hook(lambda _m, _i, o: CR.bf16r(o))
    return e


def train_logits(m, x):
    t = copy.deepcopy(m).train()
    with torch.no_grad():
        return t(x)


def run_cases(arrs):
    for tag, (nc, shape) in CR.CASES.items():
        m = build('n', nc)
        head = m.model[-1]
        bn = head.conv.bn
        shift = bn.bias - bn.weight * bn.running_mean / torch.sqrt(bn.running_var + bn.eps)
        assert 0.5 < float(shift.detach().abs().mean()) < 2.0, float(shift.detach().abs().mean())
        x = seeded_images(*shape, seed=CR.IMG_SEED)
        with torch.no_grad():
            p = m(x)
            lg = train_logits(m, x)
            m64 = copy.deepcopy(m).double()
            p64 = m64(x.double())
            lg64 = train_logits(m64, x.double())
            e = bf16_emulation(m)
            pb = e(CR.bf16r(x))
        assert tuple(p.shape) == (shape[0], nc) and p64.dtype == torch.float64
        d64 = np.array([float((p.double() - p64).abs().max()), float((lg.double() - lg64).abs().max())])
        db = float((p - pb).abs().max())
        srt = torch.sort(p, 1, descending=True).values
        n5 = min(nc, 5)
        gap = float((srt[:, 0] - srt[:, 1]).min())
        ties = int((srt[:, :min(nc, n5 + 1) - 1] == srt[:, 1:min(nc, n5 + 1)]).sum())
        print(f'{tag}: probs max {float(p.max()):.4f} top1-top2 gap {gap:.4e}  fp32-vs-fp64 probs {d64[0]:.3e} logits {d64[1]:.3e}  bf16 emulation {db:.3e} '
              f'(bound {3 * db:.3e})  |logits| max {float(lg.abs().max()):.2f}')
        assert gap >= 2 * 3 * db, (tag, gap, db)
        assert ties == 0, tag
        assert bool((p.argmax(1) == pb.argmax(1)).all())
        arrs[f'{tag}_probs'] = p.numpy()
        arrs[f'{tag}_logits_train'] = lg.numpy()
        arrs[f'{tag}_probs64'] = p64.numpy()
        arrs[f'{tag}_d64'] = d64
        arrs[f'{tag}_dbf16'] = np.array(db)
        arrs[f'{tag}_gap'] = np.array(gap)


def train_step(arrs, tag):
    nc, shape = CR.CASES[tag]
    x = seeded_images(*shape, seed=CR.IMG_SEED)
    cls = CR.seeded_labels(shape[0], nc)
    out = {}
    for dt in (torch.float32, torch.float64):
        m = build('n', nc).to(dt).train()
        loss, item = m({'img': x.to(dt), 'cls': cls})
        loss.backward()
        out[dt] = (m, float(loss))
    m, loss = out[torch.float32]
    m64, loss64 = out[torch.float64]
    arrs[f'train_{tag}/loss'] = np.array(loss, np.float64)
    arrs[f'train_{tag}/loss64'] = np.array(loss64, np.float64)
    arrs[f'train_{tag}/cls'] = cls.numpy()
    names, worst = [], (0.0, None)
    g64 = dict(m64.named_parameters())
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        names.append(k)
        g = p.grad
        rms = float(g.double().pow(2).mean().sqrt())
        d = float((g.double() - g64[k].grad).pow(2).mean().sqrt()) / max(rms, 1e-30)
        arrs[f'train_{tag}/gd64/{k}'] = np.array(d)
        if d > worst[0]:
            worst = (d, k)
        if k.startswith('model.9.'):
            st = np.array([g.double().norm().item(), g.double().sum().item()])
            if g.numel() * 4 > 800 * 1024:
                half = g.shape[0] // 2
                arrs[f'train_{tag}/gfull0/{k}'] = g[:half].numpy()
                arrs[f'train_{tag}/gfull1/{k}'] = g[half:].numpy()
            else:
                arrs[f'train_{tag}/gfull/{k}'] = g.numpy()
            arrs[f'train_{tag}/gst/{k}'] = st
        else:
            arrs[f'train_{tag}/g/{k}'], arrs[f'train_{tag}/gst/{k}'] = CR.grad_sample(g)
    arrs[f'train_{tag}/grad_names'] = np.array('\n'.join(names))
    for k, b in m.named_buffers():
        if k.endswith('running_mean') or k.endswith('running_var'):
            arrs[f'train_{tag}/bn/{k}'] = b.numpy()
    print(f'train {tag}: loss {loss:.6f} (fp64 {loss64:.6f}); worst fp32-vs-fp64 gradient difference {worst[0]:.3e} of the rms ({worst[1]})')


def metric_case(arrs):
    c = CR.METRIC_CASE
    p = CR.topk_probs(c['n'], c['nc'], c['seed'])
    t = CR.seeded_labels(c['n'], c['nc'], seed=c['seed'])
    n5 = min(c['nc'], 5)
    pred = p.argsort(1, descending=True)[:, :n5]
    met = ns.metrics.ClassifyMetrics()
    met.process([t], [pred])
    cm = ns.metrics.ConfusionMatrix(nc=c['nc'], task='classify')
    cm.process_cls_preds([pred], [t])
    arrs['metric_pred'] = pred.numpy()
    arrs['metric_top'] = np.array([met.top1, met.top5], np.float64)
    arrs['metric_matrix'] = cm.matrix.astype(np.int64)
    arrs['metric_keys'] = np.array(met.keys)
    print('metrics', met.results_dict)
    assert 0 < met.top1 < met.top5 < 1


def main():
    import yaml
    with open(REFY + 'yolov8-cls.yaml', errors='ignore', encoding='utf-8') as f:
        d = yaml.safe_load(f)
    with open(os.path.join(HERE, 'cls_yaml.json'), 'w') as f:
        json.dump(d, f, indent=1)
        f.write('\n')
    arrs = {}
    structure(arrs, 'yolov8_cls_n', build('n', 10))
    structure(arrs, 'yolov8_cls_s', build('s', 10))
    run_cases(arrs)
    for tag in CR.TRAIN_CASES:
        train_step(arrs, tag)
    metric_case(arrs)
    save(arrs)


if __name__ == '__main__':
    main()
