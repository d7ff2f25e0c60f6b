"""Generate the YOLOv3 fixtures from the reference's own Python modules (BUILD CONTAINER ONLY).

    python tests/golden/gen_yolov3.py

Same recipe as gen_yolov6.py (ref_import, seeded weights and inputs re-created from seeds, CPU fp32): the fixtures hold outputs only.  Written:
  - yolov3_yaml.json: nc, depth_multiple, width_multiple, backbone, head of the reference's models/v3/{yolov3,yolov3-spp,yolov3-tiny}.yaml, as data;
  - yolov3_NN.npz (tests/yolov3_ref.py:load_fixture merges them; each under 1 MiB), keys `<tag>/<quantity>` for the tags of yolov3_ref.GRAPHS:
      `tiny` = yolov3-tiny at full width, `v3_w025` / `spp_w025` = yolov3 / yolov3-spp built from the same rows with width_multiple 0.25 (both parsers
      read that key), nc = 80: state-dict keys / shapes, parameter count, stride; (y, feats) in full at 2x64x96 and 1x96x160; the fused model's y at
      2x64x96; `seed` and `gain` of the weights (yolov6_ref.seed_model_): the gain is lowered until every row's output rms stays inside
      yolov3_ref.RMS_RANGE, the seed walks until no decisive class score sits within SCORE_MARGIN (relative) of a confidence threshold of NMS_SETTINGS;
      per shape `<key>_d64`: the reference's own fp32 run against its float64 run (boxes px, confidences, head maps), and `<key>_dbf16`: against the
      same model with its weights and every layer's output rounded to bfloat16;
      `spp_full` = yolov3-spp at full width: keys / shapes, parameter count, stride and one fp32 y at 1x64x64 (weights: spp_w025's seed and gain);
      `v3_full` = yolov3 at full width: keys / shapes, parameter count and stride only;
  - train_yolov3_tiny.npz, train_yolov3_spp_w025.npz: the reference's `model.train()(batch); loss.backward()` on inputs.TRAIN_CASE in the layout of
    train_yolov6_n.npz (loss, items, head maps, sampled gradients with norm and sum, running statistics, `weight_seed` / `gain`, `d64`, `gd64/<name>`,
    `d64_run`, `dbf16`, `cbf16/<name>`); the weight seed walks until the float64 run takes the same assigner decisions.  On disk the per-tensor scalars
    (`gst/`, `gd64/`, `cbf16/`) are one array each in the order of `grad_names` (yolov3_ref.pack_train; 267 tensors x 4 zip entries would put the file
    over 1 MiB); yolov3_ref.load_train gives the per-name layout back.
The GPU box never runs this file.
"""
import copy
import glob
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_import  # noqa: E402
import yolov3_ref as Y3  # noqa: E402
from mgdt_yolo_amd.seeding import seeded_images  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()
REFY = '/root/reference/models/v3/'
YAML_KEYS = ('nc', 'depth_multiple', 'width_multiple', 'backbone', 'head')


def ref_yaml(name):
    import yaml
    with open(REFY + name + '.yaml') as f:
        return yaml.safe_load(f)


def save(arrs, limit=900 * 1024):
    for old in glob.glob(os.path.join(HERE, 'yolov3_[0-9][0-9].npz')):
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
        path = os.path.join(HERE, f'yolov3_{n:02d}.npz')
        np.savez_compressed(path, **sh)
        sz = os.path.getsize(path)
        print(f'yolov3_{n:02d}: {len(sh)} arrays, {sz / 1024:.1f} KiB')
        assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def yaml_json():
    with open(os.path.join(HERE, 'yolov3_yaml.json'), 'w') as f:
        json.dump({n: {k: ref_yaml(n)[k] for k in YAML_KEYS} for n in Y3.NAMES}, f, indent=1)
        f.write('\n')


def build(name, width, seed, gain, fuse=False, nc=80):
    d = ref_yaml(name)
    d['width_multiple'] = width
    m = ns.tasks.DetectionModel(d, nc=nc, verbose=False)
    assert all(isinstance(c.act, nn.SiLU) for c in m.modules() if isinstance(c, ns.modules.Conv))
    Y3.seed_model_(m, seed, gain)
    m.args = types.SimpleNamespace(box=7.5, cls=0.5, dfl=1.5)
    return (m.fuse(verbose=False) if fuse else m).eval()


def bf16_emulation(m):
    """the model with every weight and every layer output rounded to bfloat16 (fp32 arithmetic in between): the precision class of the bf16 route"""
    rb = lambda t: t.to(torch.bfloat16).float()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(rb(p))
    hook = lambda mod, i, o: rb(o) if torch.is_tensor(o) else None
    for mod in m.modules():
        if isinstance(mod, (ns.modules.Conv, nn.Conv2d)) or mod in list(m.model)[:-1]:
            if not (isinstance(mod, nn.Conv2d) and mod.weight.requires_grad is False):       # the DFL expectation stays fp32 (it is part of the decode)
                mod.register_forward_hook(hook)
    return m


def stage_rms(m, x):
    out = []
    hooks = [mod.register_forward_hook(lambda mod, i, o: out.append(float(o.pow(2).mean().sqrt()))) for mod in list(m.model)[:-1]]
    with torch.no_grad():
        m(x)
    for h in hooks:
        h.remove()
    return out


def pick_gain(name, width):
    x = seeded_images(*Y3.E2E_SHAPES[1], seed=Y3.IMG_SEED)
    for gain in (1.0, 0.95, 0.9, 0.85, 0.8, 0.75, 0.7):
        rms = stage_rms(build(name, width, 0, gain), x)
        print(f'{name} w{width} gain {gain}: row output rms ' + ' '.join(f'{v:.3g}' for v in rms))
        if Y3.RMS_RANGE[0] <= min(rms) and max(rms) <= Y3.RMS_RANGE[1]:
            return gain
    raise SystemExit('no gain keeps the seeded graph inside RMS_RANGE')


def score_margin(y):
    s = y[:, 4:].double()
    best = s.amax(1)
    return min(float((((s if kw.get('multi_label') else best) - kw['conf_thres']).abs() / kw['conf_thres']).min()) for kw in Y3.NMS_SETTINGS)


def describe(arrs, tag, m):
    sd = m.state_dict()
    arrs[f'{tag}/keys'] = np.array(list(sd.keys()))
    arrs[f'{tag}/shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
    arrs[f'{tag}/nparams'] = np.array(sum(p.numel() for p in m.parameters()), np.int64)
    arrs[f'{tag}/stride'] = m.stride.numpy()


def model(arrs, tag, name, width, gain):
    xs = {shape: seeded_images(*shape, seed=Y3.IMG_SEED) for shape in Y3.E2E_SHAPES}
    for seed in range(64):
        m = build(name, width, seed, gain)
        with torch.no_grad():
            margin = min(score_margin(m(x)[0]) for x in xs.values())
        print(f'{tag} seed {seed}: closest decisive class score to its confidence threshold, relative: {margin:.3e}')
        if margin > Y3.SCORE_MARGIN:
            break
    else:
        raise SystemExit('no seed keeps the class scores away from the NMS thresholds')
    assert ns.tasks.guess_model_task(m) == 'detect'
    describe(arrs, tag, m)
    arrs[f'{tag}/seed'], arrs[f'{tag}/gain'] = np.array(seed, np.int64), np.array(gain, np.float64)
    arrs[f'{tag}/score_margin'] = np.array(margin, np.float64)
    m64 = copy.deepcopy(m).double()
    mb = bf16_emulation(build(name, width, seed, gain))
    for shape, x in xs.items():
        key = f'{tag}/' + 'x'.join(map(str, shape))
        with torch.no_grad():
            y, feats = m(x)
            y64, f64 = m64(x.double())
            yb, fb = mb(x)
        arrs[f'{key}_anchors'] = np.array(y.shape[-1], np.int64)
        arrs[f'{key}_y'] = y.numpy()
        for i, f in enumerate(feats):
            arrs[f'{key}_feat{i}'] = f.numpy()
        diff = lambda ya, fa: [float((ya[:, :4] - y[:, :4]).abs().max()), float((ya[:, 4:] - y[:, 4:]).abs().max()),
                               max(float((a - b).abs().max()) for a, b in zip(fa, feats))]
        arrs[f'{key}_d64'] = np.array(diff(y64, f64), np.float64)
        arrs[f'{key}_dbf16'] = np.array(diff(yb, fb), np.float64)
        print(key, tuple(y.shape), 'max conf', float(y[:, 4:].max()), 'head map rms', [float(f.pow(2).mean().sqrt()) for f in feats])
        print('   fp32 vs float64: box %.3e px, conf %.3e, head maps %.3e' % tuple(arrs[f'{key}_d64']),
              '-> 4 x that against the contract (1e-3, 1e-4, 1e-3):', ['4 x d64 binds' if 4 * d > c else 'contract binds' for d, c in zip(arrs[f'{key}_d64'], (1e-3, 1e-4, 1e-3))])
        print('   bf16 emulation:  box %.3e px, conf %.3e, head maps %.3e' % tuple(arrs[f'{key}_dbf16']))
    with torch.no_grad():
        yf, _ = build(name, width, seed, gain, fuse=True)(xs[Y3.E2E_SHAPES[0]])
    arrs[f'{tag}/2x64x96_yfused'] = yf.numpy()
    return seed


def full_width(arrs, seed, gain):
    describe(arrs, 'v3_full', build('yolov3', 1.0, seed, gain))            # structure only: full yolov3 is a row subset of full yolov3-spp
    tag, name, width = Y3.FULL
    m = build(name, width, seed, gain)
    describe(arrs, tag, m)
    arrs[f'{tag}/seed'], arrs[f'{tag}/gain'] = np.array(seed, np.int64), np.array(gain, np.float64)
    with torch.no_grad():
        y, _ = m(seeded_images(*Y3.FULL_SHAPE, seed=Y3.IMG_SEED))
    arrs[f'{tag}/' + 'x'.join(map(str, Y3.FULL_SHAPE)) + '_y'] = y.numpy()
    print(tag, int(arrs[f'{tag}/nparams']), 'parameters, y', tuple(y.shape), 'max conf', float(y[:, 4:].max()))


def train_step(m, x, lab):
    """(loss, items, feats, assigner decisions) of one reference training step; gradients are left on the parameters"""
    batch = dict(img=x.clone(), **{k: v.clone() for k, v in lab.items()})
    feats, decisions = [], []
    hk = m.model[-1].register_forward_hook(lambda mod, i, o: feats.extend(o))
    Assigner = ns.tal.TaskAlignedAssigner
    orig = Assigner.forward

    def recording(self, *a, **k):
        out = orig(self, *a, **k)
        decisions.append((out[3].clone(), out[4].clone()))       # fg_mask, target_gt_idx
        return out
    Assigner.forward = recording
    try:
        loss, items = m(batch)
    finally:
        Assigner.forward = orig
        hk.remove()
    loss.backward()
    return loss, items, feats, decisions


def train(tag, name, width, gain):
    """gen_yolov6.py:train for one YOLOv3 graph (trainer.py:334-343 on the CPU)."""
    from inputs import TRAIN_CASE, grad_sample, train_inputs
    c = TRAIN_CASE
    x, lab = train_inputs()
    for seed in range(c['weight_seed'], c['weight_seed'] + 64):
        m = build(name, width, seed, gain, nc=c['nc']).train()
        m64 = copy.deepcopy(m).double()
        loss, items, feats, dec = train_step(m, x, lab)
        loss64, _, feats64, dec64 = train_step(m64, x.double(), {k: (v.double() if k == 'bboxes' else v) for k, v in lab.items()})
        same = all(torch.equal(a[0], b[0]) and torch.equal(a[1][a[0].bool()], b[1][b[0].bool()]) for a, b in zip(dec, dec64))
        fg = dec[0][0].bool()
        ngt = int(lab['cls'].shape[0])
        print(f'train {tag} seed {seed}: loss {float(loss):.6f} (float64 {float(loss64):.6f}), {int(fg.sum())} foreground anchors of {fg.numel()}, '
              f'{ngt} ground truths, assigner decisions {"equal" if same else "DIFFER"} in float64')
        if same and int(fg.sum()) > 0:
            break
    else:
        raise SystemExit('no seed gives the same assigner decisions in fp32 and float64')
    arrs = {'loss': loss.detach().numpy(), 'items': items.numpy(), 'stride': m.stride.numpy(), 'weight_seed': np.array(seed, np.int64),
            'gain': np.array(gain, np.float64), 'foreground': np.array(int(fg.sum()), np.int64)}
    for i, f in enumerate(feats):
        arrs[f'feat{i}'] = f.detach().numpy()
    names, nograd, gerr = [], [], 0.0
    p64 = dict(m64.named_parameters())
    for k, p in m.named_parameters():
        if p.grad is None:
            nograd.append(k)
            continue
        names.append(k)
        arrs['g/' + k], arrs['gst/' + k] = grad_sample(p.grad)
        g64 = p64[k].grad
        arrs['gd64/' + k] = np.array(float((p.grad.double() - g64).pow(2).mean().sqrt()), np.float64)      # rms of fp32 - float64 over the whole tensor
        gerr = max(gerr, float((p.grad.double() - g64).pow(2).mean().sqrt() / max(float(g64.pow(2).mean().sqrt()), 1e-30)))
    arrs['grad_names'] = '\n'.join(names)
    arrs['nograd_names'] = '\n'.join(nograd)
    arrs['d64'] = np.array([abs(float(loss) - float(loss64)) / float(loss64), max(float((a.double() - b).abs().max()) for a, b in zip(feats, feats64)), gerr])
    b64, rerr = dict(m64.named_buffers()), 0.0
    for k, b in m.named_buffers():
        if 'running_' in k or 'num_batches_tracked' in k:
            arrs['bn/' + k] = b.detach().numpy()
        if 'running_' in k:
            rerr = max(rerr, float(((b.double() - b64[k]).abs() / (1 + b64[k].abs())).max()))
    arrs['d64_run'] = np.array(rerr, np.float64)
    print(f'train {tag}', float(loss), items.tolist(), len(names), 'gradients;', 'no grad:', nograd)
    print('   fp32 vs float64: loss rel %.3e, head maps %.3e, worst gradient %.3e of its rms' % tuple(arrs['d64']), 'running statistics %.3e' % rerr)
    mb = bf16_emulation(build(name, width, seed, gain, nc=c['nc'])).train()
    lossb, _, featsb, _ = train_step(mb, x, lab)
    runb = {k[:-len('.running_mean')]: (b.numpy(), dict(mb.named_buffers())[k[:-len('running_mean')] + 'running_var'].numpy())
            for k, b in mb.named_buffers() if k.endswith('running_mean')}
    fig = Y3.train_figures({k: np.asarray(v) for k, v in arrs.items()}, float(lossb), [f.detach().numpy() for f in featsb],
                           {k: p.grad for k, p in mb.named_parameters() if p.grad is not None}, runb)
    arrs['dbf16'] = np.array([fig[k] for k in Y3.TRAIN_FIGURES], np.float64)
    for k, cbf in fig['per'].items():
        arrs['cbf16/' + k] = np.array(cbf, np.float64)
    print(f"   bf16 emulation: {sum(v >= Y3.INFORMATIVE_COS for v in fig['per'].values())} of {len(fig['per'])} gradient tensors keep cosine >= {Y3.INFORMATIVE_COS}")
    print('   bf16 emulation vs fp32:', {k: fig[k] for k in Y3.TRAIN_FIGURES})
    path = os.path.join(HERE, Y3.TRAIN[tag] + '.npz')
    np.savez_compressed(path, **Y3.pack_train({k: np.asarray(v) for k, v in arrs.items()}))
    sz = os.path.getsize(path)
    print(f'{Y3.TRAIN[tag]}: {sz / 1024:.1f} KiB')
    assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def main():
    yaml_json()
    arrs, picked = {}, {}
    for tag, (name, width) in Y3.GRAPHS.items():
        gain = pick_gain(name, width)
        picked[tag] = (model(arrs, tag, name, width, gain), gain)
    full_width(arrs, *picked['spp_w025'])
    save(arrs)
    for tag in Y3.TRAIN:
        train(tag, *Y3.GRAPHS[tag], picked[tag][1])


if __name__ == '__main__':
    main()
