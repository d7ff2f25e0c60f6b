"""Generate the YOLOv6 fixtures from the reference's own Python modules (BUILD CONTAINER ONLY).

    python tests/golden/gen_yolov6.py

Same recipe as gen_yolov5.py (ref_import, seeded weights and inputs re-created from seeds, CPU fp32): the fixtures hold outputs only.  Written:
  - yolov6_yaml.json: nc, activation, scales, backbone, head of the reference's models/v6/yolov6.yaml, as data;
  - yolov6_NN.npz (tests/yolov6_ref.py:load_fixture merges them; each under 1 MiB):
      DetectionModel('yolov6n.yaml', nc=80): state-dict keys / shapes, parameter count, stride; (y, feats) in full at 2x64x96 and 1x96x160; the fused
      model's y at 2x64x96; `seed` and `gain` of the weights (yolov6_ref.seed_model_): the gain is lowered until every row's output rms of the seeded
      ReLU chain stays inside yolov6_ref.RMS_RANGE, the seed walks until no decisive class score (an anchor's best class score for the single-label
      settings of yolov6_ref.NMS_SETTINGS, every class score for the multi_label one) sits within yolov6_ref.SCORE_MARGIN (relative) of its
      confidence threshold;
      per shape `<key>_d64`: the reference's own fp32 run against its float64 run (boxes px, confidences, head maps), and `<key>_dbf16`: against the
      same model with its weights and every layer's output rounded to bfloat16;
  - train_yolov6_n.npz: the reference's `model.train()(batch); loss.backward()` on inputs.TRAIN_CASE, in the layout of train_yolov8_n.npz, plus
    `weight_seed` / `gain` (the seed walks until the float64 run of the same step takes the same assigner decisions: foreground mask and assigned
    ground truths) and, of fp32 against float64: `d64` = [relative loss difference, head maps, worst gradient difference in units of the tensor's rms],
    `gd64/<name>` = the rms of the difference per gradient tensor, `d64_run` = the largest |difference| / (1 + |value|) of a running statistic; and
    `dbf16` = yolov6_ref.train_figures of the same step with the weights and every layer's output rounded to bfloat16 against the fp32 step, and
    `cbf16/<name>` = that emulation's cosine with the fp32 step per gradient tensor.
The reference leaks `activation:` into Conv.default_act for the rest of the process; this file restores it after every build.
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
import yolov6_ref as YR  # noqa: E402
from mgdt_yolo_amd.seeding import seeded_images  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()
REFY = '/root/reference/models/v6/'


def save(arrs, limit=900 * 1024):
    for old in glob.glob(os.path.join(HERE, 'yolov6_[0-9][0-9].npz')):
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
        path = os.path.join(HERE, f'yolov6_{n:02d}.npz')
        np.savez_compressed(path, **sh)
        sz = os.path.getsize(path)
        print(f'yolov6_{n:02d}: {len(sh)} arrays, {sz / 1024:.1f} KiB')
        assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def yaml_json():
    import yaml
    d = yaml.safe_load(open(REFY + 'yolov6.yaml'))
    with open(os.path.join(HERE, 'yolov6_yaml.json'), 'w') as f:
        json.dump({k: d[k] for k in ('nc', 'activation', 'scales', 'backbone', 'head')}, f, indent=1)
        f.write('\n')


def build(seed, gain, fuse=False, nc=80):
    RefConv = ns.modules.Conv
    prev = RefConv.default_act
    try:
        m = ns.tasks.DetectionModel(REFY + 'yolov6n.yaml', nc=nc, verbose=False)
    finally:
        RefConv.default_act = prev           # the reference leaves nn.ReLU() here for every later build
    assert isinstance(RefConv.default_act, nn.SiLU)
    assert all(isinstance(c.act, nn.ReLU) for c in m.modules() if isinstance(c, RefConv))
    YR.seed_model_(m, seed, gain)
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


def pick_gain():
    x = seeded_images(*YR.E2E_SHAPES[1], seed=YR.IMG_SEED)
    for gain in (1.0, 0.95, 0.9, 0.85, 0.8, 0.75, 0.7):
        rms = stage_rms(build(0, gain), x)
        print(f'gain {gain}: row output rms ' + ' '.join(f'{v:.3g}' for v in rms))
        if YR.RMS_RANGE[0] <= min(rms) and max(rms) <= YR.RMS_RANGE[1]:
            return gain
    raise SystemExit('no gain keeps the seeded ReLU chain inside RMS_RANGE')


def score_margin(y):
    """closest decisive score to its confidence threshold, relative to the threshold, over YR.NMS_SETTINGS: an anchor's best class score for the
    single-label settings (the candidate test of non_max_suppression), every class score for the multi_label one"""
    s = y[:, 4:].double()
    best = s.amax(1)
    return min(float((((s if kw.get('multi_label') else best) - kw['conf_thres']).abs() / kw['conf_thres']).min()) for kw in YR.NMS_SETTINGS)


def model(arrs, gain):
    xs = {shape: seeded_images(*shape, seed=YR.IMG_SEED) for shape in YR.E2E_SHAPES}
    for seed in range(64):
        m = build(seed, gain)
        with torch.no_grad():
            margin = min(score_margin(m(x)[0]) for x in xs.values())
        print(f'seed {seed}: closest decisive class score to its confidence threshold, relative: {margin:.3e}')
        if margin > YR.SCORE_MARGIN:
            break
    else:
        raise SystemExit('no seed keeps the class scores away from the NMS thresholds')
    assert ns.tasks.guess_model_task(m) == 'detect'
    sd = m.state_dict()
    arrs['seed'], arrs['gain'] = np.array(seed, np.int64), np.array(gain, np.float64)
    arrs['score_margin'] = np.array(margin, np.float64)
    arrs['keys'] = np.array(list(sd.keys()))
    arrs['shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
    arrs['nparams'] = np.array(sum(p.numel() for p in m.parameters()), np.int64)
    arrs['stride'] = m.stride.numpy()
    m64 = copy.deepcopy(m).double()
    mb = bf16_emulation(build(seed, gain))
    for shape, x in xs.items():
        key = 'x'.join(map(str, shape))
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
        print('   fp32 vs float64: box %.3e px, conf %.3e, head maps %.3e' % tuple(arrs[f'{key}_d64']))
        print('   bf16 emulation:  box %.3e px, conf %.3e, head maps %.3e' % tuple(arrs[f'{key}_dbf16']))
    with torch.no_grad():
        yf, _ = build(seed, gain, fuse=True)(xs[YR.E2E_SHAPES[0]])
    arrs['2x64x96_yfused'] = yf.numpy()


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


def train(gain):
    """gen_golden.py:train for the yolov6n graph (trainer.py:334-343 on the CPU)."""
    from inputs import TRAIN_CASE, grad_sample, train_inputs
    c = TRAIN_CASE
    x, lab = train_inputs()
    for seed in range(c['weight_seed'], c['weight_seed'] + 64):
        m = build(seed, gain, nc=c['nc']).train()
        m64 = copy.deepcopy(m).double()
        loss, items, feats, dec = train_step(m, x, lab)
        loss64, _, feats64, dec64 = train_step(m64, x.double(), {k: (v.double() if k == 'bboxes' else v) for k, v in lab.items()})
        same = all(torch.equal(a[0], b[0]) and torch.equal(a[1][a[0].bool()], b[1][b[0].bool()]) for a, b in zip(dec, dec64))
        print(f'train seed {seed}: loss {float(loss):.6f} (float64 {float(loss64):.6f}), {int(dec[0][0].sum())} foreground anchors, '
              f'assigner decisions {"equal" if same else "DIFFER"} in float64')
        if same:
            break
    else:
        raise SystemExit('no seed gives the same assigner decisions in fp32 and float64')
    arrs = {'loss': loss.detach().numpy(), 'items': items.numpy(), 'stride': m.stride.numpy(), 'weight_seed': np.array(seed, np.int64),
            'gain': np.array(gain, np.float64)}
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
    print('train yolov6_n', float(loss), items.tolist(), len(names), 'gradients;', 'no grad:', nograd)
    print('   fp32 vs float64: loss rel %.3e, head maps %.3e, worst gradient %.3e of its rms' % tuple(arrs['d64']), 'running statistics %.3e' % rerr)
    # the same step with the weights and every layer's output rounded to bfloat16 (and, through the casts' backward, the gradients that flow back through
    # them): how far the reference itself moves from its fp32 step in the precision class of the bf16 route, in the figures the bf16 test asserts
    mb = bf16_emulation(build(seed, gain, nc=c['nc'])).train()
    lossb, _, featsb, _ = train_step(mb, x, lab)
    runb = {k[:-len('.running_mean')]: (b.numpy(), dict(mb.named_buffers())[k[:-len('running_mean')] + 'running_var'].numpy())
            for k, b in mb.named_buffers() if k.endswith('running_mean')}
    fig = YR.train_figures({k: np.asarray(v) for k, v in arrs.items()}, float(lossb), [f.detach().numpy() for f in featsb],
                           {k: p.grad for k, p in mb.named_parameters() if p.grad is not None}, runb)
    arrs['dbf16'] = np.array([fig[k] for k in YR.TRAIN_FIGURES], np.float64)
    for k, cbf in fig['per'].items():
        arrs['cbf16/' + k] = np.array(cbf, np.float64)
    print(f"   bf16 emulation: {sum(v >= YR.INFORMATIVE_COS for v in fig['per'].values())} of {len(fig['per'])} gradient tensors keep cosine >= {YR.INFORMATIVE_COS}")
    print('   bf16 emulation vs fp32:', {k: fig[k] for k in YR.TRAIN_FIGURES})
    path = os.path.join(HERE, 'train_yolov6_n.npz')
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    sz = os.path.getsize(path)
    print(f'train_yolov6_n: {sz / 1024:.1f} KiB')
    assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def main():
    yaml_json()
    gain = pick_gain()
    arrs = {}
    model(arrs, gain)
    save(arrs)
    train(gain)


if __name__ == '__main__':
    main()
