"""Generate the YOLOv5 fixtures from the reference's own Python modules (BUILD CONTAINER ONLY).

    python tests/golden/gen_yolov5.py

Same recipe as gen_seg.py (ref_import, seeded weights and inputs re-created from seeds, CPU fp32).  Written:
  - yolov5_yaml.json: nc, scales, backbone, head of the reference's models/v5/yolov5.yaml, as data;
  - yolov5_NN.npz (tests/yolov5_ref.py:load_fixture merges them; each under 1 MiB):
      the reference's `C3` on the four cases of yolov5_ref.C3_CASES and `Conv(3, 16, 6, 2, 2)` on a float and on a uint8 / 255 image (BatchNorm eps 1e-3 as
      inside DetectionModel, seeded non-trivial running statistics);
      DetectionModel('yolov5n.yaml', nc=80), seed 0: state-dict keys / shapes, parameter count, stride; (y, feats) in full at 2x160x224 and 1x96x160, every
      25th anchor at 1x640x640; the fused model's y at 2x160x224;
      the bf16 emulation: the same model with its weights and every layer's output (each Conv / nn.Conv2d of the head, each row of the YAML) rounded to
      bfloat16 - its largest difference from its own fp32 run for boxes (px), confidences and head maps, per shape (`<key>_dbf16`);
  - train_yolov5_n.npz: the reference's `model.train()(batch); loss.backward()` on inputs.TRAIN_CASE, in the layout of train_yolov8_n.npz
    (gen_golden.py:train), so test_oracle_golden.check_train_fixture reads it unchanged.
The GPU box never runs this file.
"""
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
import yolov5_ref as YR  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()
REFY = '/root/reference/models/v5/'


def save(arrs, limit=900 * 1024):
    """Greedy shards yolov5_00.npz, yolov5_01.npz, ... of at most `limit` raw bytes, each checked against the 1 MiB limit of a committed file."""
    for old in glob.glob(os.path.join(HERE, 'yolov5_[0-9][0-9].npz')):
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
        path = os.path.join(HERE, f'yolov5_{n:02d}.npz')
        np.savez_compressed(path, **sh)
        sz = os.path.getsize(path)
        print(f'yolov5_{n:02d}: {len(sh)} arrays, {sz / 1024:.1f} KiB')
        assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def yaml_json():
    import yaml
    d = yaml.safe_load(open(REFY + 'yolov5.yaml'))
    with open(os.path.join(HERE, 'yolov5_yaml.json'), 'w') as f:
        json.dump({k: d[k] for k in ('nc', 'scales', 'backbone', 'head')}, f, indent=1)
        f.write('\n')


def _model_eps(mod):
    for sub in mod.modules():
        if isinstance(sub, nn.BatchNorm2d):
            sub.eps = 1e-3       # what initialize_weights does inside DetectionModel (torch_utils.py:254)
    return mod


def modules(arrs):
    import ultralytics.nn.modules.block as RB
    for name, (args, shape) in YR.C3_CASES.items():
        m = _model_eps(seed_state_dict_(RB.C3(*args), YR.MODULE_SEED)).eval()
        with torch.no_grad():
            arrs[f'{name}_y'] = m(YR.case_input(name, shape)).numpy()
        arrs[f'{name}_keys'] = np.array(list(m.state_dict().keys()))
    m = _model_eps(seed_state_dict_(ns.modules.Conv(*YR.STEM_ARGS), YR.MODULE_SEED)).eval()
    xf, xu = YR.stem_inputs()
    with torch.no_grad():
        arrs['stem_y_float'] = m(xf).numpy()
        arrs['stem_y_u8'] = m(xu.float() / 255).numpy()


def build(fuse=False, nc=80, seed=0):
    m = ns.tasks.DetectionModel(REFY + 'yolov5n.yaml', nc=nc, verbose=False)
    seed_state_dict_(m, seed)
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


def model(arrs):
    m = build()
    assert ns.tasks.guess_model_task(m) == 'detect'
    sd = m.state_dict()
    arrs['keys'] = np.array(list(sd.keys()))
    arrs['shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
    arrs['nparams'] = np.array(sum(p.numel() for p in m.parameters()), np.int64)
    arrs['stride'] = m.stride.numpy()
    mb = bf16_emulation(build())
    for shape, sub in YR.E2E_SHAPES.items():
        key = 'x'.join(map(str, shape))
        x = seeded_images(*shape, seed=YR.IMG_SEED)
        with torch.no_grad():
            y, feats = m(x)
            yb, fb = mb(x)
        arrs[f'{key}_anchors'] = np.array(y.shape[-1], np.int64)
        if sub == 1:
            arrs[f'{key}_y'] = y.numpy()
            for i, f in enumerate(feats):
                arrs[f'{key}_feat{i}'] = f.numpy()
        else:
            arrs[f'{key}_ysub'] = y[:, :, ::sub].numpy()
        d = [float((yb[:, :4] - y[:, :4]).abs().max()), float((yb[:, 4:] - y[:, 4:]).abs().max()), max(float((a - b).abs().max()) for a, b in zip(fb, feats))]
        arrs[f'{key}_dbf16'] = np.array(d, np.float64)
        print(key, tuple(y.shape), 'max conf', float(y[:, 4:].max()), 'bf16 emulation: box %.3e px, conf %.3e, head maps %.3e' % tuple(d))
    with torch.no_grad():
        yf, _ = build(fuse=True)(seeded_images(2, 160, 224, seed=YR.IMG_SEED))
    arrs['2x160x224_yfused'] = yf.numpy()


def train():
    """gen_golden.py:train for the yolov5n graph (trainer.py:334-343 on the CPU)."""
    from inputs import TRAIN_CASE, grad_sample, train_inputs
    c = TRAIN_CASE
    x, lab = train_inputs()
    m = build(nc=c['nc'], seed=c['weight_seed']).train()
    batch = dict(img=x.clone(), **{k: v.clone() for k, v in lab.items()})
    feats = []
    hk = m.model[-1].register_forward_hook(lambda mod, i, o: feats.extend(o))
    loss, items = m(batch)
    hk.remove()
    loss.backward()
    arrs = {'loss': loss.detach().numpy(), 'items': items.numpy(), 'stride': m.stride.numpy()}
    for i, f in enumerate(feats):
        arrs[f'feat{i}'] = f.detach().numpy()
    names, nograd = [], []
    for k, p in m.named_parameters():
        if p.grad is None:
            nograd.append(k)
            continue
        names.append(k)
        arrs['g/' + k], arrs['gst/' + k] = grad_sample(p.grad)
    arrs['grad_names'] = '\n'.join(names)
    arrs['nograd_names'] = '\n'.join(nograd)
    for k, b in m.named_buffers():
        if 'running_' in k or 'num_batches_tracked' in k:
            arrs['bn/' + k] = b.detach().numpy()
    print('train yolov5_n', float(loss), items.tolist(), len(names), 'gradients;', 'no grad:', nograd)
    path = os.path.join(HERE, 'train_yolov5_n.npz')
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    sz = os.path.getsize(path)
    print(f'train_yolov5_n: {sz / 1024:.1f} KiB')
    assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def main():
    yaml_json()
    arrs = {}
    modules(arrs)
    model(arrs)
    save(arrs)
    train()


if __name__ == '__main__':
    main()
