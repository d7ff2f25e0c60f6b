"""Generate tests/golden/optim_traj.npz from the reference's own build_optimizer / one_cycle / ModelEMA (BUILD CONTAINER ONLY).

    python tests/golden/gen_optim.py

Like gen_golden.py:optim_groups, BaseTrainer.build_optimizer is taken out of the class with `ast` and executed as is (importing
engine/trainer.py needs the whole data / logging stack).  Recorded:

  1. the `auto` decisions: name, lr, momentum and the mutated args.warmup_bias_lr for (nc, iterations) in AUTO_CASES;
  2. optimizer trajectories on the reference's mspa_c2f_gd_yolov8n (nc = 4, seed 0): per iteration the reference loop's warm-up lines
     (yolo/engine/trainer.py:317-326, restated in warmup_lines() below), clip_grad_norm_(10) (:466), optimizer.step() (:467), ModelEMA.update
     (:470) on seeded gradients (optim_inputs.traj_grad, which the tests call too).  `auto` with iterations = 5000 (-> AdamW), 5 iterations,
     snapshots after iterations 1 and 5; name='RMSProp' and name='Adam', 3 iterations, last snapshot;
  3. one_cycle(1, 0.01, 100) at epochs 0, 1, 50, 99.

The GPU box never runs this file.
"""
import ast
import os
import sys
import types

import numpy as np
import torch
from torch import nn, optim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_import  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_  # noqa: E402
from optim_inputs import (AUTO_CASES, ONE_CYCLE_EPOCHS, SAMPLE, TRAJ, TRAJ_ARGS, sample_flat, traj_grad)  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()


def reference_build_optimizer():
    src = open(os.path.join(ref_import.REF, 'yolo/engine/trainer.py')).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == 'BaseTrainer')
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == 'build_optimizer')
    env = {'nn': nn, 'optim': optim, 'LOGGER': types.SimpleNamespace(info=lambda *a, **k: None), 'colorstr': lambda *a: ''}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), 'ref:build_optimizer', 'exec'), env)
    return env['build_optimizer']


def warmup_lines(me, optimizer, ni, nw, epoch, lf):
    """yolo/engine/trainer.py:318-326, restated (self -> me; the accumulate line :320 has no effect at batch = nbs)."""
    if ni <= nw:
        xi = [0, nw]  # x interp
        for j, x in enumerate(optimizer.param_groups):
            # Bias lr falls from 0.1 to lr0, all other lrs rise from 0.0 to lr0
            x['lr'] = np.interp(ni, xi, [me.args.warmup_bias_lr if j == 0 else 0.0, x['initial_lr'] * lf(epoch)])
            if 'momentum' in x:
                x['momentum'] = np.interp(ni, xi, [me.args.warmup_momentum, me.args.momentum])


def main():
    build_optimizer = reference_build_optimizer()
    A = TRAJ_ARGS
    arrs = {}
    # 1. auto
    tiny = nn.Conv2d(1, 1, 1)
    rows = []
    for nc, iterations in AUTO_CASES:
        tiny.nc = nc
        me = types.SimpleNamespace(args=types.SimpleNamespace(warmup_bias_lr=A['warmup_bias_lr']))
        opt = build_optimizer(me, tiny, name='auto', lr=A['lr0'], momentum=A['momentum'], decay=A['weight_decay'], iterations=iterations)
        g = opt.param_groups[0]
        mom = g['momentum'] if 'momentum' in g else g['betas'][0]
        rows.append((type(opt).__name__, g['lr'], mom, me.args.warmup_bias_lr))
        print('auto', nc, iterations, rows[-1])
    arrs['auto_name'] = '\n'.join(r[0] for r in rows)
    arrs['auto_vals'] = np.array([r[1:] for r in rows], np.float64)
    # 3. one_cycle
    oc = ns.torch_utils.one_cycle(1, 0.01, 100)
    arrs['one_cycle'] = np.array([oc(e) for e in ONE_CYCLE_EPOCHS], np.float64)
    # 2. trajectories
    for tag, (name, iterations, n_it, snaps) in TRAJ.items():
        m = ns.tasks.DetectionModel(os.path.join(ref_import.REF, 'models/v8/mspa_c2f_gd_yolov8n.yaml'), nc=A['nc'], verbose=False)
        seed_state_dict_(m, 0)
        m.nc = A['nc']  # attach number of classes to model (set_model_attributes, yolo/v8/detect/train.py:72, runs before build_optimizer)
        m.train()
        me = types.SimpleNamespace(args=types.SimpleNamespace(warmup_bias_lr=A['warmup_bias_lr'], warmup_momentum=A['warmup_momentum'],
                                                              momentum=A['momentum']))
        accumulate = max(round(A['nbs'] / A['batch']), 1)
        decay = A['weight_decay'] * A['batch'] * accumulate / A['nbs']                           # trainer.py:250-251
        opt = build_optimizer(me, m, name=name, lr=A['lr0'], momentum=A['momentum'], decay=decay, iterations=iterations)
        lf = lambda x: (1 - x / A['epochs']) * (1.0 - A['lrf']) + A['lrf']  # linear (trainer.py:263)
        optim.lr_scheduler.LambdaLR(opt, lr_lambda=lf)                                           # trainer.py:264: sets initial_lr
        ema = ns.torch_utils.ModelEMA(m)
        trainable = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
        n_param = sum(p.numel() for _, p in trainable)
        arrs[f'{tag}_names'] = '\n'.join(k for k, _ in trainable)
        arrs[f'{tag}_resolved'] = np.array([opt.param_groups[0]['initial_lr'], me.args.warmup_bias_lr], np.float64)
        arrs[f'{tag}_type'] = type(opt).__name__
        lrs, moms = [], []
        for it in range(n_it):
            warmup_lines(me, opt, it, A['nw'], 0, lf)
            lrs.append([float(g['lr']) for g in opt.param_groups])
            moms.append([float(g['momentum']) if 'momentum' in g else float(g['betas'][0]) for g in opt.param_groups])
            flat = traj_grad(tag, it, n_param)
            off = 0
            for _, p in trainable:
                p.grad = flat[off:off + p.numel()].view(p.shape).clone()
                off += p.numel()
            torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=10.0)                        # trainer.py:466
            opt.step()                                                                           # trainer.py:467
            opt.zero_grad()
            ema.update(m)                                                                        # trainer.py:470
            if it + 1 in snaps:
                esd = dict(ema.ema.named_parameters())
                arrs[f'{tag}_p_{it + 1}'] = sample_flat([p for _, p in trainable]).numpy()
                arrs[f'{tag}_ema_{it + 1}'] = sample_flat([esd[k] for k, _ in trainable]).numpy()
        arrs[f'{tag}_lr'] = np.array(lrs, np.float64)              # (iterations, 3): groups [bias, decay, norm]
        arrs[f'{tag}_mom'] = np.array(moms, np.float64)
        ident = {id(p): k for k, p in m.named_parameters()}
        order = [ident[id(p)] for g in opt.param_groups for p in g['params']]
        sd = opt.state_dict()['state']
        keys = sorted({k for e in sd.values() for k in e if k != 'step'})
        by_name = {order[i]: e for i, e in sd.items()}
        assert set(by_name) == {k for k, _ in trainable}
        for key in keys:
            arrs[f'{tag}_state_{key}'] = sample_flat([by_name[k][key] for k, _ in trainable]).numpy()
        arrs[f'{tag}_state_step'] = np.array(sorted({float(e['step']) for e in sd.values() if 'step' in e}), np.float64)
        print(tag, type(opt).__name__, 'lr', lrs, 'state', keys, 'sampled', arrs[f'{tag}_p_{n_it}'].shape, 'of', n_param, 'SAMPLE', SAMPLE)
    path = os.path.join(HERE, 'optim_traj.npz')
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print(f'optim_traj: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
