"""Generate tests/golden/rtdetr_loss_NN.npz: RT-DETR criterion and validator fixtures from the reference's own Python modules (BUILD CONTAINER ONLY).

    python tests/golden/gen_rtdetr_loss.py

Recipe of gen_rtdetr.py (imported for its harness: ref_import, the `ultralytics.vit` shell packages, the stub cv2, the model builder and the
torch.topk tap).  The outputs come from the reference's HungarianMatcher and RTDETRDetectionLoss (imported as they are) and from
RTDETRValidator.postprocess / update_metrics and DetectionValidator._process_batch / get_stats (taken out of their classes with `ast` and executed as
they are, as gen_golden.py does: importing the validator modules needs the whole dataset / plotting stack).  Only recorded inputs and outputs are
written, no reference program text.  Per case of tests/rtdetr_loss_ref.py:CASES (the inputs are regenerated from the seeds there; their checksums
are recorded):
  - match_indices of every layer as a query-major (l, B, nq) array (the global ground-truth index or -1), from the fp32 run; the .double() run must
    give the same;
  - every entry of the loss dict in fp32 and from the .double() copy; autograd gradients of the summed dict with respect to boxes and logits in
    fp64 (case a: d_logits of the last layer only - the whole tensor is 2.7 MB - the tests pin the restatement on what is recorded and compare the
    device against the restatement), and the largest fp32-vs-fp64 difference per quantity over the WHOLE tensors;
  - the gap per (layer, image): the second-best assignment cost minus the best, every optimal pair forbidden in turn, in float64.
Conditions, asserted: every gap >= GAP_MIN (the generator walks the seed until it holds and prints what it tried; the table's seed must be the one
found); every pair of confidences of the validator case differs.  Case (h): the model of case D of tests/rtdetr_ref.py with `training` set on the
head and its decoder only and num_denoising = 0, the recorded query index forced; then the reference's `loss(batch, preds)` on those predictions.
Case (i): the validator.  The GPU box never runs this file.
"""
import ast
import copy
import glob
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_rtdetr as GR  # noqa: E402  (installs the harness)
import rtdetr_loss_ref as LR  # noqa: E402
import rtdetr_ref as RR  # noqa: E402

ns = GR.ns
import importlib  # noqa: E402
ref_loss = importlib.import_module('ultralytics.vit.utils.loss')
REF = GR.REF


def save(arrs, limit=900 * 1024):
    for old in glob.glob(os.path.join(HERE, 'rtdetr_loss_[0-9][0-9].npz')):
        os.remove(old)
    shards, cur, size = [], {}, 0
    for k, v in arrs.items():
        v = np.asarray(v)
        assert v.dtype != object and v.nbytes <= limit, (k, v.dtype, v.nbytes)
        if size + v.nbytes > limit:
            shards.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    shards.append(cur)
    for n, sh in enumerate(shards):
        path = os.path.join(HERE, f'rtdetr_loss_{n:02d}.npz')
        np.savez_compressed(path, **sh)
        sz = os.path.getsize(path)
        print(f'rtdetr_loss_{n:02d}: {len(sh)} arrays, {sz / 1024:.1f} KiB')
        assert sz < 900 * 1024, f'{path} is {sz} bytes'


class DefaultDtype:
    """with DefaultDtype(dt): the reference in `dt` throughout.  Its criterion creates the target-score buffer in the default dtype and VarifocalLoss
    casts its operands with `.float()`: in the float64 run the default dtype is float64 and Tensor.float converts to float64, so that
    the `.double()` copy is float64 from end to end (the truth the fp32 runs are measured against)."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        torch.set_default_dtype(self.dtype)
        self._float = torch.Tensor.float
        if self.dtype == torch.float64:
            torch.Tensor.float = lambda t, *a, **k: t.double()

    def __exit__(self, *exc):
        torch.Tensor.float = self._float
        torch.set_default_dtype(torch.float32)
        return False


def query_major(match_indices, nq):
    a = np.full((len(match_indices), nq), -1, np.int64)
    for i, (q, g) in enumerate(match_indices):
        a[i, q.long().numpy()] = g.long().numpy()
    return a


def ref_criterion(tag, inp, dtype):
    """the reference's RTDETRDetectionLoss on a case in `dtype` -> (dict of 0-d tensors, match (l, B, nq), leaves)"""
    c = LR.CASES[tag]
    crit = ref_loss.RTDETRDetectionLoss(nc=c['nc'], **{'use_vfl': True, **c['kw']})
    t = lambda k: torch.from_numpy(inp[k]).to(dtype)
    boxes, logits = t('boxes').requires_grad_(), t('logits').requires_grad_()
    batch = {'cls': torch.from_numpy(inp['gt_cls']), 'bboxes': t('gt_boxes'), 'gt_groups': list(c['groups'])}
    kw, leaves = {}, [boxes, logits]
    if 'dn' in c:
        db, dl = t('dn_boxes').requires_grad_(), t('dn_logits').requires_grad_()
        kw = dict(dn_bboxes=db, dn_scores=dl, dn_meta={'dn_pos_idx': [torch.from_numpy(p) for p in inp['dn_pos_idx']], 'dn_num_group': inp['dn_num_group'],
                                                       'dn_num_split': inp['dn_num_split']})
        leaves += [db, dl]
    # the matcher is called per layer inside: record what it returns
    calls = []
    orig = crit.matcher.forward

    def tap(*a, **k):
        r = orig(*a, **k)
        calls.append(r)
        return r
    crit.matcher.forward = tap
    with DefaultDtype(dtype):
        d = crit((boxes, logits), batch, **kw)
    nq, l = c['nq'], c['layers']
    # call order of the reference: the last layer first, then the auxiliary layers (one call for all of them with use_uni_match)
    match = np.full((l, len(c['groups']), nq), -1, np.int64)
    match[-1] = query_major(calls[0], nq)
    if c['kw'].get('use_uni_match'):
        assert len(calls) == 2
        match[:-1] = query_major(calls[1], nq)
    else:
        assert len(calls) == l
        for i in range(l - 1):
            match[i] = query_major(calls[1 + i], nq)
    sum(d.values()).backward()
    return d, match, leaves


def run_case(arrs, tag):
    c = LR.CASES[tag]
    groups, nq = c['groups'], c['nq']
    off = np.concatenate([[0], np.cumsum(groups)])
    seed = c['seed']
    while True:
        inp = LR.make_inputs(tag, seed)
        t64 = lambda k: torch.from_numpy(inp[k])
        C64 = LR.cost_matrix(t64('boxes'), t64('logits'), t64('gt_boxes'), torch.from_numpy(inp['gt_cls'])).numpy()
        gaps = np.full((c['layers'], len(groups)), np.inf)
        for li in range(c['layers']):
            for bi, n in enumerate(groups):
                if n:
                    gaps[li, bi] = LR.gap_of(C64[li, bi][:, off[bi]:off[bi + 1]])
        ok = bool((gaps >= LR.GAP_MIN).all())
        print(f'{tag}: seed {seed}: smallest gap {gaps.min():.3e} ' + ('ok' if ok else f'< {LR.GAP_MIN}: rejected'))
        if ok:
            break
        seed += 1
        assert seed < c['seed'] + 20
    assert seed == c['seed'], f'{tag}: the gap condition holds at seed {seed}, not the table\'s {c["seed"]}: change it'
    d32, m32, g32 = ref_criterion(tag, inp, torch.float32)
    d64, m64, g64 = ref_criterion(tag, inp, torch.float64)
    assert np.array_equal(m32, m64), f'{tag}: fp32 and fp64 match differently'
    arrs[f'{tag}_gap'] = gaps
    arrs[f'{tag}_match'] = m32.astype(np.int32)
    for k in ('boxes', 'logits', 'gt_boxes', 'gt_cls'):
        arrs[f'{tag}_sum_{k}'] = np.array(LR.checksum(inp[k]))
    keys = sorted(d64)
    arrs[f'{tag}_keys'] = np.array(keys)
    arrs[f'{tag}_loss32'] = np.array([float(d32[k]) for k in keys], np.float64)
    arrs[f'{tag}_loss64'] = np.array([float(d64[k]) for k in keys], np.float64)
    names = ['d_boxes', 'd_logits'] + (['dn_d_boxes', 'dn_d_logits'] if 'dn' in c else [])
    dd = {}
    gr = lambda t: torch.zeros_like(t) if t.grad is None else t.grad        # no ground truth at all: the boxes do not reach the loss
    for n, a, b in zip(names, g32, g64):
        dd[n] = float((gr(a).double() - gr(b)).abs().max())
        full = gr(b).numpy()
        arrs[f'{tag}_{n}64'] = full[-1:] if (tag == 'a' and n == 'd_logits') else full
        arrs[f'{tag}_{n}_absmax'] = np.array(float(np.abs(full).max()))
    arrs[f'{tag}_d64'] = np.array([dd[n] for n in names] + [max(abs(float(d32[k]) - float(d64[k])) for k in keys)], np.float64)
    arrs[f'{tag}_loss_d64'] = np.array([abs(float(d32[k]) - float(d64[k])) for k in keys], np.float64)
    print(f'{tag}: losses ' + '  '.join(f'{k} {float(d64[k]):.6f}' for k in keys if float(d64[k]) != 0))
    print(f'{tag}: fp32 vs fp64 ' + '  '.join(f'{n} {v:.3e}' for n, v in dd.items()) + f'  loss {arrs[f"{tag}_d64"][-1]:.3e}')


def method(path, cls_name, name, env):
    src = open(path).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), f'ref:{name}', 'exec'), env)
    return env[name]


def validator(arrs):
    v = LR.VAL
    seed = v['seed']
    while True:
        imgs = LR.make_val_inputs(seed)
        conf = np.concatenate([im['scores'].max(-1) for im in imgs])          # across the images as well: get_stats sorts every row together
        ok = len(np.unique(conf)) == len(conf)
        print(f'i: seed {seed}: confidences ' + ('pairwise distinct' if ok else 'tied: rejected'))
        if ok:
            break
        seed += 1
    assert seed == v['seed']
    from pathlib import Path
    env = {'np': np, 'torch': torch, 'ops': ns.ops, 'box_iou': ns.metrics.box_iou, 'Path': Path}
    rv = os.path.join(REF, 'vit', 'rtdetr', 'val.py')
    dv = os.path.join(REF, 'yolo', 'v8', 'detect', 'val.py')
    post, upd = method(rv, 'RTDETRValidator', 'postprocess', env), method(rv, 'RTDETRValidator', 'update_metrics', env)
    pb, gs = method(dv, 'DetectionValidator', '_process_batch', env), method(dv, 'DetectionValidator', 'get_stats', env)
    me = types.SimpleNamespace(iouv=torch.linspace(0.5, 0.95, 10), niou=10, device=torch.device('cpu'), seen=0, stats=[], nc=v['nc'],
                               args=types.SimpleNamespace(single_cls=False, plots=False, save_json=False, save_txt=False),
                               metrics=ns.metrics.DetMetrics(names={i: str(i) for i in range(v['nc'])}), confusion_matrix=None)
    me._process_batch = lambda det, lab: pb(me, det, lab)
    cls_l, box_l, idx_l = [], [], []
    for si, im in enumerate(imgs):       # one image per call: the images have different query counts
        rows = post(me, (torch.from_numpy(im['boxes'])[None, None].clone(), torch.from_numpy(im['scores'])[None, None].clone()))
        arrs[f'i_rows_{si}'] = rows[0].numpy()
        batch = dict(batch_idx=torch.zeros(len(im['labels'])), cls=torch.from_numpy(im['labels'][:, :1]), bboxes=torch.from_numpy(im['labels'][:, 1:]),
                     ori_shape=[v['ori_shape'][si]])
        upd(me, rows, batch)
        arrs[f'i_correct_{si}'] = me.stats[-1][0].numpy()
        print(f'i: image {si}: {len(rows[0])} rows, true positives per IoU level {me.stats[-1][0].sum(0).tolist()}')
        assert me.stats[-1][0][:, 0].any() and not me.stats[-1][0].all()
    res = gs(me)
    arrs['i_metric_keys'] = np.array(list(res.keys()))
    arrs['i_metrics'] = np.array([float(x) for x in res.values()], np.float64)
    print('i: ' + '  '.join(f'{k} {float(x):.6f}' for k, x in res.items()))
    for si, im in enumerate(imgs):
        for k in ('boxes', 'scores', 'labels'):
            arrs[f'i_sum_{k}_{si}'] = np.array(LR.checksum(im[k]))


def model_level(arrs, tmp):
    tag = 'D'
    _, nc, (b, h, w) = RR.CASES[tag]
    nq, ndl = RR.case_nq_ndl(tag)
    fx = RR.load_fixtures(HERE)
    idx = torch.from_numpy(fx['D_index'])
    m = GR.build(tag, tmp)
    from mgdt_yolo_amd.seeding import seeded_images
    x = seeded_images(b, h, w, seed=RR.IMG_SEED)
    outs = {}
    for name, mm, xx in (('32', m, x), ('64', copy.deepcopy(m).double(), x.double())):
        head = mm.model[-1]
        head.num_denoising = 0
        head.training = True
        head.decoder.training = True
        with torch.no_grad(), GR.TopkTap(idx) as tap:
            o = mm._predict_once(xx)
        head.training = False
        head.decoder.training = False
        assert tap.calls == 1 and o[4] is None and tuple(o[0].shape) == (ndl, b, nq, 4) and tuple(o[1].shape) == (ndl, b, nq, nc)
        outs[name] = o
    assert np.array_equal(outs['32'][0][-1].numpy(), fx['D_dec_bboxes']), 'the last layer is the eval forward'
    wh = torch.tensor([w, h, w, h], dtype=torch.float64)
    for i, k in enumerate(('dec_bboxes', 'dec_scores', 'enc_bboxes', 'enc_scores')):
        arrs[f'h_{k}'] = outs['32'][i].numpy()
        arrs[f'h_{k}64'] = outs['64'][i].numpy()
    arrs['h_d64'] = np.array([float(((outs['32'][0].double() - outs['64'][0]) * wh).abs().max()), float((outs['32'][1].double() - outs['64'][1]).abs().max())])
    print(f'h: fp32 vs fp64: box {arrs["h_d64"][0]:.3e} px, logits {arrs["h_d64"][1]:.3e}')
    # the reference's loss(batch, preds) on these predictions; labels walked until every gap holds
    seed = 0
    while True:
        r = np.random.RandomState(8000 + seed)
        n = 4
        lab = np.concatenate([r.uniform(0.2, 0.8, (n, 2)), r.uniform(0.1, 0.4, (n, 2))], 1).astype(np.float32)
        cls = r.randint(0, nc, (n, 1)).astype(np.float32)
        stack_b = torch.cat([outs['64'][2][None], outs['64'][0]])
        stack_s = torch.cat([outs['64'][3][None], outs['64'][1]])
        C = LR.cost_matrix(stack_b, stack_s, torch.from_numpy(lab).double(), torch.from_numpy(cls[:, 0]).long()).numpy()
        gaps = np.array([LR.gap_of(C[li, 0]) for li in range(C.shape[0])])
        print(f'h: label seed {seed}: smallest gap {gaps.min():.3e}')
        if gaps.min() >= LR.GAP_MIN:
            break
        seed += 1
        assert seed < 20
    arrs['h_labels'] = np.concatenate([cls, lab], 1)
    arrs['h_gap'] = gaps
    for name, mm in (('32', m), ('64', copy.deepcopy(m).double())):
        dt = torch.float32 if name == '32' else torch.float64
        batch = dict(img=torch.zeros(b, 3, h, w, dtype=dt), batch_idx=torch.zeros(n), cls=torch.from_numpy(cls), bboxes=torch.from_numpy(lab).to(dt))
        mm.__dict__.pop('criterion', None)
        mm.nc = nc                            # init_criterion reads self.nc, which the reference's trainer sets on the model
        with DefaultDtype(dt):
            total, items = mm.loss(batch, preds=tuple(t.to(dt) if t is not None else None for t in outs[name]))
        arrs[f'h_loss{name}'] = np.array([float(total)] + [float(v) for v in items], np.float64)
    print(f'h: loss(batch, preds) = {arrs["h_loss64"].tolist()}, fp32 off by {np.abs(arrs["h_loss32"] - arrs["h_loss64"]).max():.3e}')


def main():
    arrs = {}
    for tag in LR.CASES:
        run_case(arrs, tag)
    validator(arrs)
    with tempfile.TemporaryDirectory() as tmp:
        model_level(arrs, tmp)
    save(arrs)


if __name__ == '__main__':
    main()
